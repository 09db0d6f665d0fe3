// bbd_map.hip - a scene map fused on a voxel grid: the points of many frames, each placed in the world by its pose, are
// summed per voxel in a caller-owned open-addressing hash table and finished into 16-byte PLY vertices, one per voxel
// (pointcloud.SceneMap, evaluate_pose.py --save_map).
//
// What a candidate pixel becomes - its voxel key, the 16-bit offsets inside the voxel, its colour bytes - the hash and
// the vertex of a finished voxel are bbd_map_math.h, shared with the host port.  What is here:
//
//   clear       map_clear_kernel       every key = empty (all ones), sums and counters = 0
//   accumulate  map_accumulate_kernel  a lane per candidate, striding over the call's n * cap candidates.  A kept point
//                                      probes linearly from hash(key) & (T - 1): a relaxed load of the slot's key, a
//                                      64-bit atomicCAS(empty -> key) where it reads empty; the slot is the point's when
//                                      either returns its key.  A key, once written, never changes, so a stale load can
//                                      only send a lane to the CAS.  The probe is a for loop of T iterations: a full
//                                      table ends it, the point is counted as dropped.  On the slot: three 64-bit and
//                                      four 32-bit no-return atomicAdd (q_x q_y q_z; r g b 1).  By default a run of
//                                      neighbouring lanes with one key is summed in the wave first and its first lane
//                                      adds for all (BBD_MAP_NO_MERGE: every point adds for itself; same bytes).  The
//                                      call's counters are summed per lane, then per wave: one atomicAdd per wave.
//   finish      map_count_kernel, map_scan_kernel, map_write_kernel: the compaction of bbd_compact.h over the T slots in
//                                      chunks of 256; a slot is kept when it is occupied and count >= min_points.
//
// Only integers are added, so the sums do not depend on the order of arrival.  Which SLOT a key takes does (it depends
// on who wins a CAS), and with it the order of bbd_map_finish's output: out_keys is there so that the caller can put the
// voxels in key order, which is unique.  Plain vector global atomics at agent scope; no inline assembly.
// No allocation, no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_compact.h"
#include "bbd_device_util.h"
#include "bbd_map_math.h"

namespace {

typedef unsigned long long u64;

constexpr int AT = 256;               // threads of the clear and accumulate kernels
constexpr int CT = BBD_MAP_CHUNK;     // threads of the count and write kernels: one slot each
constexpr int CW = CT / 64;
constexpr int ST = 1024;              // threads of the scan kernel
constexpr int SW = ST / 64;
constexpr long MAX_GRID = 4096;       // work beyond this is reached by striding

struct MapCall {
  BbdMapParams p;
  u64* keys;          // [T]
  u64* pos;           // [T,3]
  uint32_t* col;      // [T,4]
  u64* counters;      // [BBD_MAP_COUNTERS]
  int T;
};

struct FinishCall {
  const u64* keys;
  const u64* pos;
  const uint32_t* col;
  int64_t* out_keys;
  uint4* vertices;
  int32_t* out_counts;
  int32_t* m;
  int32_t* chunks;
  double voxel;
  int T, min_points;
};

__global__ __launch_bounds__(AT) void map_clear_kernel(u64* keys, u64* pos, uint32_t* col, u64* counters, int T) {
  for (long s = blockIdx.x * (long)AT + threadIdx.x; s < T; s += (long)gridDim.x * AT) {
    keys[s] = BBD_MAP_EMPTY;
    pos[3 * s] = 0; pos[3 * s + 1] = 0; pos[3 * s + 2] = 0;
    reinterpret_cast<uint4*>(col)[s] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (blockIdx.x == 0 && threadIdx.x < BBD_MAP_COUNTERS) counters[threadIdx.x] = 0;
}

// The slot of `key`, or -1 when all T slots hold other keys.
__device__ __forceinline__ int map_slot(u64* keys, int T, u64 key) {
  int slot = (int)(bbd_map_hash(key) & (u64)(T - 1));
  for (int it = 0; it < T; ++it) {
    u64 seen = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == BBD_MAP_EMPTY) seen = atomicCAS(keys + slot, (u64)BBD_MAP_EMPTY, key);
    if (seen == BBD_MAP_EMPTY || seen == key) return slot;
    slot = (slot + 1) & (T - 1);
  }
  return -1;
}

__device__ __forceinline__ u64 wave_count(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// The sums of one point, or of a run of points of one voxel, onto the voxel's slot.
__device__ __forceinline__ void map_add(const MapCall& a, int slot, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t r,
                                        uint32_t g, uint32_t b, uint32_t count) {
  u64* pos = a.pos + 3 * (size_t)slot;
  uint32_t* col = a.col + 4 * (size_t)slot;
  atomicAdd(pos, (u64)q0);
  atomicAdd(pos + 1, (u64)q1);
  atomicAdd(pos + 2, (u64)q2);
  atomicAdd(col, r);
  atomicAdd(col + 1, g);
  atomicAdd(col + 2, b);
  atomicAdd(col + 3, count);
}

// MERGE: neighbouring lanes of a wave are neighbouring pixels of a row and often fall into one voxel (road, walls).  A
// run of kept lanes with equal keys is summed inside the wave - a segmented suffix sum by shuffles, six steps, of five
// words: q_x, q_y, q_z (at most 64 * 65536 each), r | g << 16 and b | count << 16 (at most 64 * 255 and 64) - and the
// run's first lane alone probes and adds.  Integer sums: the state's bytes are those of the plain form.
template <bool MERGE>
__global__ __launch_bounds__(AT) void map_accumulate_kernel(MapCall a) {
  const double scale = a.p.scale ? *a.p.scale : 1.0;
  const long cap = (long)a.p.ncy * a.p.ncx, total = (long)a.p.n * cap;        // <= n h w <= INT_MAX
  const int lane = threadIdx.x & 63;
  u64 kept = 0, out_of_range = 0, full = 0;
  // g0 is the wave's first candidate: the loop is uniform over the wave, the last wave's tail lanes idle inside it
  for (long g0 = blockIdx.x * (long)AT + (threadIdx.x - lane); g0 < total; g0 += (long)gridDim.x * AT) {
    const long g = g0 + lane;
    BbdMapPoint pt = {BBD_MAP_EMPTY, {0u, 0u, 0u}, {0u, 0u, 0u}};
    int verdict = BBD_MAP_REJECTED;
    if (g < total) {
      const int i = (int)(g / cap), c = (int)(g - (long)i * cap);
      verdict = bbd_map_point(&a.p, scale, i, c, &pt);
    }
    if (verdict == BBD_MAP_OUT_OF_RANGE) ++out_of_range;
    const bool valid = verdict == BBD_MAP_KEPT;
    const u64 key = valid ? pt.key : BBD_MAP_EMPTY;                            // no kept point has the empty key
    uint32_t q0 = pt.q[0], q1 = pt.q[1], q2 = pt.q[2], rg = pt.rgb[0] | (pt.rgb[1] << 16), bc = pt.rgb[2] | (1u << 16);
    bool head = valid;
    if (MERGE) {
      const u64 before = __shfl_up(key, 1, 64);
      head = valid && (lane == 0 || before != key);
      const unsigned long long heads = __ballot(head);
      // the run a lane belongs to: heads at or below it; lanes that are not kept get run 0, which no kept lane has
      const int run = valid ? __popcll(heads & (~0ull >> (63 - lane))) : 0;
      for (int o = 1; o < 64; o <<= 1) {
        const int other = __shfl_down(run, o, 64);
        const uint32_t t0 = __shfl_down(q0, o, 64), t1 = __shfl_down(q1, o, 64), t2 = __shfl_down(q2, o, 64);
        const uint32_t t3 = __shfl_down(rg, o, 64), t4 = __shfl_down(bc, o, 64);
        if (lane + o < 64 && other == run) {
          q0 += t0; q1 += t1; q2 += t2; rg += t3; bc += t4;
        }
      }
    }
    if (!head) continue;
    const uint32_t count = bc >> 16;
    const int slot = map_slot(a.keys, a.T, key);                               // < T, or -1
    if (slot < 0) {
      full += count;
      continue;
    }
    kept += count;
    map_add(a, slot, q0, q1, q2, rg & 0xffffu, rg >> 16, bc & 0xffffu, count);
  }
  kept = wave_count(kept);
  out_of_range = wave_count(out_of_range);
  full = wave_count(full);
  if (lane == 0) {
    if (kept) atomicAdd(a.counters + 1, kept);
    if (out_of_range) atomicAdd(a.counters + 2, out_of_range);
    if (full) atomicAdd(a.counters + 3, full);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.counters, (u64)total);
}

__device__ __forceinline__ bool map_keep(const FinishCall& a, int s) {
  return s < a.T && a.keys[s] != BBD_MAP_EMPTY && a.col[4 * (size_t)s + 3] >= (uint32_t)a.min_points;
}

__global__ __launch_bounds__(CT) void map_count_kernel(FinishCall a) {
  __shared__ int wave_kept[CW];
  const int n_chunks = bbd_map_chunks(a.T);
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {         // uniform over the workgroup
    compact_ballot(map_keep(a, chunk * CT + (int)threadIdx.x), wave_kept);
    __syncthreads();
    if (threadIdx.x == 0) a.chunks[chunk] = compact_total<CW>(wave_kept);
    __syncthreads();
  }
}

__global__ __launch_bounds__(ST) void map_scan_kernel(FinishCall a) {
  __shared__ int wave_total[SW];
  compact_scan<ST>(a.chunks, bbd_map_chunks(a.T), wave_total, a.m);
}

__global__ __launch_bounds__(CT) void map_write_kernel(FinishCall a) {
  __shared__ int wave_kept[CW];
  const int n_chunks = bbd_map_chunks(a.T);
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int s = chunk * CT + (int)threadIdx.x;
    const bool keep = map_keep(a, s);
    const unsigned long long mask = compact_ballot(keep, wave_kept);
    __syncthreads();
    if (keep) {
      const int slot = compact_slot(a.chunks[chunk], mask, wave_kept);         // < *m <= T
      const uint4 c = reinterpret_cast<const uint4*>(a.col)[s];
      const uint32_t col[4] = {c.x, c.y, c.z, c.w};
      const uint64_t sums[3] = {a.pos[3 * (size_t)s], a.pos[3 * (size_t)s + 1], a.pos[3 * (size_t)s + 2]};
      uint32_t v[4];
      bbd_map_vertex(a.keys[s], sums, col, a.voxel, v);
      a.out_keys[slot] = (int64_t)a.keys[s];
      a.vertices[slot] = make_uint4(v[0], v[1], v[2], v[3]);
      a.out_counts[slot] = (int32_t)c.w;
    }
    __syncthreads();
  }
}

unsigned grid_for(long items, int threads) {
  const long blocks = (items + threads - 1) / threads;
  return (unsigned)(blocks < 1 ? 1 : blocks < MAX_GRID ? blocks : MAX_GRID);
}

}  // namespace

extern "C" long bbd_map_state_bytes(int T) {
  if (T < 1) return BBD_E_BADARG;
  if (T > BBD_MAP_MAX_T) return BBD_E_TOOMANY;
  if (!bbd_map_pow2(T)) return BBD_E_BADARG;
  return (long)T * BBD_MAP_SLOT_BYTES + BBD_MAP_COUNTERS * 8L;
}

extern "C" int bbd_map_finish_scratch_ints(int T) {
  if (T < 1) return BBD_E_BADARG;
  if (T > BBD_MAP_MAX_T) return BBD_E_TOOMANY;
  return bbd_map_pow2(T) ? bbd_map_chunks(T) : BBD_E_BADARG;
}

extern "C" int bbd_map_clear(uint64_t* keys, uint64_t* pos, uint32_t* col, int64_t* counters, int T, void* stream) {
  const int rc = bbd_map_state_status(keys, pos, col, T);
  if (rc) return rc;
  if (!counters || ((uintptr_t)col & 15) != 0) return BBD_E_BADARG;
  hipLaunchKernelGGL(map_clear_kernel, dim3(grid_for(T, AT)), dim3(AT), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<u64*>(keys), reinterpret_cast<u64*>(pos), col, reinterpret_cast<u64*>(counters), T);
  return launch_status();
}

extern "C" int bbd_map_accumulate(uint64_t* keys, uint64_t* pos, uint32_t* col, int64_t* counters, int T,
                                  const float* disp, const float* rgb, const double* poses, const float* inv_K,
                                  const double* scale, int n, int h, int w, int r0, int r1, int c0, int c1, int stride,
                                  double min_depth, double max_depth, double voxel, int flags, void* stream) {
  int rc = bbd_map_state_status(keys, pos, col, T);
  if (rc) return rc;
  rc = bbd_map_accumulate_status(counters, disp, rgb, poses, inv_K, n, h, w, stride, min_depth, max_depth, voxel, flags);
  if (rc) return rc;
  MapCall a;
  a.p.disp = disp; a.p.rgb = rgb; a.p.poses = poses; a.p.inv_K = inv_K; a.p.scale = scale;
  a.p.n = n; a.p.h = h; a.p.w = w; a.p.stride = stride; a.p.flags = flags;
  a.p.lo = min_depth; a.p.hi = max_depth; a.p.voxel = voxel;
  bbd_map_grid(h, w, r0, r1, c0, c1, stride, &a.p);
  a.keys = reinterpret_cast<u64*>(keys); a.pos = reinterpret_cast<u64*>(pos); a.col = col;
  a.counters = reinterpret_cast<u64*>(counters); a.T = T;
  const long total = (long)n * a.p.ncy * a.p.ncx;
  if (total == 0) return 0;                                                    // the window misses the image
  const dim3 grid(grid_for(total, AT));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (flags & BBD_MAP_NO_MERGE) {
    hipLaunchKernelGGL(map_accumulate_kernel<false>, grid, dim3(AT), 0, st, a);
  } else {
    hipLaunchKernelGGL(map_accumulate_kernel<true>, grid, dim3(AT), 0, st, a);
  }
  return launch_status();
}

extern "C" int bbd_map_finish(const uint64_t* keys, const uint64_t* pos, const uint32_t* col, int T, int min_points,
                              double voxel, int64_t* out_keys, void* vertices, int32_t* out_counts, int32_t* m,
                              int32_t* scratch, int scratch_ints, void* stream) {
  const int rc = bbd_map_state_status(keys, pos, col, T);
  if (rc) return rc;
  if (!out_keys || !vertices || !out_counts || !m || !scratch || min_points < 1) return BBD_E_BADARG;
  if (!(voxel > 0.0) || !bbd_map_finite(voxel)) return BBD_E_BADARG;
  if (((uintptr_t)vertices & (BBD_CLOUD_VERTEX - 1)) != 0 || ((uintptr_t)col & 15) != 0) return BBD_E_BADARG;
  if (scratch_ints < bbd_map_chunks(T)) return BBD_E_BADARG;
  FinishCall a;
  a.keys = reinterpret_cast<const u64*>(keys); a.pos = reinterpret_cast<const u64*>(pos); a.col = col;
  a.out_keys = out_keys; a.vertices = static_cast<uint4*>(vertices); a.out_counts = out_counts; a.m = m;
  a.chunks = scratch; a.voxel = voxel; a.T = T; a.min_points = min_points;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(grid_for(T, CT));
  hipLaunchKernelGGL(map_count_kernel, grid, dim3(CT), 0, st, a);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(ST), 0, st, a);
  hipLaunchKernelGGL(map_write_kernel, grid, dim3(CT), 0, st, a);
  return launch_status();
}
