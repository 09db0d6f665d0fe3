// bbd_view.hip - a rasteriser: points (the 16-byte vertex records of bbd_point_cloud and bbd_map_finish) and polylines
// (trajectories) go into a caller-owned z-buffered canvas of 64-bit cells, which is then resolved to RGB bytes
// (pointcloud.Canvas, evaluate_pose.py --save_plot, test_simple.py --cloud_view).
//
// A cell holds ONE key, rank << 32 | colour, and every write is an unsigned 64-bit atomicMin: the smallest key offered
// to a cell is what it ends with, whatever the order of lanes, launches and calls.  The projection, the keys, the
// footprint of a point, the box of a segment and the distance of a pixel from it are bbd_view_math.h, shared with the
// host port.  What is here:
//
//   clear    view_clear_kernel    every cell = empty (all ones), counters = 0
//   points   view_points_kernel   a lane per vertex, striding over min(*count, n_max) of them (count is read in the
//                                 kernel; records past it are never read).  Project, classify, then one atomicMin per
//                                 pixel of the footprint.  The four counters are summed per lane, then per wave: one
//                                 atomicAdd per wave and counter.
//   lines    view_lines_kernel    a WAVE per segment, striding over the segments; the segment's box, cut to the canvas,
//                                 is spread over the 64 lanes, each pixel tests its distance and offers the overlay key.
//                                 The work of a segment is its box on the canvas, wherever its ends lie.
//   resolve  view_resolve_kernel  a lane per four neighbouring pixels: 32 bytes of cells in, 12 bytes of colour out
//
// Before an atomicMin the cell is loaded (relaxed): keys only decrease, so a cell that already holds a key <= the lane's
// own can be left alone.  Plain vector global atomics at agent scope; no float atomics, no inline assembly.
// No allocation, no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_view_math.h"

namespace {

typedef unsigned long long u64;

constexpr int VT = 256;               // threads of every kernel here
constexpr long MAX_GRID = 4096;       // work beyond this is reached by striding

struct PointsCall {
  u64* cells;
  u64* counters;
  const uint4* vertices;
  const int32_t* count;
  const double* view;
  int H, W, n_max, size;
};

struct LinesCall {
  u64* cells;
  const double* xyz;
  const double* view;
  u64 key;
  double r2, r;
  int H, W, P, segments;
};

__global__ __launch_bounds__(VT) void view_clear_kernel(u64* cells, u64* counters, long n) {
  for (long c = blockIdx.x * (long)VT + threadIdx.x; c < n; c += (long)gridDim.x * VT) cells[c] = BBD_VIEW_EMPTY;
  if (blockIdx.x == 0 && threadIdx.x < BBD_VIEW_COUNTERS) counters[threadIdx.x] = 0;
}

__device__ __forceinline__ void offer(u64* cell, u64 key) {
  if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(cell, key);
}

__device__ __forceinline__ u64 wave_count(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(VT) void view_points_kernel(PointsCall a) {
  long n = a.n_max;
  if (a.count) {
    const long given = *a.count;
    n = given < 0 ? 0 : (given < n ? given : n);
  }
  double V[16];
  for (int k = 0; k < 16; ++k) V[k] = a.view[k];
  u64 drawn = 0, clipped = 0, rejected = 0;
  for (long g = blockIdx.x * (long)VT + threadIdx.x; g < n; g += (long)gridDim.x * VT) {
    const uint4 rec = a.vertices[g];
    BbdViewProj p;
    const int verdict = bbd_view_project(V, (double)__uint_as_float(rec.x), (double)__uint_as_float(rec.y),
                                         (double)__uint_as_float(rec.z), &p);
    if (verdict == BBD_VIEW_REJECTED) {
      ++rejected;
      continue;
    }
    BbdViewBox b;
    if (verdict == BBD_VIEW_BEHIND || !bbd_view_footprint(&p, a.size, a.H, a.W, &b)) {
      ++clipped;
      continue;
    }
    ++drawn;
    const u64 key = bbd_view_point_key(p.d, rec.w);
    for (int y = b.y0; y <= b.y1; ++y)                       // 0 <= y < H and 0 <= x < W: bbd_view_cut
      for (int x = b.x0; x <= b.x1; ++x) offer(a.cells + ((size_t)y * a.W + x), key);
  }
  drawn = wave_count(drawn);
  clipped = wave_count(clipped);
  rejected = wave_count(rejected);
  if ((threadIdx.x & 63) == 0) {
    if (drawn) atomicAdd(a.counters + 1, drawn);
    if (clipped) atomicAdd(a.counters + 2, clipped);
    if (rejected) atomicAdd(a.counters + 3, rejected);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(a.counters, (u64)n);
}

__global__ __launch_bounds__(VT) void view_lines_kernel(LinesCall a) {
  const int lane = threadIdx.x & 63;
  const long wave = (blockIdx.x * (long)VT + threadIdx.x) >> 6, waves = ((long)gridDim.x * VT) >> 6;
  double V[16];
  for (int k = 0; k < 16; ++k) V[k] = a.view[k];
  for (long s = wave; s < a.segments; s += waves) {          // uniform over the wave
    const double* pa = a.xyz + 3 * s;
    const double* pb = a.xyz + 3 * ((s + 1) % a.P);          // P = 1: the vertex itself; the closing segment: vertex 0
    BbdViewProj qa, qb;
    if (bbd_view_project(V, pa[0], pa[1], pa[2], &qa) != BBD_VIEW_FRONT) continue;
    if (bbd_view_project(V, pb[0], pb[1], pb[2], &qb) != BBD_VIEW_FRONT) continue;
    BbdViewBox b;
    if (!bbd_view_segment_box(&qa, &qb, a.r, a.H, a.W, &b)) continue;
    const long bw = b.x1 - b.x0 + 1, cells = bw * (b.y1 - b.y0 + 1);       // <= H * W <= 2^28
    for (long c = lane; c < cells; c += 64) {
      const int y = b.y0 + (int)(c / bw), x = b.x0 + (int)(c % bw);
      if (bbd_view_dist2(x, y, qa.u, qa.v, qb.u, qb.v) <= a.r2) offer(a.cells + ((size_t)y * a.W + x), a.key);
    }
  }
}

__global__ __launch_bounds__(VT) void view_resolve_kernel(const u64* cells, long n, uint32_t background, uint8_t* out,
                                                          bool aligned) {
  const long quads = (n + 3) / 4;
  for (long q = blockIdx.x * (long)VT + threadIdx.x; q < quads; q += (long)gridDim.x * VT) {
    const long first = 4 * q;
    const uint32_t cnt = (uint32_t)(n - first < 4 ? n - first : 4);
    uint32_t c[4];
    for (uint32_t k = 0; k < cnt; ++k) c[k] = bbd_view_cell_rgb(cells[first + k], background);
    store_quad(out + 3 * first, aligned, cnt, c);
  }
}

unsigned grid_for(long items, int threads) {
  const long blocks = (items + threads - 1) / threads;
  return (unsigned)(blocks < 1 ? 1 : blocks < MAX_GRID ? blocks : MAX_GRID);
}

}  // namespace

extern "C" int bbd_view_clear(uint64_t* cells, int64_t* counters, int H, int W, void* stream) {
  const int rc = bbd_view_canvas_status(cells, H, W);
  if (rc) return rc;
  if (!counters) return BBD_E_BADARG;
  const long n = (long)H * W;
  hipLaunchKernelGGL(view_clear_kernel, dim3(grid_for(n, VT)), dim3(VT), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<u64*>(cells), reinterpret_cast<u64*>(counters), n);
  return launch_status();
}

extern "C" int bbd_view_points(uint64_t* cells, int64_t* counters, int H, int W, const void* vertices,
                               const int32_t* count, int n_max, const double* view, int size, void* stream) {
  const int rc = bbd_view_points_status(cells, counters, H, W, vertices, n_max, view, size);
  if (rc) return rc;
  if (n_max == 0) return 0;
  PointsCall a;
  a.cells = reinterpret_cast<u64*>(cells); a.counters = reinterpret_cast<u64*>(counters);
  a.vertices = static_cast<const uint4*>(vertices); a.count = count; a.view = view;
  a.H = H; a.W = W; a.n_max = n_max; a.size = size;
  hipLaunchKernelGGL(view_points_kernel, dim3(grid_for(n_max, VT)), dim3(VT), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

extern "C" int bbd_view_lines(uint64_t* cells, int64_t* counters, int H, int W, const double* xyz, int P,
                              const double* view, int rgb, double width, int layer, int closed, void* stream) {
  const int rc = bbd_view_lines_status(cells, counters, H, W, xyz, P, view, rgb, width, layer, closed);
  if (rc) return rc;
  LinesCall a;
  a.cells = reinterpret_cast<u64*>(cells); a.xyz = xyz; a.view = view;
  a.key = bbd_view_overlay_key(layer, rgb);
  a.r = width / 2.0; a.r2 = a.r * a.r;
  a.H = H; a.W = W; a.P = P; a.segments = bbd_view_segments(P, closed);
  hipLaunchKernelGGL(view_lines_kernel, dim3(grid_for((long)a.segments * 64, VT)), dim3(VT), 0,
                     static_cast<hipStream_t>(stream), a);
  return launch_status();
}

extern "C" int bbd_view_resolve(const uint64_t* cells, int H, int W, int background_rgb, uint8_t* out, void* stream) {
  const int rc = bbd_view_canvas_status(cells, H, W);
  if (rc) return rc;
  if (!out || background_rgb < 0 || background_rgb > 0xffffff) return BBD_E_BADARG;
  const long n = (long)H * W;
  hipLaunchKernelGGL(view_resolve_kernel, dim3(grid_for((n + 3) / 4, VT)), dim3(VT), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const u64*>(cells), n, (uint32_t)background_rgb, out, ((uintptr_t)out & 3) == 0);
  return launch_status();
}
