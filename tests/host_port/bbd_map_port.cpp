// Host port of bbd_map.hip for the CPU test tier: the argument rules, the candidate grid, what a candidate becomes, the
// hash and the vertex are bbd_map_math.h, shared with the kernels; the probe, the sums and the compaction are serial
// loops here.  Same C signatures as the bbd_map_* entries minus `stream`, plus hp_map_points, which hands out what
// bbd_map_point made of every candidate (the tests' fusion stage starts from it).
#include <cstdint>
#include <cstring>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_map_math.h"

extern "C" long hp_map_state_bytes(int T) {
  if (T < 1) return BBD_E_BADARG;
  if (T > BBD_MAP_MAX_T) return BBD_E_TOOMANY;
  if (!bbd_map_pow2(T)) return BBD_E_BADARG;
  return (long)T * BBD_MAP_SLOT_BYTES + BBD_MAP_COUNTERS * 8L;
}

extern "C" int hp_map_finish_scratch_ints(int T) {
  if (T < 1) return BBD_E_BADARG;
  if (T > BBD_MAP_MAX_T) return BBD_E_TOOMANY;
  return bbd_map_pow2(T) ? bbd_map_chunks(T) : BBD_E_BADARG;
}

extern "C" int hp_map_clear(uint64_t* keys, uint64_t* pos, uint32_t* col, int64_t* counters, int T) {
  const int rc = bbd_map_state_status(keys, pos, col, T);
  if (rc) return rc;
  if (!counters || ((uintptr_t)col & 15) != 0) return BBD_E_BADARG;
  for (long s = 0; s < T; ++s) keys[s] = BBD_MAP_EMPTY;
  memset(pos, 0, (size_t)T * 24);
  memset(col, 0, (size_t)T * 16);
  memset(counters, 0, BBD_MAP_COUNTERS * 8);
  return 0;
}

static int fill(BbdMapParams* a, const float* disp, const float* rgb, const double* poses, const float* inv_K,
                const double* scale, int n, int h, int w, int r0, int r1, int c0, int c1, int stride, double min_depth,
                double max_depth, double voxel, int flags) {
  a->disp = disp; a->rgb = rgb; a->poses = poses; a->inv_K = inv_K; a->scale = scale;
  a->n = n; a->h = h; a->w = w; a->stride = stride; a->flags = flags;
  a->lo = min_depth; a->hi = max_depth; a->voxel = voxel;
  bbd_map_grid(h, w, r0, r1, c0, c1, stride, a);
  return a->ncy * a->ncx;
}

extern "C" int hp_map_accumulate(uint64_t* keys, uint64_t* pos, uint32_t* col, int64_t* counters, int T,
                                 const float* disp, const float* rgb, const double* poses, const float* inv_K,
                                 const double* scale, int n, int h, int w, int r0, int r1, int c0, int c1, int stride,
                                 double min_depth, double max_depth, double voxel, int flags) {
  int rc = bbd_map_state_status(keys, pos, col, T);
  if (rc) return rc;
  rc = bbd_map_accumulate_status(counters, disp, rgb, poses, inv_K, n, h, w, stride, min_depth, max_depth, voxel, flags);
  if (rc) return rc;
  BbdMapParams a;
  const int cap = fill(&a, disp, rgb, poses, inv_K, scale, n, h, w, r0, r1, c0, c1, stride, min_depth, max_depth, voxel,
                       flags);
  const double s = scale ? *scale : 1.0;
  for (int i = 0; i < n; ++i) {
    for (int c = 0; c < cap; ++c) {
      BbdMapPoint pt;
      const int verdict = bbd_map_point(&a, s, i, c, &pt);
      counters[0] += 1;
      if (verdict == BBD_MAP_OUT_OF_RANGE) counters[2] += 1;
      if (verdict != BBD_MAP_KEPT) continue;
      int slot = (int)(bbd_map_hash(pt.key) & (uint64_t)(T - 1)), found = -1;
      for (int it = 0; it < T; ++it) {
        if (keys[slot] == BBD_MAP_EMPTY) keys[slot] = pt.key;
        if (keys[slot] == pt.key) {
          found = slot;
          break;
        }
        slot = (slot + 1) & (T - 1);
      }
      if (found < 0) {
        counters[3] += 1;
        continue;
      }
      counters[1] += 1;
      for (int j = 0; j < 3; ++j) pos[3 * (size_t)found + j] += pt.q[j];
      for (int j = 0; j < 3; ++j) col[4 * (size_t)found + j] += pt.rgb[j];
      col[4 * (size_t)found + 3] += 1;
    }
  }
  return 0;
}

extern "C" int hp_map_finish(const uint64_t* keys, const uint64_t* pos, const uint32_t* col, int T, int min_points,
                             double voxel, int64_t* out_keys, void* vertices, int32_t* out_counts, int32_t* m,
                             int32_t* scratch, int scratch_ints) {
  const int rc = bbd_map_state_status(keys, pos, col, T);
  if (rc) return rc;
  if (!out_keys || !vertices || !out_counts || !m || !scratch || min_points < 1) return BBD_E_BADARG;
  if (!(voxel > 0.0) || !bbd_map_finite(voxel)) return BBD_E_BADARG;
  if (((uintptr_t)vertices & (BBD_CLOUD_VERTEX - 1)) != 0 || ((uintptr_t)col & 15) != 0) return BBD_E_BADARG;
  if (scratch_ints < bbd_map_chunks(T)) return BBD_E_BADARG;
  int kept = 0;
  for (long s = 0; s < T; ++s) {
    if (keys[s] == BBD_MAP_EMPTY || col[4 * s + 3] < (uint32_t)min_points) continue;
    uint32_t v[4];
    bbd_map_vertex(keys[s], pos + 3 * s, col + 4 * s, voxel, v);
    out_keys[kept] = (int64_t)keys[s];
    memcpy(static_cast<uint8_t*>(vertices) + (size_t)kept * BBD_CLOUD_VERTEX, v, BBD_CLOUD_VERTEX);
    out_counts[kept] = (int32_t)col[4 * s + 3];
    ++kept;
  }
  *m = kept;
  return 0;
}

// What every candidate of a call becomes, in candidate order: verdict int32 [n * cap] (BBD_MAP_REJECTED / _KEPT /
// _OUT_OF_RANGE), and for the kept ones key int64, q uint32 [.,3], rgb uint32 [.,3].  Returns n * cap, or the status.
extern "C" int hp_map_points(const float* disp, const float* rgb, const double* poses, const float* inv_K,
                             const double* scale, int n, int h, int w, int r0, int r1, int c0, int c1, int stride,
                             double min_depth, double max_depth, double voxel, int flags, int32_t* verdict,
                             int64_t* key, uint32_t* q, uint32_t* colour) {
  int64_t dummy = 0;
  const int rc = bbd_map_accumulate_status(&dummy, disp, rgb, poses, inv_K, n, h, w, stride, min_depth, max_depth, voxel,
                                           flags);
  if (rc) return rc;
  BbdMapParams a;
  const int cap = fill(&a, disp, rgb, poses, inv_K, scale, n, h, w, r0, r1, c0, c1, stride, min_depth, max_depth, voxel,
                       flags);
  const double s = scale ? *scale : 1.0;
  for (int i = 0; i < n; ++i) {
    for (int c = 0; c < cap; ++c) {
      const size_t g = (size_t)i * cap + c;
      BbdMapPoint pt;
      verdict[g] = bbd_map_point(&a, s, i, c, &pt);
      if (verdict[g] != BBD_MAP_KEPT) continue;
      key[g] = (int64_t)pt.key;
      for (int j = 0; j < 3; ++j) q[3 * g + j] = pt.q[j];
      for (int j = 0; j < 3; ++j) colour[3 * g + j] = pt.rgb[j];
    }
  }
  return n * cap;
}
