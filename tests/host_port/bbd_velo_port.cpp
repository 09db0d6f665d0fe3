// Host port of bbd_velo.hip for the CPU test tier: the same per-point function (bbd_velo_math.h) and the same four
// reductions, run serially in point order.  Same C signature as bbd_velo_depth minus `stream`.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_ragged_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_velo_math.h"

extern "C" int hp_velo_depth_scratch_ints(int total_pixels, int n_frames) {
  if (total_pixels < 0 || n_frames < 0 || total_pixels > 0x7fffffff / 4) return BBD_E_TOOMANY;
  return 4 * total_pixels;
}

extern "C" int hp_velo_depth(const float* points, const int32_t* desc, const double* proj, int32_t* scratch,
                             int scratch_ints, float* out, int n_frames, int max_points, int flags) {
  if (!desc || !proj || !scratch || !out || n_frames <= 0 || max_points < 0 || scratch_ints < 0 ||
      (!points && max_points > 0) || (flags & ~BBD_VELO_VEL_DEPTH))
    return BBD_E_BADARG;
  const int vel_depth = (flags & BBD_VELO_VEL_DEPTH) ? 1 : 0;
  std::memset(scratch, 0, (size_t)scratch_ints * sizeof(int32_t));
  for (int f = 0; f < n_frames; ++f) {
    const int32_t* d = desc + (size_t)f * BBD_VELO_DESC;
    const size_t off = bbd_join64(d[0], d[1]);
    const int h = d[2], w = d[3], n = d[4];
    const long poff = d[5], soff = d[6], npx = (long)h * w;
    if (h < 1 || w < 1 || n < 0 || n > max_points || poff < 0 || soff < 0 || 4 * (soff + npx) > scratch_ints) return BBD_E_BADARG;
    const float* pts = points + 4 * poff;
    const double* P = proj + (size_t)f * 12;
    uint32_t* last = reinterpret_cast<uint32_t*>(scratch) + 4 * soff;
    uint32_t *first = last + npx, *count = first + npx, *least = count + npx;
    bbd_velo_hit_t hit;
    for (uint32_t i = 0; i < (uint32_t)n; ++i) {
      if (!bbd_velo_project(P, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], h, w, vel_depth, &hit)) continue;
      last[hit.pixel] = std::max(last[hit.pixel], i + 1u);
      first[hit.key] = std::max(first[hit.key], ~i);
      count[hit.key] += 1u;
      least[hit.key] = std::max(least[hit.key], ~bbd_viz_order_key(hit.depth));
    }
    for (long p = 0; p < npx; ++p) {
      float v = 0.0f;
      const uint32_t l = last[p];
      if (l && bbd_velo_project(P, pts[4 * (l - 1)], pts[4 * (l - 1) + 1], pts[4 * (l - 1) + 2], h, w, vel_depth, &hit)) v = hit.depth;
      const int r = (int)(p / w), c = (int)(p - (long)r * w);
      const int32_t key = bbd_velo_key(r, c, w);
      if (count[key] > 1u) {
        const uint32_t i = ~first[key];
        if (bbd_velo_project(P, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], h, w, vel_depth, &hit) && hit.pixel == (int32_t)p)
          v = bbd_viz_key_value(~least[key]);
      }
      out[off + p] = bbd_velo_finish(v);
    }
  }
  return 0;
}
