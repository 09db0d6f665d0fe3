// Host port of bbd_view.hip for the CPU test tier: the argument rules, the projection, the keys, the footprint, the
// segment box and the pixel distance are bbd_view_math.h, shared with the kernels; the atomic minimum is a comparison
// and the launches are serial loops here.  Same C signatures as the bbd_view_* entries minus `stream`.
#include <cstdint>
#include <cstring>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_ragged_math.h"  // bbd_put_rgb
#include "../../baseboostdepth_amd/csrc/bbd_view_math.h"

static inline void offer(uint64_t* cell, uint64_t key) {
  if (*cell > key) *cell = key;
}

extern "C" int hp_view_clear(uint64_t* cells, int64_t* counters, int H, int W) {
  const int rc = bbd_view_canvas_status(cells, H, W);
  if (rc) return rc;
  if (!counters) return BBD_E_BADARG;
  for (long c = 0; c < (long)H * W; ++c) cells[c] = BBD_VIEW_EMPTY;
  memset(counters, 0, BBD_VIEW_COUNTERS * 8);
  return 0;
}

extern "C" int hp_view_points(uint64_t* cells, int64_t* counters, int H, int W, const void* vertices,
                              const int32_t* count, int n_max, const double* view, int size) {
  const int rc = bbd_view_points_status(cells, counters, H, W, vertices, n_max, view, size);
  if (rc) return rc;
  long n = n_max;
  if (count) n = *count < 0 ? 0 : (*count < n ? *count : n);
  const uint32_t* words = static_cast<const uint32_t*>(vertices);
  for (long g = 0; g < n; ++g) {
    float xyz[3];
    memcpy(xyz, words + 4 * g, 12);
    counters[0] += 1;
    BbdViewProj p;
    const int verdict = bbd_view_project(view, (double)xyz[0], (double)xyz[1], (double)xyz[2], &p);
    if (verdict == BBD_VIEW_REJECTED) {
      counters[3] += 1;
      continue;
    }
    BbdViewBox b;
    if (verdict == BBD_VIEW_BEHIND || !bbd_view_footprint(&p, size, H, W, &b)) {
      counters[2] += 1;
      continue;
    }
    counters[1] += 1;
    const uint64_t key = bbd_view_point_key(p.d, words[4 * g + 3]);
    for (int y = b.y0; y <= b.y1; ++y)
      for (int x = b.x0; x <= b.x1; ++x) offer(cells + ((size_t)y * W + x), key);
  }
  return 0;
}

extern "C" int hp_view_lines(uint64_t* cells, int64_t* counters, int H, int W, const double* xyz, int P,
                             const double* view, int rgb, double width, int layer, int closed) {
  const int rc = bbd_view_lines_status(cells, counters, H, W, xyz, P, view, rgb, width, layer, closed);
  if (rc) return rc;
  const uint64_t key = bbd_view_overlay_key(layer, rgb);
  const double r = width / 2.0, r2 = r * r;
  const int segments = bbd_view_segments(P, closed);
  for (long s = 0; s < segments; ++s) {
    const double* pa = xyz + 3 * s;
    const double* pb = xyz + 3 * ((s + 1) % P);
    BbdViewProj qa, qb;
    if (bbd_view_project(view, pa[0], pa[1], pa[2], &qa) != BBD_VIEW_FRONT) continue;
    if (bbd_view_project(view, pb[0], pb[1], pb[2], &qb) != BBD_VIEW_FRONT) continue;
    BbdViewBox b;
    if (!bbd_view_segment_box(&qa, &qb, r, H, W, &b)) continue;
    for (int y = b.y0; y <= b.y1; ++y)
      for (int x = b.x0; x <= b.x1; ++x)
        if (bbd_view_dist2(x, y, qa.u, qa.v, qb.u, qb.v) <= r2) offer(cells + ((size_t)y * W + x), key);
  }
  return 0;
}

extern "C" int hp_view_resolve(const uint64_t* cells, int H, int W, int background_rgb, uint8_t* out) {
  const int rc = bbd_view_canvas_status(cells, H, W);
  if (rc) return rc;
  if (!out || background_rgb < 0 || background_rgb > 0xffffff) return BBD_E_BADARG;
  for (long c = 0; c < (long)H * W; ++c) bbd_put_rgb(out + 3 * c, bbd_view_cell_rgb(cells[c], (uint32_t)background_rgb));
  return 0;
}
