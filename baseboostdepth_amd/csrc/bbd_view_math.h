/* bbd_view_math.h - everything of the bbd_view_* entries that is not launch geometry or an atomic, shared by
 * bbd_view.hip and its host port (tests/host_port/bbd_view_port.cpp): the argument rules, the projection of a point, the
 * key of a cell, a point's footprint, a segment's box and the distance of a pixel centre from a segment.  Compiled with
 * -ffp-contract=off: every product, sum and quotient below is one IEEE operation, rounded where it is written.  All
 * arithmetic on coordinates is float64.
 *
 *   project   p_r = ((V[4r] * x + V[4r+1] * y) + V[4r+2] * z) + V[4r+3], r = 0 .. 3, V the row-major 4x4 view
 *             u = p_0 / p_3, v = p_1 / p_3, d = p_2
 *             REJECTED when any of u, v, d, p_3 is not finite - p_3 = 0 makes u and v infinite or NaN, so it lands here;
 *             else BEHIND when p_3 <= 0 or d <= 0; else IN FRONT
 *   key       rank << 32 | colour;  colour = r << 24 | g << 16 | b << 8 | 0xff;  the empty key is all ones
 *             point rank   = 0x80000000 | (bits((float)d) >> 1): positive floats order like their bits, nearer = smaller
 *             overlay rank = 0x7fffffff - layer, 0 <= layer < 2^16: below every point rank, a higher layer is smaller
 *             no key is the empty one: the largest rank is 0x80000000 | (0x7f800000 >> 1)
 *   point     pixel (floor(u), floor(v)); footprint = the size x size square centred on it, size in {1, 3, 5, 7}; CLIPPED
 *             when the square misses the canvas (decided in float64, before any conversion to int), else cut to it
 *   segment   r = width / 2; columns floor(min(a_x, b_x) - r - 0.5) .. ceil(max(a_x, b_x) + r - 0.5) cut to [0, W - 1],
 *             rows likewise: a superset of the pixels whose centre can lie within r; the distance decides
 *   distance  of c = (i + 0.5, j + 0.5) from segment a b, squared: e = b - a, w = c - a, l = e_x e_x + e_y e_y,
 *             t = l > 0 ? (w_x e_x + w_y e_y) / l : 0, cut to [0, 1]; q = a + t e; (c_x - q_x)^2 + (c_y - q_y)^2.
 *             Painted when that is <= r * r.  No square root.
 */
#ifndef BBD_VIEW_MATH_H
#define BBD_VIEW_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h" /* BBD_HD */

#define BBD_VIEW_EMPTY 0xffffffffffffffffull

/* bbd_view_project's verdicts */
#define BBD_VIEW_REJECTED 0
#define BBD_VIEW_FRONT 1
#define BBD_VIEW_BEHIND 2

struct BbdViewProj {
  double u, v, d;
};

struct BbdViewBox {
  int x0, x1, y0, y1; /* inclusive */
};

BBD_HD int bbd_view_finite(double v) { return v - v == 0.0; }

/* Status of the canvas arguments: 0, BBD_E_BADARG or BBD_E_TOOMANY. */
BBD_HD int bbd_view_canvas_status(const void* cells, int H, int W) {
  if (!cells || H < 1 || W < 1) return BBD_E_BADARG;
  if ((long)H * (long)W > BBD_VIEW_MAX_CELLS) return BBD_E_TOOMANY;
  return 0;
}

BBD_HD int bbd_view_points_status(const void* cells, const void* counters, int H, int W, const void* vertices, int n_max,
                                  const void* view, int size) {
  const int rc = bbd_view_canvas_status(cells, H, W);
  if (rc) return rc;
  if (!counters || !vertices || !view || n_max < 0) return BBD_E_BADARG;
  if (((uintptr_t)vertices & (BBD_CLOUD_VERTEX - 1)) != 0) return BBD_E_BADARG;
  return (size == 1 || size == 3 || size == 5 || size == 7) ? 0 : BBD_E_BADARG;
}

BBD_HD int bbd_view_lines_status(const void* cells, const void* counters, int H, int W, const void* xyz, int P,
                                 const void* view, int rgb, double width, int layer, int closed) {
  const int rc = bbd_view_canvas_status(cells, H, W);
  if (rc) return rc;
  if (!counters || !xyz || !view || P < 1) return BBD_E_BADARG;
  if (rgb < 0 || rgb > 0xffffff || layer < 0 || layer > BBD_VIEW_MAX_LAYER || (closed != 0 && closed != 1))
    return BBD_E_BADARG;
  return (width > 0.0 && bbd_view_finite(width)) ? 0 : BBD_E_BADARG; /* a NaN width lands here */
}

/* The segments of a polyline of P vertices: one disc for a single vertex. */
BBD_HD int bbd_view_segments(int P, int closed) { return P == 1 ? 1 : (closed && P > 2 ? P : P - 1); }

BBD_HD int bbd_view_project(const double* V, double x, double y, double z, BbdViewProj* o) {
  double p[4];
  for (int r = 0; r < 4; ++r) p[r] = ((V[4 * r] * x + V[4 * r + 1] * y) + V[4 * r + 2] * z) + V[4 * r + 3];
  o->u = p[0] / p[3];
  o->v = p[1] / p[3];
  o->d = p[2];
  if (!(bbd_view_finite(o->u) && bbd_view_finite(o->v) && bbd_view_finite(o->d) && bbd_view_finite(p[3])))
    return BBD_VIEW_REJECTED;
  return (p[3] <= 0.0 || o->d <= 0.0) ? BBD_VIEW_BEHIND : BBD_VIEW_FRONT;
}

BBD_HD uint32_t bbd_view_float_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, sizeof b);
  return b;
}

/* `word` is a vertex record's fourth word, r | g << 8 | b << 16 | a << 24. */
BBD_HD uint64_t bbd_view_point_key(double d, uint32_t word) {
  const uint32_t rank = 0x80000000u | (bbd_view_float_bits((float)d) >> 1);
  const uint32_t colour = ((word & 0xffu) << 24) | ((word & 0xff00u) << 8) | ((word >> 8) & 0xff00u) | 0xffu;
  return ((uint64_t)rank << 32) | colour;
}

/* `rgb` is r | g << 8 | b << 16. */
BBD_HD uint64_t bbd_view_overlay_key(int layer, int rgb) {
  const uint32_t rank = 0x7fffffffu - (uint32_t)layer, c = (uint32_t)rgb;
  const uint32_t colour = ((c & 0xffu) << 24) | ((c & 0xff00u) << 8) | ((c >> 8) & 0xff00u) | 0xffu;
  return ((uint64_t)rank << 32) | colour;
}

/* The packed colour (r | g << 8 | b << 16) of a cell, `background` where it is empty. */
BBD_HD uint32_t bbd_view_cell_rgb(uint64_t key, uint32_t background) {
  if (key == BBD_VIEW_EMPTY) return background;
  const uint32_t c = (uint32_t)key;
  return (c >> 24) | ((c >> 8) & 0xff00u) | ((c << 8) & 0xff0000u);
}

/* [lo, hi] in float64 cut to [0, n - 1]; 0 when nothing is left. */
BBD_HD int bbd_view_cut(double lo, double hi, int n, int* i0, int* i1) {
  if (lo < 0.0) lo = 0.0;
  if (hi > (double)(n - 1)) hi = (double)(n - 1);
  if (!(lo <= hi)) return 0;
  *i0 = (int)lo;
  *i1 = (int)hi;
  return 1;
}

/* The footprint of a point in front; 0 when it misses the canvas. */
BBD_HD int bbd_view_footprint(const BbdViewProj* p, int size, int H, int W, BbdViewBox* b) {
  const double half = (double)(size / 2), fu = floor(p->u), fv = floor(p->v);
  return bbd_view_cut(fu - half, fu + half, W, &b->x0, &b->x1) && bbd_view_cut(fv - half, fv + half, H, &b->y0, &b->y1);
}

/* The pixels a segment of half-width r can paint; 0 when none is on the canvas. */
BBD_HD int bbd_view_segment_box(const BbdViewProj* a, const BbdViewProj* b, double r, int H, int W, BbdViewBox* o) {
  const double xlo = a->u < b->u ? a->u : b->u, xhi = a->u < b->u ? b->u : a->u;
  const double ylo = a->v < b->v ? a->v : b->v, yhi = a->v < b->v ? b->v : a->v;
  return bbd_view_cut(floor(xlo - r - 0.5), ceil(xhi + r - 0.5), W, &o->x0, &o->x1) &&
         bbd_view_cut(floor(ylo - r - 0.5), ceil(yhi + r - 0.5), H, &o->y0, &o->y1);
}

/* Squared distance of the centre of pixel (i, j) from the segment a b. */
BBD_HD double bbd_view_dist2(int i, int j, double ax, double ay, double bx, double by) {
  const double cx = (double)i + 0.5, cy = (double)j + 0.5;
  const double ex = bx - ax, ey = by - ay, wx = cx - ax, wy = cy - ay;
  const double l = ex * ex + ey * ey;
  double t = l > 0.0 ? (wx * ex + wy * ey) / l : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double gx = cx - (ax + t * ex), gy = cy - (ay + t * ey);
  return gx * gx + gy * gy;
}

#endif /* BBD_VIEW_MATH_H */
