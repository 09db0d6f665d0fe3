/* bbd_compare_math.h - per-pixel arithmetic of the checkpoint comparison sheets (bbd_compare.hip), shared with the host
 * port of the test tier (tests/host_port/bbd_compare_port.cpp).
 *
 *   GT picture   v = 1.0f / g, v > max_inv -> 0; lut[bbd_viz_lut_index(v, min, max)], min / max of v without its NaNs
 *                (validation.py:250-254: 1 / gt_depth, values above 80 zeroed, Normalize(min, max), magma)
 *   error map    at a valid ground-truth pixel (bbd_eval.hip's predicate, inside the crop window) the abs_rel summand of
 *                bbd_depth_metrics: p = bbd_eval_resample(disparity), p *= ratio, clamp, e = |g - p| / g; every output
 *                pixel shows the maximum e within Chebyshev distance `radius`, or the darkened grey of the input picture
 *
 * Colours travel as r | g << 8 | b << 16.  Compile with -ffp-contract=off. */
#ifndef BBD_COMPARE_MATH_H
#define BBD_COMPARE_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_eval_math.h"
#include "bbd_viz_math.h"

#define BBD_COMPARE_NAN_BITS 0x7fc00000u      /* the quiet NaN bbd_eval.hip writes */

/* One ground-truth map and the prediction it is compared with. */
struct BbdCompareMap {
  const float* gt;        /* [GH, GW] */
  const float* pred;      /* [h, w] scaled disparity */
  int GH, GW, r0, r1, c0, c1, h, w;
  float min_depth, max_depth, scale_factor, ratio;
  int flags;              /* BBD_EVAL_NO_MEDIAN_SCALING or 0 */
  int radius;
};

/* validation.py:250-251 for one pixel: IEEE division (a zero gives +inf), then the cut. */
BBD_HD float bbd_compare_gt_inverse(float g, float max_inv) {
  const float v = 1.0f / g;
  return v > max_inv ? 0.0f : v;
}

/* Is (y, x) a pixel bbd_depth_metrics scores?  Then *e is its abs_rel summand (bbd_eval.hip:146-160). */
BBD_HD bool bbd_compare_error_at(const BbdCompareMap& m, int y, int x, float* e) {
  if (y < m.r0 || y >= m.r1 || x < m.c0 || x >= m.c1 || y < 0 || y >= m.GH || x < 0 || x >= m.GW) return false;
  const float g = m.gt[(size_t)y * m.GW + x];
  if (!(g > m.min_depth && g < m.max_depth)) return false;
  float p = bbd_eval_resample(m.pred, m.h, m.w, m.scale_factor, 0.0f, 0.0f, BBD_EVAL_PRED_IS_DISP, y, x, m.GH, m.GW);
  if (!(m.flags & BBD_EVAL_NO_MEDIAN_SCALING)) p *= m.ratio;
  p = p < m.min_depth ? m.min_depth : p;
  p = p > m.max_depth ? m.max_depth : p;
  const float df = g - p;
  *e = fabsf(df) / g;
  return true;
}

/* Maximum error over the valid pixels within Chebyshev distance `radius` of (y, x); false when there is none.  A NaN
 * error (a NaN prediction) wins and stays, so the result does not depend on the order of the visit. */
BBD_HD bool bbd_compare_error_max(const BbdCompareMap& m, int y, int x, float* e_max) {
  bool any = false;
  float best = 0.0f;
  for (int dy = -m.radius; dy <= m.radius; ++dy)
    for (int dx = -m.radius; dx <= m.radius; ++dx) {
      float e;
      if (!bbd_compare_error_at(m, y + dy, x + dx, &e)) continue;
      if (!any) best = e;
      else if (best == best && (e > best || e != e)) best = e;
      any = true;
    }
  *e_max = best;
  return any;
}

/* Background of the error map: the input picture's grey, darkened by half ((r + g + b) / 6), in all three channels. */
BBD_HD uint32_t bbd_compare_grey(const uint8_t* rgb) {
  const uint32_t v = ((uint32_t)rgb[0] + (uint32_t)rgb[1] + (uint32_t)rgb[2]) / 6u;
  return v | (v << 8) | (v << 16);
}

#endif /* BBD_COMPARE_MATH_H */
