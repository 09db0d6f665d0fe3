/* bbd_viz_math.h - per-pixel arithmetic of the colour-mapped disparity (bbd_viz.hip), shared with the
 * host port of the test tier (tests/host_port/bbd_viz_port.cpp).  Restates test_simple.py:135-148:
 *
 *   s    = min_disp + (max_disp - min_disp) * d             layers.disp_to_depth: one multiply, one add
 *   vmax = np.percentile(s, p)                               numpy "linear" method on a float32 array
 *   x    = (s - vmin) / (vmax - vmin)                        matplotlib Normalize, float32, IEEE division
 *   rgb  = trunc(magma[trunc(x * 256)] * 255)                ScalarMappable.to_rgba()[..., :3] * 255 -> uint8
 *
 * Compile with -ffp-contract=off: every rounding below is one the reference performs. */
#ifndef BBD_VIZ_MATH_H
#define BBD_VIZ_MATH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "bbd_math.h"

BBD_HD uint32_t bbd_viz_float_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(v);
#else
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
#endif
}
BBD_HD float bbd_viz_bits_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float v;
  memcpy(&v, &b, 4);
  return v;
#endif
}

/* upsample_bilinear2d, align_corners=False: source index and lambda for output index o at ANY size ratio.  Same as
 * bbd_up_src (bbd_math.h) except that the source coordinate scale * (o + 0.5) - 0.5 is rounded once: ATen's CPU
 * kernels are built with contraction on, so area_pixel_compute_source_index is a single FMA.  At the ratios the
 * training path uses (powers of two) the product is exact and both forms agree; at the ragged ratios of prediction
 * (192x640 -> 375x1242) the twice-rounded form moves lambda by an ulp on about 1 % of the pixels. */
BBD_HD void bbd_viz_up_src(int o, int in_size, int out_size, int* i0, int* i1, float* l0, float* l1) {
  const float scale = (float)in_size / (float)out_size;
  float src = fmaf(scale, (float)o + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  int i = (int)src;
  i = i < in_size - 1 ? i : in_size - 1;
  *i0 = i;
  *i1 = i + (i < in_size - 1 ? 1 : 0);
  *l1 = src - (float)i;
  *l0 = 1.0f - *l1;
}

/* layers.disp_to_depth: the two Python doubles meet the fp32 tensor as fp32 scalars (lo, span). */
BBD_HD float bbd_viz_scaled(float d, float lo, float span) {
  const float m = span * d;
  return lo + m;
}

/* Monotone map float -> uint32 (the order bbd_eval.hip selects in) and back. */
BBD_HD uint32_t bbd_viz_order_key(float v) {
  const uint32_t b = bbd_viz_float_bits(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
BBD_HD float bbd_viz_key_value(uint32_t k) {
  return bbd_viz_bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

/* np.percentile(a, p) on a float32 array of n values, numpy 2.x: the quantile q = float32(p) / float32(100) and the
 * virtual index (n - 1) * q are float32 (q takes the array's dtype, the Python int n - 1 is a weak scalar), the two
 * bracketing order statistics are taken at floor(index) and floor(index) + 1, both the maximum once index >= n - 1.
 * `q` is computed once on the host by bbd_viz_quantile. */
BBD_HD float bbd_viz_quantile(double percentile) { return (float)percentile / 100.0f; }
BBD_HD void bbd_viz_ranks(uint32_t n, float q, uint32_t* lower, uint32_t* upper, float* gamma) {
  const float last = (float)(n - 1u);
  const float vi = last * q;
  if (!(vi < last)) {          /* numpy: indexes_above_bounds -> arr[-1] twice */
    *lower = n - 1u;
    *upper = n - 1u;
    *gamma = 0.0f;             /* both values equal: any weight gives the maximum */
    return;
  }
  const float fl = (float)(uint32_t)vi;      /* vi >= 0: truncation is floor */
  uint32_t lo = (uint32_t)vi;
  lo = lo < n - 1u ? lo : n - 1u;
  *lower = lo;
  *upper = lo + 1u < n ? lo + 1u : n - 1u;
  *gamma = vi - fl;
}
/* numpy _lerp with every operand float32: a + (b-a)*t, replaced by b - (b-a)*(1-t) where t >= 0.5. */
BBD_HD float bbd_viz_lerp(float a, float b, float t) {
  const float diff = b - a;
  if (t >= 0.5f) {
    const float m = diff * (1.0f - t);
    return b - m;
  }
  const float m = diff * t;
  return a + m;
}

/* matplotlib Normalize + Colormap.__call__ index (N = 256) for one value.  vmax == vmin: Normalize returns zeros.
 * x * 256 == 256 is the last entry; above it the colour map's "over" colour, which for magma is its last entry;
 * x < 0 cannot occur (vmin is the minimum).  A NaN takes entry 0 (matplotlib would draw its "bad" colour; a sigmoid
 * output holds no NaN). */
BBD_HD int bbd_viz_lut_index(float s, float vmin, float vmax) {
  if (vmax == vmin) return 0;
  const float x = (s - vmin) / (vmax - vmin);
  const float xi = x * 256.0f;
  if (!(xi < 256.0f)) return xi != xi ? 0 : 255;
  const int i = (int)xi;
  return i < 0 ? 0 : i;
}

#endif /* BBD_VIZ_MATH_H */
