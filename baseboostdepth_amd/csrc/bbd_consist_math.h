/* bbd_consist_math.h - everything of bbd_depth_consistency that is not launch geometry, a wave sum or an atomic, shared
 * by bbd_consist.hip and its host port (tests/host_port/bbd_consist_port.cpp): the argument rules, the transform of a
 * (reference, source) pair and what one reference pixel becomes.  Compiled with -ffp-contract=off: every product, sum
 * and quotient below is one IEEE operation, rounded where it is written; `float` lines are float32, `double` lines
 * float64.  No transcendental function: a correctly rounding host and the device give the same bits.
 *
 *   pair (i, v)  src = sources[i][v], taken as -1 (none) outside [0, n).  M = the first three rows of
 *                inv(P_src) . P_ref, P = poses[.] row-major 4x4 camera to world, the general inverse of the odometry
 *                code (bbd_odom_inv4: Gauss-Jordan, partial pivoting), then bbd_odom_mul4d.  No source: twelve zeros.
 *   pixel k = y * w + x of frame i:
 *   1 depth    d = 1.0f / disp[i][k]               float32 (BBD_CONSIST_INPUT_IS_DEPTH: d = disp[i][k])
 *              VALID when d > 0 and finite - the same rule for a reference pixel and for a tap of a source
 *   2 ray      p = bbd_syns_backproject(inv_K, k, h, w, pixel rays, d)     float32: the point the scene map takes
 *   3 scale    q_j = scale * (double)p_j
 *   per source v with src >= 0:
 *   4 move     X_r = ((M[4r] * q_0 + M[4r+1] * q_1) + M[4r+2] * q_2) + M[4r+3], r = 0, 1, 2;  z = X_2
 *   5 project  c_r = ((K[3r] * X_0 + K[3r+1] * X_1) + K[3r+2] * X_2) with K widened to double;  u = c_0 / c_2,
 *              t = c_1 / c_2
 *   6 visible  z > 0 and finite, 0 <= u <= w - 1, 0 <= t <= h - 1 (a NaN fails), h >= 2 and w >= 2, and the four taps
 *              (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) of frame src VALID, x0 = min((int)floor(u), w - 2),
 *              y0 = min((int)floor(t), h - 2): u = w - 1 is inside, with weight 1 on the last column
 *   7 sample   INVERSE depth, bilinear: a tap's s = (double)disp (depth input: (double)(1.0f / disp));  fx = u - x0,
 *              fy = t - y0;  top = s00 + fx * (s01 - s00), bot = s10 + fx * (s11 - s10), s = top + fy * (bot - top)
 *              - inverse depth is affine in the pixel on a plane, so the sample is exact there up to rounding
 *   8 compare  d_b = scale / s, which must be above 0 and finite for the sample to be visible (a scale that is not
 *              positive and finite fails here or at z);  e = fabs(z - d_b) / (z + d_b) in [0, 1];  err = (float)e,
 *              rounded once
 *              the sample AGREES when (double)err < threshold (strict)
 *   pixel      seen = visible sources, agree = agreeing ones, err = the smallest over the visible ones (none: the quiet
 *              NaN 0x7fc00000), kept = VALID and agree >= min_views, filtered = kept ? disp[i][k] : 0.0f
 *   counters   per frame: VALID pixels, visible samples, agreeing samples, sum over visible samples of
 *              (int64)((double)err * 16777216.0 + 0.5), kept pixels - integers only
 */
#ifndef BBD_CONSIST_MATH_H
#define BBD_CONSIST_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_cloud_math.h" /* bbd_cloud_float_bits; brings bbd_syns_math.h (bbd_syns_backproject) */
#include "bbd_odom_math.h"  /* bbd_odom_inv4, bbd_odom_mul4d */

#define BBD_CONSIST_NAN_BITS 0x7fc00000u
#define BBD_CONSIST_ERR_ONE 16777216.0 /* 2^24: the fixed point of the err sums */

/* What the per-pixel function reads of a call. */
struct BbdConsistParams {
  const float* disp;   /* [n,h,w] */
  const float* K;      /* [3,3] */
  const float* inv_K;  /* [3,3] */
  int n, h, w, V, flags, min_views;
  double threshold;
};

/* What a reference pixel becomes. */
struct BbdConsistPixel {
  int valid, seen, agree, kept;
  int64_t err_sum;
  uint32_t err_bits;  /* bits of the smallest err, or BBD_CONSIST_NAN_BITS */
  float filtered;
};

/* Status of bbd_depth_consistency's arguments: 0, BBD_E_BADARG or BBD_E_TOOMANY. */
BBD_HD int bbd_consist_status(const void* disp, const void* poses, const void* K, const void* inv_K, const void* sources,
                              const void* transforms, const void* seen, const void* agree, const void* counters, int n,
                              int h, int w, int V, double threshold, int min_views, int flags) {
  if (!disp || !poses || !K || !inv_K || !sources || !transforms || !seen || !agree || !counters) return BBD_E_BADARG;
  if (n < 1 || h < 1 || w < 1 || V < 1 || V > BBD_CONSIST_MAX_VIEWS || min_views < 0) return BBD_E_BADARG;
  if (!(threshold >= 0.0)) return BBD_E_BADARG; /* a NaN threshold lands here */
  if (flags & ~BBD_CONSIST_INPUT_IS_DEPTH) return BBD_E_BADARG;
  if ((long)n * (long)h * (long)w > 0x7fffffffL) return BBD_E_TOOMANY;
  return 0;
}

/* Source v of frame i, or -1: an entry outside [0, n) means none. */
BBD_HD int bbd_consist_source(const int32_t* sources, int n, int V, int i, int v) {
  const int32_t s = sources[(size_t)i * V + v];
  return (s >= 0 && s < n) ? (int)s : -1;
}

/* out[12] = rows 0..2 of inv(poses[src]) . poses[ref]; twelve zeros where src < 0. */
BBD_HD void bbd_consist_transform(const double* poses, int ref, int src, double* out) {
  if (src < 0) {
    for (int e = 0; e < 12; ++e) out[e] = 0.0;
    return;
  }
  double inv[16], prod[16];
  bbd_odom_inv4(poses + (size_t)src * 16, inv);
  bbd_odom_mul4d(inv, poses + (size_t)ref * 16, prod);
  for (int e = 0; e < 12; ++e) out[e] = prod[e];
}

/* Step 1: the depth of a stored value; *valid = it is above 0 and finite. */
BBD_HD float bbd_consist_depth(float raw, int flags, int* valid) {
  const float d = (flags & BBD_CONSIST_INPUT_IS_DEPTH) ? raw : 1.0f / raw;
  *valid = (d > 0.0f) && (d - d == 0.0f);
  return d;
}

/* The inverse depth of a VALID tap, widened. */
BBD_HD double bbd_consist_inverse(float raw, int flags) {
  return (double)((flags & BBD_CONSIST_INPUT_IS_DEPTH) ? 1.0f / raw : raw);
}

/* Steps 4 to 8 for one source: 1 and *err where the sample is visible, else 0.  q = the scaled point of the reference
 * pixel, M = the pair's transform (any 12 doubles), K9 = K widened, plane = the source frame's h x w values. */
BBD_HD int bbd_consist_sample(const BbdConsistParams* a, double scale, const double* q, const double* M, const double* K9,
                              const float* plane, float* err) {
  double X[3], c[3];
  for (int r = 0; r < 3; ++r) X[r] = ((M[4 * r] * q[0] + M[4 * r + 1] * q[1]) + M[4 * r + 2] * q[2]) + M[4 * r + 3];
  const double z = X[2];
  if (!(z > 0.0 && z - z == 0.0)) return 0;
  for (int r = 0; r < 3; ++r) c[r] = ((K9[3 * r] * X[0] + K9[3 * r + 1] * X[1]) + K9[3 * r + 2] * X[2]);
  const double u = c[0] / c[2], t = c[1] / c[2];
  const int h = a->h, w = a->w;
  if (h < 2 || w < 2) return 0;
  if (!(u >= 0.0 && u <= (double)(w - 1) && t >= 0.0 && t <= (double)(h - 1))) return 0;
  int x0 = (int)floor(u), y0 = (int)floor(t);
  x0 = x0 < w - 2 ? x0 : w - 2;
  y0 = y0 < h - 2 ? y0 : h - 2;
  const float* r0 = plane + (size_t)y0 * w + x0;
  const float t00 = r0[0], t01 = r0[1], t10 = r0[w], t11 = r0[w + 1];
  int v00, v01, v10, v11;
  bbd_consist_depth(t00, a->flags, &v00);
  bbd_consist_depth(t01, a->flags, &v01);
  bbd_consist_depth(t10, a->flags, &v10);
  bbd_consist_depth(t11, a->flags, &v11);
  if (!(v00 && v01 && v10 && v11)) return 0;
  const double s00 = bbd_consist_inverse(t00, a->flags), s01 = bbd_consist_inverse(t01, a->flags);
  const double s10 = bbd_consist_inverse(t10, a->flags), s11 = bbd_consist_inverse(t11, a->flags);
  const double fx = u - (double)x0, fy = t - (double)y0;
  const double top = s00 + fx * (s01 - s00), bot = s10 + fx * (s11 - s10);
  const double s = top + fy * (bot - top);
  const double d_b = scale / s;
  if (!(d_b > 0.0 && d_b - d_b == 0.0)) return 0; /* a scale that is not positive and finite: no comparison */
  const double e = fabs(z - d_b) / (z + d_b);
  *err = (float)e;
  return 1;
}

/* Pixel k of frame i: steps 1 to 8 over its V sources.  `scale` is the value the call read once; src[v] and M[v] are
 * the sources and transforms of frame i (src[v] < 0: none). */
BBD_HD void bbd_consist_pixel(const BbdConsistParams* a, double scale, const double* K9, const int* src, const double* M,
                              int i, int k, BbdConsistPixel* o) {
  const size_t plane = (size_t)a->h * (size_t)a->w;
  const float raw = a->disp[(size_t)i * plane + (size_t)k];
  int valid;
  const float d = bbd_consist_depth(raw, a->flags, &valid);
  o->valid = valid;
  o->seen = 0;
  o->agree = 0;
  o->err_sum = 0;
  o->err_bits = BBD_CONSIST_NAN_BITS;
  float best = 2.0f; /* every err is at most 1 */
  if (valid) {
    float p[3];
    bbd_syns_backproject(a->inv_K, k, a->h, a->w, 1, d, p);
    const double q[3] = {scale * (double)p[0], scale * (double)p[1], scale * (double)p[2]};
    for (int v = 0; v < a->V; ++v) {
      if (src[v] < 0) continue;
      float err;
      if (!bbd_consist_sample(a, scale, q, M + 12 * v, K9, a->disp + (size_t)src[v] * plane, &err)) continue;
      o->seen += 1;
      o->agree += ((double)err < a->threshold) ? 1 : 0;
      o->err_sum += (int64_t)((double)err * BBD_CONSIST_ERR_ONE + 0.5);
      best = err < best ? err : best;
    }
    if (o->seen) o->err_bits = bbd_cloud_float_bits(best);
  }
  o->kept = valid && o->agree >= a->min_views;
  o->filtered = o->kept ? raw : 0.0f;
}

#endif /* BBD_CONSIST_MATH_H */
