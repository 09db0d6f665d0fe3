/* bbd_geo_math.h - everything of the geometry-consistency loss (bbd_geo_fwd / bbd_geo_bwd) that is not
 * launch geometry, a wave sum or an atomic, shared by bbd_geo.hip and its host port (tests/host_port/geo.cpp): the
 * argument rules, what one (target pixel, source) sample is, its derivatives, the fixed point of the scattered sums and
 * the order of every floating-point addition.  Compiled with -ffp-contract=off: every product, sum and quotient below is
 * one IEEE operation, rounded where it is written; `float` lines are float32, `double` lines float64.  Divisions go
 * through bbd_div (bbd_math.h: correctly rounded on the device, `/` on the host).  No transcendental function.
 *
 *   q_tgt [B,H,W], q_src [V,B,H,W] inverse depths, T [V,B,12] rows 0..2 of target-to-source, K / inv_K [B,16] (4x4
 *   row-major, the 3x3 part is read).  Pixel k = y * W + x of sample b, source v:
 *   1 ray      r_j = (iK[4j] * x + iK[4j+1] * y) + iK[4j+2];  p_j = r_j / q_tgt                                  j = 0..2
 *              the target pixel is VALID when q_tgt > 0 and finite
 *   2 move     X_r = ((T[4r] * p_0 + T[4r+1] * p_1) + T[4r+2] * p_2) + T[4r+3];  z = X_2
 *   3 project  c_r = (K[4r] * X_0 + K[4r+1] * X_1) + K[4r+2] * X_2;  u = c_0 / c_2, t = c_1 / c_2
 *   4 visible  VALID, z finite and z > BBD_GEO_MIN_Z, 0 <= u <= W - 1, 0 <= t <= H - 1 (a NaN fails), H >= 2 and W >= 2,
 *              the four taps at x0 = min((int)floor(u), W - 2), y0 = min((int)floor(t), H - 2) above 0 and finite - the
 *              cell and edge rules of bbd_consist_math.h: u = W - 1 is inside, with weight 1 on the last column -
 *              and the two range rules below
 *   5 sample   fx = u - x0, fy = t - y0;  top = s00 + fx * (s01 - s00), bot = s10 + fx * (s11 - s10),
 *              s = top + fy * (bot - top): the source's INVERSE depth (affine in the pixel on a plane)
 *   6 compare  a = z * s;  e = fabs(a - 1) / (a + 1) in [0, 1): algebraically |z - d| / (z + d) with d = 1 / s, the err
 *              of bbd_consist_math.h
 *   range      s >= BBD_GEO_MIN_S and a finite, else the sample is NOT visible.  The first rule is what bounds the
 *              scattered gradient: |de/ds| = 2 z / (z s + 1)^2 <= 1 / (2 s) <= 2^9 (the maximum over z is at z = 1 / s)
 *   code       bit 0 = visible, bit 1 = a > 1 (set only where visible)
 *
 *   sums       pair_sum: the integer sum over visible samples of (int64)floor((double)e * 2^36 + 0.5), times 2^-36 at
 *              the end: e < 1 and a pair has at most 2^23 samples, so the sum stays below 2^59.  Integers: order-free.
 *
 *   backward   per visible sample, WITHOUT the upstream factor g[v,b]:
 *              D = sign(a - 1) * (2 / ((a + 1) * (a + 1)))   (0 at a == 1)
 *              ds = D * z  -> the taps: ds * ((1 - fx) * (1 - fy)), ds * (fx * (1 - fy)), ds * ((1 - fx) * fy),
 *                             ds * (fx * fy), each (int64)floor((double)value * 2^30 + 0.5), added to the pair's plane
 *                             with integer atomics.  |value| <= 2^9 (1 + 2^-20), at most one value per sample and tap,
 *                             H * W <= 2^23 samples (BBD_E_TOOMANY otherwise): |sum| < 2^63.  Nothing can wrap.
 *              gu = ds * ((s01 - s00) + fy * ((s11 - s10) - (s01 - s00))),  gt = ds * (bot - top)
 *              gc_0 = gu / c_2, gc_1 = gt / c_2, gc_2 = -((gu * u + gt * t) / c_2)
 *              gX_j = (K[j] * gc_0 + K[4+j] * gc_1) + K[8+j] * gc_2, and gX_2 += D * s
 *              grad_T[4r+j] takes (double)gX_r * (double)p_j (exact), grad_T[4r+3] takes (double)gX_r
 *              gp_j = (T[j] * gX_0 + T[4+j] * gX_1) + T[8+j] * gX_2
 *              gq = -(((gp_0 * p_0 + gp_1 * p_1) + gp_2 * p_2) / q_tgt)
 *   grad_q_tgt the pixel's lane adds g[v,b] * (double)gq over v = 0 .. V-1 in that order, rounds to float once
 *   grad_q_src (float)(g[v,b] * ((double)sum * 2^-30))
 *   grad_T     a WORK ITEM is BBD_GEO_RUN = 2048 neighbouring pixels of one sample, taken by 256 lanes: lane l adds its
 *              pixels l, l + 256, ... in that order (float64), the 64 lanes of a wave are added as a tree
 *              (bbd_geo_tree64: strides 32, 16, ... 1), the 4 waves in index order, and the items of a pair in index
 *              order; then (float)(g[v,b] * total).  Every output is written by one lane.
 */
#ifndef BBD_GEO_MATH_H
#define BBD_GEO_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"

#define BBD_GEO_MIN_Z 0.001f          /* metres in the network's units: a point this close to the image plane is no sample */
#define BBD_GEO_MIN_S 0.0009765625f   /* 2^-10: inverse depths below it (depths above 1024) are no sample */
#define BBD_GEO_SUM_ONE 68719476736.0 /* 2^36: the fixed point of pair_sum */
#define BBD_GEO_TAP_ONE 1073741824.0  /* 2^30: the fixed point of the grad_q_src sums */
#define BBD_GEO_MAX_PLANE 8388608L    /* 2^23 pixels per map */
#define BBD_GEO_LANES 256
#define BBD_GEO_PASSES (BBD_GEO_RUN / BBD_GEO_LANES)

BBD_HD long bbd_geo_items(int H, int W) { return ((long)H * W + BBD_GEO_RUN - 1) / BBD_GEO_RUN; }
/* 8-byte words of scratch: forward B * items * V * 2, backward V * B * H * W + B * items * V * 12. */
BBD_HD long bbd_geo_fwd_words(int B, int H, int W, int V) { return (long)B * bbd_geo_items(H, W) * V * 2; }
BBD_HD long bbd_geo_bwd_words(int B, int H, int W, int V) {
  return (long)V * B * H * W + (long)B * bbd_geo_items(H, W) * V * 12;
}

BBD_HD int bbd_geo_shape_status(int B, int H, int W, int V) {
  if (B < 1 || H < 1 || W < 1 || V < 1 || V > BBD_GEO_MAX_VIEWS) return BBD_E_BADARG;
  if ((long)H * (long)W > BBD_GEO_MAX_PLANE) return BBD_E_TOOMANY;
  if ((long)V * (long)B * (long)H * (long)W > 0x7fffffffL) return BBD_E_TOOMANY;
  return 0;
}
BBD_HD int bbd_geo_fwd_status(const void* q_tgt, const void* q_src, const void* T, const void* K, const void* inv_K,
                              const void* pair_sum, const void* pair_count, const void* scratch, long scratch_words,
                              int B, int H, int W, int V) {
  if (!q_tgt || !q_src || !T || !K || !inv_K || !pair_sum || !pair_count || !scratch) return BBD_E_BADARG;
  const int rc = bbd_geo_shape_status(B, H, W, V);
  if (rc) return rc;
  return scratch_words < bbd_geo_fwd_words(B, H, W, V) ? BBD_E_BADARG : 0;
}
BBD_HD int bbd_geo_bwd_status(const void* q_tgt, const void* q_src, const void* T, const void* K, const void* inv_K,
                              const void* g, const void* grad_q_tgt, const void* grad_q_src, const void* grad_T,
                              const void* scratch, long scratch_words, int B, int H, int W, int V) {
  if (!q_tgt || !q_src || !T || !K || !inv_K || !g || !grad_q_tgt || !grad_q_src || !grad_T || !scratch)
    return BBD_E_BADARG;
  const int rc = bbd_geo_shape_status(B, H, W, V);
  if (rc) return rc;
  return scratch_words < bbd_geo_bwd_words(B, H, W, V) ? BBD_E_BADARG : 0;
}

/* Above 0 and finite: the rule for a target pixel and for a tap. */
BBD_HD int bbd_geo_positive(float q) { return (q > 0.0f) && (q - q == 0.0f); }

/* Round to the nearest integer of the fixed point `one` (halves towards +inf). */
BBD_HD int64_t bbd_geo_fixed(float value, double one) { return (int64_t)floor((double)value * one + 0.5); }

/* What the samples of one sample b share: the 3x3 parts of K and inv_K. */
struct BbdGeoCamera {
  float K[9], iK[9];
};
BBD_HD void bbd_geo_camera(const float* K, const float* inv_K, int b, BbdGeoCamera* cam) {
  for (int r = 0; r < 3; ++r)
    for (int j = 0; j < 3; ++j) {
      cam->K[3 * r + j] = K[(size_t)b * 16 + 4 * r + j];
      cam->iK[3 * r + j] = inv_K[(size_t)b * 16 + 4 * r + j];
    }
}

/* Step 1.  Returns VALID; p is written only then. */
BBD_HD int bbd_geo_point(const BbdGeoCamera* cam, float q, int x, int y, float p[3]) {
  if (!bbd_geo_positive(q)) return 0;
  const float fx = (float)x, fy = (float)y;
  for (int j = 0; j < 3; ++j) p[j] = bbd_div((cam->iK[3 * j] * fx + cam->iK[3 * j + 1] * fy) + cam->iK[3 * j + 2], q);
  return 1;
}

/* One visible sample, as far as the backward needs it. */
struct BbdGeoSample {
  float X[3], c2, u, t, fx, fy, s00, s01, s10, s11, top, bot, s, a, e;
  int x0, y0;
};

/* Steps 2 to 6 for one source: 1 where the sample is visible.  p = the target pixel's point, T = the pair's 12 floats,
 * plane = the source's H x W inverse depths. */
BBD_HD int bbd_geo_sample(const BbdGeoCamera* cam, const float* p, const float* T, const float* plane, int H, int W,
                          BbdGeoSample* o) {
  for (int r = 0; r < 3; ++r) o->X[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
  const float z = o->X[2];
  if (!(z > BBD_GEO_MIN_Z && z - z == 0.0f)) return 0;
  float c[3];
  for (int r = 0; r < 3; ++r) c[r] = (cam->K[3 * r] * o->X[0] + cam->K[3 * r + 1] * o->X[1]) + cam->K[3 * r + 2] * o->X[2];
  o->c2 = c[2];
  o->u = bbd_div(c[0], c[2]);
  o->t = bbd_div(c[1], c[2]);
  if (H < 2 || W < 2) return 0;
  if (!(o->u >= 0.0f && o->u <= (float)(W - 1) && o->t >= 0.0f && o->t <= (float)(H - 1))) return 0;
  int x0 = (int)floorf(o->u), y0 = (int)floorf(o->t);
  x0 = x0 < W - 2 ? x0 : W - 2;
  y0 = y0 < H - 2 ? y0 : H - 2;
  o->x0 = x0;
  o->y0 = y0;
  const float* r0 = plane + (size_t)y0 * W + x0;
  o->s00 = r0[0]; o->s01 = r0[1]; o->s10 = r0[W]; o->s11 = r0[W + 1];
  if (!(bbd_geo_positive(o->s00) && bbd_geo_positive(o->s01) && bbd_geo_positive(o->s10) && bbd_geo_positive(o->s11)))
    return 0;
  o->fx = o->u - (float)x0;
  o->fy = o->t - (float)y0;
  o->top = o->s00 + o->fx * (o->s01 - o->s00);
  o->bot = o->s10 + o->fx * (o->s11 - o->s10);
  o->s = o->top + o->fy * (o->bot - o->top);
  if (!(o->s >= BBD_GEO_MIN_S)) return 0;
  o->a = z * o->s;
  if (!(o->a - o->a == 0.0f)) return 0;
  o->e = bbd_div(fabsf(o->a - 1.0f), o->a + 1.0f);
  return 1;
}

BBD_HD int bbd_geo_code(const BbdGeoSample* o) { return 1 | (o->a > 1.0f ? 2 : 0); }

/* The derivatives of one visible sample's e, without the upstream factor. */
struct BbdGeoGrad {
  float tap[4];   /* to s00, s01, s10, s11 */
  float gX[3];
  float gq;       /* to the target pixel's inverse depth */
};
BBD_HD void bbd_geo_sample_grad(const BbdGeoCamera* cam, const float* p, float q, const float* T, const BbdGeoSample* o,
                                BbdGeoGrad* g) {
  const float a1 = o->a + 1.0f;
  const float mag = bbd_div(2.0f, a1 * a1);
  const float D = o->a > 1.0f ? mag : (o->a < 1.0f ? -mag : 0.0f);
  const float ds = D * o->X[2];
  const float ex = 1.0f - o->fx, ey = 1.0f - o->fy;
  g->tap[0] = ds * (ex * ey);
  g->tap[1] = ds * (o->fx * ey);
  g->tap[2] = ds * (ex * o->fy);
  g->tap[3] = ds * (o->fx * o->fy);
  const float dtop = o->s01 - o->s00, dbot = o->s11 - o->s10;
  const float gu = ds * (dtop + o->fy * (dbot - dtop));
  const float gt = ds * (o->bot - o->top);
  const float gc0 = bbd_div(gu, o->c2), gc1 = bbd_div(gt, o->c2);
  const float gc2 = -bbd_div(gu * o->u + gt * o->t, o->c2);
  for (int j = 0; j < 3; ++j) g->gX[j] = (cam->K[j] * gc0 + cam->K[3 + j] * gc1) + cam->K[6 + j] * gc2;
  g->gX[2] = g->gX[2] + D * o->s;
  float gp[3];
  for (int j = 0; j < 3; ++j) gp[j] = (T[j] * g->gX[0] + T[4 + j] * g->gX[1]) + T[8 + j] * g->gX[2];
  g->gq = -bbd_div((gp[0] * p[0] + gp[1] * p[1]) + gp[2] * p[2], q);
}

/* acc[12] += this sample's share of grad_T, float64. */
BBD_HD void bbd_geo_pose_add(const float* p, const BbdGeoGrad* g, double* acc) {
  for (int r = 0; r < 3; ++r) {
    const double gx = (double)g->gX[r];
    for (int j = 0; j < 3; ++j) acc[4 * r + j] += gx * (double)p[j];
    acc[4 * r + 3] += gx;
  }
}

/* The wave sum's order on 64 values (v[0] takes the total): what `v += shfl_down(v, o)` for o = 32 .. 1 gives lane 0. */
BBD_HD double bbd_geo_tree64(double* v) {
  for (int o = 32; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) v[l] += v[l + o];
  return v[0];
}

BBD_HD double bbd_geo_pair_sum(int64_t fixed) { return (double)fixed * (1.0 / BBD_GEO_SUM_ONE); }
BBD_HD float bbd_geo_tap_value(int64_t fixed, double g) { return (float)(g * ((double)fixed * (1.0 / BBD_GEO_TAP_ONE))); }

#endif /* BBD_GEO_MATH_H */
