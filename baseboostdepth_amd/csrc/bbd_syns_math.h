/* bbd_syns_math.h - per-pixel arithmetic of the SYNS-Patches evaluation (evaluate_depth.py:26-102, :244-297), shared
 * by bbd_syns.hip and its host port (tests/host_port/bbd_syns_port.cpp).  Compiled with -ffp-contract=off: every
 * product and sum below is rounded where it is written.
 *
 *   L   = (d > 0) * log(max(d, 2^-23))                       to_log; log in double, rounded to float32
 *   B   = GaussianBlur 3x3, sigma 1, BORDER_REFLECT_101       float32, horizontal pass then vertical pass,
 *                                                            k1 * (a + c) + k0 * b
 *   dx, dy = 5x5 Sobel of B in float64 (smooth 1 4 6 4 1, derivative -1 -2 0 2 1, same border)
 *   mag = sqrt(dx*dx + dy*dy)                                float64
 */
#ifndef BBD_SYNS_MATH_H
#define BBD_SYNS_MATH_H

#include <math.h>
#include <stdint.h>

#include "bbd_math.h"

/* float32(exp(-x^2 / 2) / (1 + 2 exp(-1/2))) for x = 0 and x = +-1: cv2.getGaussianKernel(3, 1) cast to float32 */
#define BBD_SYNS_K0 0.45186275243759155f
#define BBD_SYNS_K1 0.2740686237812042f
#define BBD_SYNS_LOG_FLOOR 1.1920928955078125e-07f /* 2^-23 */

/* Distance transforms: vertical distances saturate at 2^15; its square, 2^30, is the "no set pixel" value.
 * (GW-1)^2 + 2^30 must stay below 2^31 and every real squared distance below 2^30: sizes with GH^2 + GW^2 >= 2^30
 * are refused (BBD_E_TOOMANY). */
#define BBD_SYNS_EDT_FAR 32768
#define BBD_SYNS_EDT_NONE 1073741824

BBD_HD int bbd_syns_reflect101(int i, int n) { /* gfedcb|abcdefgh|gfedcba; n == 1 -> 0 */
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

BBD_HD float bbd_syns_log(float d) {
  const float c = d > BBD_SYNS_LOG_FLOOR ? d : BBD_SYNS_LOG_FLOOR; /* np.clip(min=): NaN stays NaN */
  const float l = (float)log((double)(d != d ? d : c));
  return (d > 0.0f ? 1.0f : 0.0f) * l;
}

BBD_HD float bbd_syns_blur3(float a, float b, float c) { return BBD_SYNS_K1 * (a + c) + BBD_SYNS_K0 * b; }

/* B at (y, x) from the log map L [GH, GW] */
BBD_HD float bbd_syns_blur(const float* L, int y, int x, int GH, int GW) {
  const int xm = bbd_syns_reflect101(x - 1, GW), xp = bbd_syns_reflect101(x + 1, GW);
  const float* r0 = L + (size_t)bbd_syns_reflect101(y - 1, GH) * GW;
  const float* r1 = L + (size_t)y * GW;
  const float* r2 = L + (size_t)bbd_syns_reflect101(y + 1, GH) * GW;
  const float h0 = bbd_syns_blur3(r0[xm], r0[x], r0[xp]);
  const float h1 = bbd_syns_blur3(r1[xm], r1[x], r1[xp]);
  const float h2 = bbd_syns_blur3(r2[xm], r2[x], r2[xp]);
  return bbd_syns_blur3(h0, h1, h2);
}

/* Gradient magnitude at (y, x) from the blurred map B [GH, GW]: rows top to bottom, taps left to right. */
BBD_HD double bbd_syns_sobel_mag(const float* B, int y, int x, int GH, int GW) {
  const double sm[5] = {1.0, 4.0, 6.0, 4.0, 1.0}, dv[5] = {-1.0, -2.0, 0.0, 2.0, 1.0};
  int xs[5];
  for (int i = 0; i < 5; ++i) xs[i] = bbd_syns_reflect101(x + i - 2, GW);
  double dx = 0.0, dy = 0.0;
  for (int j = 0; j < 5; ++j) {
    const float* r = B + (size_t)bbd_syns_reflect101(y + j - 2, GH) * GW;
    double rd = 0.0, rs = 0.0;
    for (int i = 0; i < 5; ++i) {
      const double v = (double)r[xs[i]];
      rd += dv[i] * v;
      rs += sm[i] * v;
    }
    dx += sm[j] * rd;
    dy += dv[j] * rs;
  }
  return sqrt(dx * dx + dy * dy);
}

/* Squared distance between two points, from the differences. */
BBD_HD float bbd_syns_dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

/* Ray of flat pixel k of a GH x GW map times its depth: depth * inv_K[:3,:3] (u, v, 1).
 * reference rays (BBD_SYNS_RAYS_PIXEL clear): u = k / GH, v = k % GH - evaluate_depth.py:31-32 builds the grid with
 * torch.meshgrid(arange(w), arange(h)) in ij order and flattens it against the row-major depth map;
 * pixel rays: u = k % GW, v = k / GW.  Row j: ((K[j][0] * u + K[j][1] * v) + K[j][2]) * depth, float32. */
BBD_HD void bbd_syns_backproject(const float* iK, int k, int GH, int GW, int pixel_rays, float depth, float* p) {
  const float u = (float)(pixel_rays ? k % GW : k / GH), v = (float)(pixel_rays ? k / GW : k % GH);
  for (int j = 0; j < 3; ++j) p[j] = ((iK[3 * j] * u + iK[3 * j + 1] * v) + iK[3 * j + 2]) * depth;
}

/* Precision, recall -> F-score and IoU (evaluate_depth.py:49-55), float32, in the reference's order. */
BBD_HD void bbd_syns_f_iou(float P, float R, float* f, float* iou) {
  if (P < 1e-3f && R < 1e-3f) {
    *f = P;
    *iou = P;
    return;
  }
  *f = ((2.0f * P) * R) / (P + R);
  *iou = (P * R) / ((P + R) - (P * R));
}

#endif /* BBD_SYNS_MATH_H */
