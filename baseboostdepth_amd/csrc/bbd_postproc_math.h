/* bbd_postproc_math.h - per-pixel arithmetic of the flip post-processing of a disparity (bbd_postproc.hip), shared
 * with the host port of the test tier (tests/host_port/bbd_postproc_port.cpp).  Restates Monodepth2's
 * batch_post_process_disparity(l_disp, r_disp) with r_disp the prediction of the flipped image, flipped back:
 *
 *   m      = 0.5 * (l_disp + r_disp)                              float32
 *   l      = np.linspace(0, 1, w)  along x                        float64
 *   l_mask = 1 - np.clip(20 * (l - 0.05), 0, 1);  r_mask = l_mask[:, :, ::-1]
 *   out    = r_mask * l_disp + l_mask * r_disp + (1 - l_mask - r_mask) * m          float64
 *
 * rounded once to float32 (the scoring kernels take float32; Monodepth2 keeps the float64).
 * Compile with -ffp-contract=off: every rounding below is one numpy performs. */
#ifndef BBD_POSTPROC_MATH_H
#define BBD_POSTPROC_MATH_H

#include "bbd_math.h"

/* np.linspace(0, 1, w): step = 1 / (w - 1) once, element x = x * step, the last element set to 1.  The division is done
 * once per call on the host and handed to the kernel, so that no device division takes part. */
BBD_HD double bbd_postproc_step(int w) { return w > 1 ? 1.0 / (double)(w - 1) : 0.0; }

BBD_HD double bbd_postproc_lin(int x, int w, double step) {
  if (w == 1) return 0.0;
  if (x == w - 1) return 1.0;
  return (double)x * step;
}

/* l_mask at column x: 1 up to 5 % of the width, a ramp down to 0 at 10 %. */
BBD_HD double bbd_postproc_mask(int x, int w, double step) {
  const double d = bbd_postproc_lin(x, w, step) - 0.05;
  double t = 20.0 * d;
  t = t > 0.0 ? t : 0.0;
  t = t < 1.0 ? t : 1.0;
  return 1.0 - t;
}

/* ld = the prediction at (y, x); rd = the flipped image's prediction at (y, w-1-x); a = l_mask(x), b = l_mask(w-1-x). */
BBD_HD float bbd_postproc_blend(float ld, float rd, double a, double b) {
  const float s = ld + rd;
  const float m = s * 0.5f;
  const double pl = b * (double)ld;
  const double pr = a * (double)rd;
  const double c = (1.0 - a) - b;
  const double pm = c * (double)m;
  return (float)((pl + pr) + pm);
}

#endif /* BBD_POSTPROC_MATH_H */
