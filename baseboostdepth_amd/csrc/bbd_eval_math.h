/* bbd_eval_math.h - the prediction at a ground-truth pixel, shared by bbd_eval.hip (KITTI metrics) and bbd_syns.hip
 * (SYNS edge / point-cloud metrics) and by their host ports.  Moved here from bbd_eval.hip unchanged: the same
 * operations in the same order.  bbd_eval_resample_linear is the resize alone: bbd_uncert.hip resamples an uncertainty
 * map with it, at the taps and weights the disparity gets. */
#ifndef BBD_EVAL_MATH_H
#define BBD_EVAL_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"

/* cv2.resize(img, (GW, GH)) - INTER_LINEAR on float32 - at pixel (y, x): half-pixel centres, coordinate in double ->
 * float, edge taps collapse to weight 0, horizontal pass then vertical pass, products and sums rounded separately. */
BBD_HD float bbd_eval_resample_linear(const float* img, int h, int w, int y, int x, int GH, int GW) {
  const double sx_ = (double)w / (double)GW, sy_ = (double)h / (double)GH;
  float fx = (float)(((double)x + 0.5) * sx_ - 0.5);
  float fy = (float)(((double)y + 0.5) * sy_ - 0.5);
  int ix = (int)floorf(fx), iy = (int)floorf(fy);
  fx -= (float)ix;
  fy -= (float)iy;
  if (ix < 0) { ix = 0; fx = 0.0f; }
  if (ix >= w - 1) { ix = w - 1; fx = 0.0f; }
  if (iy < 0) { iy = 0; fy = 0.0f; }
  if (iy >= h - 1) { iy = h - 1; fy = 0.0f; }
  const int ix1 = ix < w - 1 ? ix + 1 : ix, iy1 = iy < h - 1 ? iy + 1 : iy;
  const float* r0 = img + (size_t)iy * w;
  const float* r1 = img + (size_t)iy1 * w;
  const float top = r0[ix] * (1.0f - fx) + r0[ix1] * fx;
  const float bot = r1[ix] * (1.0f - fx) + r1[ix1] * fx;
  return top * (1.0f - fy) + bot * fy;
}

/* Prediction `img` [h,w] at ground-truth pixel (y, x) of a GH x GW map. */
BBD_HD float bbd_eval_resample(const float* img, int h, int w, float scale_factor, float clamp_lo, float clamp_hi,
                               int flags, int y, int x, int GH, int GW) {
  if (flags & BBD_EVAL_PRED_IS_DISP) {
    /* cv2.resize(pred_disp, (gt_width, gt_height)) (evaluate_depth.py:248); then pred_depth = 1 / pred_disp. */
    const float d = bbd_eval_resample_linear(img, h, w, y, x, GH, GW);
    return (1.0f / d) * scale_factor;            /* evaluate_depth.py:252, :275 */
  }
  /* F.interpolate(depth_pred, [gt_h, gt_w], bilinear, align_corners=False) then clamp (trainer.py:599) */
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  bbd_up_src(y, h, GH, &y0, &y1, &ly0, &ly1);
  bbd_up_src(x, w, GW, &x0, &x1, &lx0, &lx1);
  const float* r0 = img + (size_t)y0 * w;
  const float* r1 = img + (size_t)y1 * w;
  float v = bbd_up_blend(r0[x0], r0[x1], r1[x0], r1[x1], ly0, ly1, lx0, lx1, GH + GW <= 128);
  v = v < clamp_lo ? clamp_lo : v;             /* torch.clamp: NaN propagates */
  v = v > clamp_hi ? clamp_hi : v;
  return v;
}

#endif /* BBD_EVAL_MATH_H */
