/* bbd_align_math.h - affine-invariant depth evaluation (bbd_align.hip): a disparity-like prediction in any
 * affine gauge is aligned to the ground truth by least squares in inverse-depth space, per image, and then scored.
 * Shared with the host port of the test tier (tests/host_port/bbd_align_port.cpp): the argument rules, the per-pixel
 * terms, the finished row and - written ONCE, here - the order of every float64 addition.
 *
 *   pixels   window pixel j of the crop window cut to the map lies at (r0 + j / ww, c0 + j % ww); it is scored when
 *            min_depth < g && g < max_depth in float32 - the pixels bbd_depth_metrics scores, N of them
 *   samples  x = bbd_eval_resample_linear(pred) (float32, no reciprocal, no scale factor), t = 1.0 / (double)g
 *   sweep 1  sum x, sum t, N, the float32 minimum and maximum of x;      mx = sum x / N, mt = sum t / N
 *   sweep 2  sum (x - mx)^2, sum (x - mx)(t - mt);     scale = Sxt / Sxx, shift = mt - scale * mx
 *   sweep 3  a = scale * x + shift, capped below at 1 / max_depth; p = (float)(1.0 / a) clamped to the depth range in
 *            float32; the seven summands of bbd_depth_metrics, and sum d, sum d^2 (d = logf(p) - logf(g)), sum (1/p - 1/g)^2
 *
 *   order    EVERY float64 sum is taken the same way.  Partial k of BBD_ALIGN_THREADS (1024) starts at 0.0 and adds the
 *            summands of the scored pixels among j = k, k + 1024, k + 2048, ... in that order.  The 1024 partials are
 *            combined by bbd_align_combine: within each run of 64 (a wave) pairwise, l += l + 32, l += l + 16, ...,
 *            l += l + 1, then the 16 run sums are added to 0.0 in index order.  A function of the window alone: scale,
 *            shift and count are the same bytes on the device, in the port and from run to run.  No atomics.
 *
 * Compile with -ffp-contract=off: the device and g++ then agree to the byte on everything but logf. */
#ifndef BBD_ALIGN_MATH_H
#define BBD_ALIGN_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_eval_math.h"
#include "bbd_uncert_math.h"

#define BBD_ALIGN_THREADS 1024       /* partial sums per image: the threads of its workgroup */
#define BBD_ALIGN_LANES 64
#define BBD_ALIGN_WAVES (BBD_ALIGN_THREADS / BBD_ALIGN_LANES)
#define BBD_ALIGN_ERR_SUMS 10        /* sweep 3: abs_rel, sq_rel, (g - p)^2, d^2 in float32, a1, a2, a3, d, d^2, (1/p - 1/g)^2 */

/* Status of a call's arguments: 0 or BBD_E_BADARG. */
BBD_HD int bbd_align_status(const void* pred, const void* gt, const void* desc, const void* out, int n, int h, int w,
                            double min_depth, double max_depth, int flags) {
  if (!pred || !gt || !desc || !out || n <= 0 || h < 1 || w < 1 || flags != 0) return BBD_E_BADARG;
  if (!(min_depth >= 0.0) || !(max_depth > min_depth)) return BBD_E_BADARG;
  return 0;
}

/* The 1024 partials of one sum -> the sum; a[] is used up. */
BBD_HD double bbd_align_combine(double* a) {
  for (int wv = 0; wv < BBD_ALIGN_WAVES; ++wv)
    for (int o = BBD_ALIGN_LANES / 2; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l) a[wv * BBD_ALIGN_LANES + l] += a[wv * BBD_ALIGN_LANES + l + o];
  double s = 0.0;
  for (int wv = 0; wv < BBD_ALIGN_WAVES; ++wv) s += a[wv * BBD_ALIGN_LANES];
  return s;
}

/* Sweep 1 at a scored pixel: s = {sum x, sum t}, the running float32 extrema (a NaN is never taken). */
BBD_HD void bbd_align_sample(float x, float g, double* s, float* lo, float* hi) {
  s[0] += (double)x;
  s[1] += 1.0 / (double)g;
  *lo = x < *lo ? x : *lo;
  *hi = x > *hi ? x : *hi;
}

/* Sweep 2 at a scored pixel: s = {sum (x - mx)^2, sum (x - mx)(t - mt)}. */
BBD_HD void bbd_align_centred(float x, float g, double mx, double mt, double* s) {
  const double dx = (double)x - mx, dt = 1.0 / (double)g - mt;
  s[0] += dx * dx;
  s[1] += dx * dt;
}

/* An image the line cannot be fitted to: fewer than two scored pixels, or a prediction without spread on them. */
BBD_HD bool bbd_align_degenerate(double N, float lo, float hi) { return N < 2.0 || lo == hi; }

struct BbdAlignFit {
  double scale, shift;
};

BBD_HD BbdAlignFit bbd_align_fit(double sx, double st, double sxx, double sxt, double N) {
  const double mx = sx / N, mt = st / N;
  BbdAlignFit f;
  f.scale = sxt / sxx;
  f.shift = mt - f.scale * mx;
  return f;
}

/* The aligned depth of a sample: the disparity cap of the published protocol - a pixel the fit sends to zero or to a
 * negative disparity is scored at max_depth - then the float32 clamp of bbd_depth_metrics. */
BBD_HD float bbd_align_depth(float x, BbdAlignFit f, double max_depth, float lo, float hi) {
  double a = f.scale * (double)x + f.shift;
  const double cap = 1.0 / max_depth;
  a = a < cap ? cap : a;
  float p = (float)(1.0 / a);
  p = p < lo ? lo : p;
  p = p > hi ? hi : p;
  return p;
}

/* Sweep 3 at a scored pixel: the seven summands of bbd_depth_metrics' loop (bbd_eval.hip, float32 operations, float64
 * sums) into s[0..6], then d, d^2 and the squared inverse-depth difference, formed in float64. */
BBD_HD void bbd_align_errors(float p, float g, double* s) {
  const float t0 = g / p, t1 = p / g;
  const float th = t0 > t1 ? t0 : t1;
  s[4] += th < 1.25f ? 1.0 : 0.0;
  s[5] += th < 1.5625f ? 1.0 : 0.0;
  s[6] += th < 1.953125f ? 1.0 : 0.0;
  const float df = g - p;
  const float d2 = df * df;
  const float d = logf(p) - logf(g);               /* the log residual: minus that loop's dl, the same square */
  s[2] += (double)d2;
  s[3] += (double)(d * d);
  s[0] += (double)(fabsf(df) / g);
  s[1] += (double)(d2 / g);
  s[7] += (double)d;
  s[8] += (double)d * (double)d;
  const double di = 1.0 / (double)p - 1.0 / (double)g;
  s[9] += di * di;
}

/* Every NaN leaves as the one quiet NaN 0x7ff8000000000000.  Chosen on the bit pattern: a floating-point select
 * `v != v ? nan : v` may be folded to `v` by the compiler, and the device's sqrt of a NaN carries a sign. */
BBD_HD double bbd_align_quiet(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
  memcpy(&v, &b, sizeof v);
  return v;
}

/* The row of a degenerate image: quiet NaNs and the count. */
BBD_HD void bbd_align_empty(double N, double* out) {
  for (int j = 0; j < BBD_ALIGN_OUT; ++j) out[j] = j == 10 ? N : bbd_uncert_quiet_nan();
}

/* The row of a fitted image from the ten sums of sweep 3.  A NaN of the fit (a non-finite x among the scored pixels)
 * reaches every column as the one quiet NaN; the three threshold shares, whose compares are false on a NaN and would
 * read 0, take it from the fit. */
BBD_HD void bbd_align_finish(const double* s, double N, BbdAlignFit f, double* out) {
  const double lost = (f.scale != f.scale || f.shift != f.shift) ? bbd_uncert_quiet_nan() : 0.0;
  out[0] = bbd_align_quiet(s[0] / N);
  out[1] = bbd_align_quiet(s[1] / N);
  out[2] = bbd_align_quiet(sqrt(s[2] / N));
  out[3] = bbd_align_quiet(sqrt(s[3] / N));
  for (int k = 4; k < 7; ++k) out[k] = bbd_align_quiet(s[k] / N + lost);
  out[7] = bbd_align_quiet(f.scale);
  out[8] = bbd_align_quiet(f.shift);
  const double md = s[7] / N;
  double var = s[8] / N - md * md;
  var = var < 0.0 ? 0.0 : var;                     /* max(., 0): a NaN stays */
  out[9] = bbd_align_quiet(100.0 * sqrt(var));
  out[10] = N;
  out[11] = bbd_align_quiet(1000.0 * sqrt(s[9] / N));
}

#endif /* BBD_ALIGN_MATH_H */
