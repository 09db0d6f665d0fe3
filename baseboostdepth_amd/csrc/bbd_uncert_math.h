/* bbd_uncert_math.h - depth uncertainty from the flip pass and its sparsification scores (bbd_uncert.hip), shared with
 * the host port of the test tier (tests/host_port/bbd_uncert_port.cpp): the argument rules, the scratch layout, the
 * per-pixel terms, the sort key and - written ONCE, here - the order of every float64 addition.
 *
 *   terms    at a pixel bbd_depth_metrics scores (bbd_eval.hip:129-148, float32, one IEEE operation each):
 *              p = bbd_eval_resample(disparity) [* ratio], clamped;  df = g - p
 *              e_abs = fabsf(df) / g;  e_sq = df * df;  th = max(g / p, p / g);  a1 = th < 1.25f
 *              u = bbd_eval_resample_linear(uncertainty map)
 *   order    by key descending, pixel order ascending among equal keys: a STABLE ascending sort of bbd_uncert_sort_key
 *   buckets  bucket b of K holds ranks [floor(b N / K), floor((b + 1) N / K)); lane l of BBD_UNCERT_LANES adds ranks
 *            first + l, first + l + 64, ... in that order (bbd_uncert_lane_sums), the 64 lane sums are added pairwise,
 *            l += l + 32, l += l + 16, ... (bbd_uncert_tree) - a function of N and K only
 *   curves   suffix sums from the last bucket down, the three metrics, trapezoids, AUSE / AURG (bbd_uncert_finish)
 *
 * Compile with -ffp-contract=off: the device and g++ then agree to the byte (float64 sums, divisions, square roots). */
#ifndef BBD_UNCERT_MATH_H
#define BBD_UNCERT_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_eval_math.h"
#include "bbd_ragged_math.h"
#include "bbd_viz_math.h"

#define BBD_UNCERT_CHUNK 1024        /* pixels (then sorted slots) per workgroup */
#define BBD_UNCERT_LANES 64
#define BBD_UNCERT_NAN_BITS 0x7fc00000u
#define BBD_UNCERT_BSUMS (6 * BBD_SPARS_MAX_INTERVALS)     /* doubles per image: [sparse, oracle][abs, sq, a1][K] */

/* The crop window of a BBD_EVAL_DESC row, cut to the map: `area` pixels, pixel j at (r0 + j / ww, c0 + j % ww). */
struct BbdUncertWindow {
  size_t off;
  int GH, GW, r0, c0, ww;
  long area;
};

BBD_HD BbdUncertWindow bbd_uncert_window(const int32_t* desc, int i) {
  const BbdEvalRow m = bbd_eval_row(desc, i);
  BbdUncertWindow v;
  v.off = m.off; v.GH = m.GH; v.GW = m.GW;
  const int r0 = m.r0 < 0 ? 0 : m.r0, r1 = m.r1 > m.GH ? m.GH : m.r1;
  const int c0 = m.c0 < 0 ? 0 : m.c0, c1 = m.c1 > m.GW ? m.GW : m.c1;
  v.r0 = r0; v.c0 = c0;
  v.ww = c1 > c0 ? c1 - c0 : 0;
  v.area = (r1 > r0 && c1 > c0) ? (long)(r1 - r0) * (long)(c1 - c0) : 0;
  return v;
}

/* Where the pieces of the scratch lie (byte offsets), for P window pixels and n images.  The call cannot see the
 * windows from the host: the capacity P is READ from scratch_bytes, which must be the header's formula for a whole P. */
struct BbdUncertLayout {
  long P, C;                /* pixel capacity; chunk capacity P / BBD_UNCERT_CHUNK + n */
  size_t pix_off;           /* int64 [n + 1]   first slot of image i */
  size_t bsum;              /* double [n, BBD_UNCERT_BSUMS] bucket sums */
  size_t keys, order;       /* uint32 [2 buffers, 4 orderings, P] each: sort keys and the slots they belong to */
  size_t e_abs, e_sq, th;   /* float [P] each, by slot */
  size_t chunk_off;         /* int32 [n + 1]   first chunk of image i */
  size_t count;             /* int32 [n]       N */
  size_t chunk_total;       /* int32 [C]       valid pixels of a chunk, then their exclusive prefix in the image */
  size_t hist;              /* uint32 [4, C, 256] digit counts of a chunk, then the first rank of (digit, chunk) */
  size_t end;
};

BBD_HD int bbd_uncert_layout(long scratch_bytes, int n, BbdUncertLayout* L) {
  const long fixed = (long)BBD_SPARS_SCRATCH_CALL + (long)n * BBD_SPARS_SCRATCH_IMAGE;
  if (scratch_bytes < fixed || (scratch_bytes - fixed) % BBD_SPARS_SCRATCH_PIXEL != 0) return BBD_E_BADARG;
  const long P = (scratch_bytes - fixed) / BBD_SPARS_SCRATCH_PIXEL;
  if (P > 0x7fffffffL - 2 * BBD_UNCERT_CHUNK) return BBD_E_BADARG;
  const long C = P / BBD_UNCERT_CHUNK + n;
  size_t at = 64;                                      /* [0, 64): int32 flag "the windows do not fit" */
  L->P = P; L->C = C;
  L->pix_off = at;     at += 8 * ((size_t)n + 1);
  L->bsum = at;        at += 8 * (size_t)BBD_UNCERT_BSUMS * (size_t)n;
  L->keys = at;        at += 4 * 8 * (size_t)P;
  L->order = at;       at += 4 * 8 * (size_t)P;
  L->e_abs = at;       at += 4 * (size_t)P;
  L->e_sq = at;        at += 4 * (size_t)P;
  L->th = at;          at += 4 * (size_t)P;
  L->chunk_off = at;   at += 4 * ((size_t)n + 1);
  L->count = at;       at += 4 * (size_t)n;
  L->chunk_total = at; at += 4 * (size_t)C;
  L->hist = at;        at += 4 * 4 * 256 * (size_t)C;
  L->end = at;
  return at <= (size_t)scratch_bytes ? 0 : BBD_E_BADARG;     /* holds for every P and n: see the header's formula */
}

/* Status of a call's arguments: 0 or BBD_E_BADARG; *L is the scratch layout then. */
BBD_HD int bbd_uncert_status(const void* pred, const void* uncert, const void* gt, const void* desc, const void* rows,
                             const void* out, const void* scratch, long scratch_bytes, int n, int h, int w,
                             int intervals, int flags, BbdUncertLayout* L) {
  if (!pred || !uncert || !gt || !desc || !rows || !out || !scratch) return BBD_E_BADARG;
  if (n < 1 || n > 65535 || h < 1 || w < 1 || intervals < 1 || intervals > BBD_SPARS_MAX_INTERVALS) return BBD_E_BADARG;
  if (flags & ~BBD_EVAL_NO_MEDIAN_SCALING) return BBD_E_BADARG;
  if (((uintptr_t)scratch & 7u) != 0) return BBD_E_BADARG;
  return bbd_uncert_layout(scratch_bytes, n, L);
}

/* uncert[i][y][x] of the flip pass: one float32 subtraction. */
BBD_HD float bbd_uncert_flip(float ld, float rd) { return fabsf(ld - rd); }

/* Does bbd_depth_metrics score a pixel of depth g? */
BBD_HD bool bbd_uncert_valid(float g, float min_depth, float max_depth) { return g > min_depth && g < max_depth; }

struct BbdUncertTerms {
  float u, e_abs, e_sq, th;
};

/* The terms of the valid pixel (y, x) of a GH x GW map with depth g; pred and uncert are the image's [h,w] planes. */
BBD_HD BbdUncertTerms bbd_uncert_terms(const float* pred, const float* uncert, int h, int w, float g, int y, int x,
                                       int GH, int GW, float min_depth, float max_depth, float scale_factor,
                                       float ratio, int flags) {
  float p = bbd_eval_resample(pred, h, w, scale_factor, 0.0f, 0.0f, BBD_EVAL_PRED_IS_DISP, y, x, GH, GW);
  if (!(flags & BBD_EVAL_NO_MEDIAN_SCALING)) p *= ratio;
  p = p < min_depth ? min_depth : p;
  p = p > max_depth ? max_depth : p;
  BbdUncertTerms t;
  const float df = g - p;
  t.e_abs = fabsf(df) / g;
  t.e_sq = df * df;
  const float t0 = g / p, t1 = p / g;
  t.th = t0 > t1 ? t0 : t1;
  t.u = bbd_eval_resample_linear(uncert, h, w, y, x, GH, GW);
  return t;
}

/* Key of a stable ASCENDING sort that leaves the values descending: every NaN becomes 0x7fc00000 and -0 becomes +0,
 * the monotone order key of that float (a NaN above +inf) is inverted. */
BBD_HD uint32_t bbd_uncert_sort_key(float v) {
  if (v != v) v = bbd_viz_bits_float(BBD_UNCERT_NAN_BITS);
  if (v == 0.0f) v = 0.0f;
  return ~bbd_viz_order_key(v);
}

/* First rank of bucket k of K over N ranked pixels; bucket K - 1 ends at N. */
BBD_HD long bbd_uncert_rank(int k, long N, int K) { return k >= K ? N : (long)k * N / (long)K; }

/* Lane `lane` of BBD_UNCERT_LANES over the ranks [first, last) of an ordering (`order` = its slots by rank): the sums
 * of e_abs and e_sq as doubles and the number of a1 pixels, rank by rank upwards. */
BBD_HD void bbd_uncert_lane_sums(const float* e_abs, const float* e_sq, const float* th, const uint32_t* order,
                                 long first, long last, int lane, double s[3]) {
  double s_abs = 0.0, s_sq = 0.0;
  long a1 = 0;
  for (long r = first + lane; r < last; r += BBD_UNCERT_LANES) {
    const uint32_t slot = order[r];
    s_abs += (double)e_abs[slot];
    s_sq += (double)e_sq[slot];
    a1 += th[slot] < 1.25f ? 1 : 0;
  }
  s[0] = s_abs; s[1] = s_sq; s[2] = (double)a1;
}

/* The 64 lane sums of a bucket, added pairwise; a[] is used up. */
BBD_HD double bbd_uncert_tree(double* a) {
  for (int o = BBD_UNCERT_LANES / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) a[l] += a[l + o];
  return a[0];
}

BBD_HD double bbd_uncert_trapz(const double* c, int K) {
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += (c[k] + c[k + 1]) / 2.0;
  return s / (double)K;
}

BBD_HD double bbd_uncert_quiet_nan(void) { return (double)bbd_viz_bits_float(BBD_UNCERT_NAN_BITS); }

/* One curve [K + 1] of metric 0 abs_rel, 1 rmse, 2 a1 from its K bucket sums b: S_k = bucket k + S_(k+1), from the last
 * bucket down; a NaN prediction's NaNs leave as the one quiet NaN. */
BBD_HD void bbd_uncert_curve(const double* b, long N, int K, int metric, double* curve) {
  double suffix = 0.0;
  for (int k = K - 1; k >= 0; --k) {
    suffix = b[k] + suffix;
    const double left = (double)(N - bbd_uncert_rank(k, N, K));
    const double mean = suffix / left;
    const double v = metric == 1 ? sqrt(mean) : mean;
    curve[k] = v != v ? bbd_uncert_quiet_nan() : v;
  }
  curve[K] = metric == 2 ? 1.0 : 0.0;
}

/* AUSE and AURG of one metric from the finished curves [2][3][K + 1] into summary[metric] and summary[3 + metric]. */
BBD_HD void bbd_uncert_scores(const double* curves, int K, int metric, double* summary) {
  const double* sparse = curves + (size_t)metric * (K + 1);
  const double* oracle = curves + (size_t)(3 + metric) * (K + 1);
  const double ts = bbd_uncert_trapz(sparse, K), to = bbd_uncert_trapz(oracle, K);
  const double ause = metric == 2 ? to - ts : ts - to;
  const double aurg = metric == 2 ? ts - sparse[0] : sparse[0] - ts;
  summary[metric] = ause != ause ? bbd_uncert_quiet_nan() : ause;
  summary[3 + metric] = aurg != aurg ? bbd_uncert_quiet_nan() : aurg;
}

/* Element j of the row of an image without a scored pixel (N = 0), or of any image when the windows do not fit. */
BBD_HD double bbd_uncert_empty(int j, bool fits) {
  return j == 7 || (j == 6 && fits) ? 0.0 : bbd_uncert_quiet_nan();
}

/* One image's row of `out` from its bucket sums bsum [6, BBD_SPARS_MAX_INTERVALS] (sparse abs, sq, a1; oracle abs, sq,
 * a1; K used of each): out = {AUSE abs_rel, rmse, a1, AURG abs_rel, rmse, a1, N, 0} and the curves [2][3][K + 1].  The
 * kernel gives the six curves and the three metrics a lane each; the pieces are these. */
BBD_HD void bbd_uncert_finish(const double* bsum, long N, int K, bool fits, double* out) {
  const int width = BBD_SPARS_SUMMARY + 6 * (K + 1);
  if (N < 1 || !fits) {
    for (int j = 0; j < width; ++j) out[j] = bbd_uncert_empty(j, fits);
    return;
  }
  for (int c = 0; c < 6; ++c)
    bbd_uncert_curve(bsum + (size_t)c * BBD_SPARS_MAX_INTERVALS, N, K, c % 3, out + BBD_SPARS_SUMMARY + (size_t)c * (K + 1));
  for (int metric = 0; metric < 3; ++metric) bbd_uncert_scores(out + BBD_SPARS_SUMMARY, K, metric, out);
  out[6] = (double)N;
  out[7] = 0.0;
}

#endif /* BBD_UNCERT_MATH_H */
