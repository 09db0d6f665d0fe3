/* bbd_sgm_math.h - every rule of the semi-global stereo matcher (bbd_sgm_hints) that is not launch
 * geometry or a cross-lane minimum, shared by bbd_sgm.hip and its host port (tests/host_port/sgm.cpp).  Integer
 * arithmetic throughout; the only floating-point operations are the two of bbd_sgm_byte (one float32 product, one
 * float32 sum, -ffp-contract=off).  Device, port and the numpy reference of the tests agree byte for byte.
 *
 *   frame      Everything below is written in MATCHING coordinates: column x of an image with side[b] == 0 is its own
 *              column x, column x of an image with side[b] != 0 is column W - 1 - x of BOTH input images and of the
 *              output.  In matching coordinates the partner's pixel of (x, y) at disparity d is (x - d, y).  The
 *              reflection is applied where the inputs are loaded and where disp16 is stored, nowhere else.
 *   grey       per channel v = (int)floorf(c * 255.0f + 0.5f), NaN and values below 0 give 0, above 255 give 255;
 *              Y = (77 R + 150 G + 29 B + 128) >> 8                                                        (0 .. 255)
 *   census     window 9 wide x 7 high: bit k of the 64-bit word, k = 0 .. 61, is Y(clamp(x + dx), clamp(y + dy)) <
 *              Y(x, y) for the k-th offset of (dy = -3 .. 3, dx = -4 .. 4) in that order with (0, 0) left out; bits 62
 *              and 63 are 0.  Coordinates clamp to the image.
 *   cost       C(x, y, d) = popcount(cL(x, y) ^ cR(x - d, y)) for x - d >= 0, BBD_SGM_COST_OOB = 31 (half the bits)
 *              otherwise; 0 <= C <= BBD_SGM_COST_MAX = 62.
 *   paths      direction r = (dx, dy), in this order: (1,0) (-1,0) (0,1) (0,-1) | (1,1) (-1,1) (1,-1) (-1,-1); 4 paths
 *              are the first four.  With q = p - r the previous pixel of p on the path:
 *                L_r(p, d) = C(p, d)                                                   where q lies outside the image
 *                L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d - 1) + P1, L_r(q, d + 1) + P1, m + P2) - m,
 *                m = min_k L_r(q, k); the terms d - 1 < 0 and d + 1 >= D are left out.
 *              Bound: the minimum is at least m and at most m + P2, so C <= L_r <= C + P2 <= 62 + P2.  With
 *              0 < P1 < P2 <= BBD_SGM_MAX_P2 = 8129 every intermediate (L_r + P1 <= 62 + 2 * 8129 = 16320) fits 16
 *              bits, and S = the sum over 8 paths <= 8 * (62 + 8129) = 65528 <= 65535: uint16 cannot wrap.  Larger P2
 *              is refused.
 *   WTA        dL(x, y) = the d of the smallest key S * 256 + d: the lowest S, ties to the lowest d.
 *   unique     with u = uniqueness in percent (0 .. 99, 0 = off): NOT unique when some d with |d - dL| > 1 has
 *              S(d) * (100 - u) < S(dL) * 100   (OpenCV's StereoSGBM test).
 *   left-right dR(x, y) = the d in 0 .. min(D, W - x) - 1 of the smallest key S(x + d, y, d) * 256 + d.  A pixel is
 *              VALID when it is unique, x - dL >= 0 and |dR(x - dL, y) - dL| <= 1.
 *   sub-pixel  disp16 = 16 dL + o.  o = 0 at dL = 0 and dL = D - 1; else with a = S(dL - 1), c = S(dL + 1),
 *              den = max(a + c - 2 S(dL), 1):  o = floor(((a - c) * 16 + den) / (2 * den)), written with the
 *              non-negative numerator (a - c) * 16 + 33 * den, truncated, minus 16 (a - c >= -den because S(dL) is a
 *              minimum).  -8 <= o <= 8.  Invalid pixels are BBD_SGM_INVALID = -16.
 *   count      valid_count[b] = the VALID pixels of image b, counted before the fill.
 *   fill       (optional) an invalid pixel takes the value of the nearest valid pixel at a smaller x of its row, in
 *              matching coordinates; failing that of the nearest at a larger x; a row with none stays invalid.
 */
#ifndef BBD_SGM_MATH_H
#define BBD_SGM_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"

#define BBD_SGM_COST_OOB 31
#define BBD_SGM_COST_MAX 62
#define BBD_SGM_MAX_PIXELS 67108864L /* 2^26 pixels a call: with D <= 256 every index fits 2^34 */
#define BBD_SGM_MAX_BATCH 65535      /* images a call */

typedef struct BbdSgmScratch {
  uint8_t* grey;    /* [B,2,H,W] in matching coordinates, 0 = left */
  uint64_t* census; /* [B,2,H,W] */
  uint8_t* cost;    /* [B,H,W,D] */
  uint16_t* S;      /* [B,H,W,D] */
  uint32_t* sel;    /* [B,H,W]: dL | dR << 8 | not unique << 16 */
} BbdSgmScratch;

BBD_HD long bbd_sgm_align8(long n) { return (n + 7) / 8 * 8; }

/* Bytes of scratch: grey 2 P (rounded up to 8), census 16 P, cost P D, S 2 P D, sel 4 P (rounded up to 8), P = B H W.
 * `paths` does not change it.  0 for a shape the call refuses. */
BBD_HD long bbd_sgm_bytes(int B, int H, int W, int D, int paths) {
  if (B < 1 || B > BBD_SGM_MAX_BATCH || H < 1 || W < 1 || D < 64 || D > 256 || D % 64 || (paths != 4 && paths != 8)) return 0;
  if ((long)B * H > BBD_SGM_MAX_PIXELS || (long)B * H * W > BBD_SGM_MAX_PIXELS) return 0;
  const long P = (long)B * H * W;
  return bbd_sgm_align8(2 * P) + 16 * P + 3 * P * D + bbd_sgm_align8(4 * P);
}

BBD_HD void bbd_sgm_carve(void* scratch, int B, int H, int W, int D, BbdSgmScratch* s) {
  const long P = (long)B * H * W;
  uint8_t* at = (uint8_t*)scratch;
  s->grey = at;                at += bbd_sgm_align8(2 * P);
  s->census = (uint64_t*)at;   at += 16 * P;
  s->cost = at;                at += P * D;
  s->S = (uint16_t*)at;        at += 2 * P * D;
  s->sel = (uint32_t*)at;
}

BBD_HD int bbd_sgm_status(const void* left, const void* right, const void* side, const void* disp16,
                          const void* valid_count, const void* scratch, long scratch_bytes, int B, int H, int W, int D,
                          int paths, int p1, int p2, int uniqueness, int fill) {
  if (!left || !right || !side || !disp16 || !valid_count || !scratch) return BBD_E_BADARG;
  if (B < 1 || H < 1 || W < 1 || D < 64 || D > 256 || D % 64 || (paths != 4 && paths != 8)) return BBD_E_BADARG;
  if (p1 < 1 || p2 <= p1 || p2 > BBD_SGM_MAX_P2 || uniqueness < 0 || uniqueness > 99 || (fill != 0 && fill != 1))
    return BBD_E_BADARG;
  if (B > BBD_SGM_MAX_BATCH || (long)B * H > BBD_SGM_MAX_PIXELS || (long)B * H * W > BBD_SGM_MAX_PIXELS) return BBD_E_TOOMANY;
  if (((uintptr_t)scratch & 7) || scratch_bytes < bbd_sgm_bytes(B, H, W, D, paths)) return BBD_E_BADARG;
  return 0;
}

/* ---- grey ---- */
BBD_HD int bbd_sgm_byte(float c) {
  const float v = floorf(c * 255.0f + 0.5f);
  return v >= 255.0f ? 255 : v >= 0.0f ? (int)v : 0; /* a NaN fails both comparisons */
}
BBD_HD int bbd_sgm_luma(float r, float g, float b) {
  return (77 * bbd_sgm_byte(r) + 150 * bbd_sgm_byte(g) + 29 * bbd_sgm_byte(b) + 128) >> 8;
}
/* The column of the tensors that holds matching column x. */
BBD_HD int bbd_sgm_column(int x, int W, int mirrored) { return mirrored ? W - 1 - x : x; }

/* ---- census ---- */
BBD_HD int bbd_sgm_clamp(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }
BBD_HD uint64_t bbd_sgm_census(const uint8_t* grey, int H, int W, int x, int y) {
  const int centre = grey[(size_t)y * W + x];
  uint64_t word = 0;
  int k = 0;
  for (int dy = -3; dy <= 3; ++dy) {
    const uint8_t* row = grey + (size_t)bbd_sgm_clamp(y + dy, H) * W;
    for (int dx = -4; dx <= 4; ++dx) {
      if (dx == 0 && dy == 0) continue;
      word |= (uint64_t)(row[bbd_sgm_clamp(x + dx, W)] < centre) << k;
      ++k;
    }
  }
  return word;
}

/* ---- cost ---- */
BBD_HD int bbd_sgm_popcount(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}
/* `census_l`, `census_r`: the two census rows of the pixel's image row. */
BBD_HD int bbd_sgm_cost(const uint64_t* census_l, const uint64_t* census_r, int x, int d) {
  return x - d >= 0 ? bbd_sgm_popcount(census_l[x] ^ census_r[x - d]) : BBD_SGM_COST_OOB;
}

/* ---- paths ---- */
BBD_HD void bbd_sgm_direction(int r, int* dx, int* dy) {
  *dx = r == 2 || r == 3 ? 0 : (r & 1) ? -1 : 1;
  *dy = r < 2 ? 0 : (r == 2 || r == 4 || r == 5) ? 1 : -1;
}
/* The pixels of a direction are walked as LINES of `steps` pixels each.  dy == 0: a line is an image row, walked in the
 * direction of dx.  dy != 0: a line is walked over all rows in the direction of dy and starts in column `line`; its
 * column moves by dx a step and wraps round the image, and the pixel after a wrap begins a new path.  Every pixel is on
 * exactly one line, and its predecessor on the path, where it has one, is the line's pixel before it. */
BBD_HD int bbd_sgm_lines(int dy, int H, int W) { return dy == 0 ? H : W; }
BBD_HD int bbd_sgm_steps(int dy, int H, int W) { return dy == 0 ? W : H; }
/* Pixel t of a line -> (*x, *y); 1 when a path starts there (its predecessor lies outside the image). */
BBD_HD int bbd_sgm_line_pixel(int dx, int dy, int H, int W, int line, int t, int* x, int* y) {
  if (dy == 0) {
    *y = line;
    *x = dx > 0 ? t : W - 1 - t;
    return t == 0;
  }
  *y = dy > 0 ? t : H - 1 - t;
  long m = ((long)line + (long)dx * t) % W;
  if (m < 0) m += W;
  *x = (int)m;
  return t == 0 || (dx > 0 && m == 0) || (dx < 0 && m == W - 1);
}
/* One term of the recurrence: `same`, `below`, `above` = L_r(q, d), L_r(q, d - 1), L_r(q, d + 1), m = min_k L_r(q, k). */
BBD_HD int bbd_sgm_step(int c, int same, int below, int above, int has_below, int has_above, int m, int p1, int p2) {
  int best = m + p2;
  if (same < best) best = same;
  if (has_below && below + p1 < best) best = below + p1;
  if (has_above && above + p1 < best) best = above + p1;
  return c + best - m;
}

/* ---- selection ---- */
BBD_HD uint32_t bbd_sgm_key(int s, int d) { return (uint32_t)s * 256u + (uint32_t)d; }
BBD_HD int bbd_sgm_rivals(int s, int d, int best_s, int best_d, int uniqueness) {
  const int apart = d > best_d ? d - best_d : best_d - d;
  return uniqueness > 0 && apart > 1 && s * (100 - uniqueness) < best_s * 100;
}
BBD_HD uint32_t bbd_sgm_sel(int dl, int dr, int not_unique) {
  return (uint32_t)dl | (uint32_t)dr << 8 | (uint32_t)(not_unique != 0) << 16;
}
/* `sel_row`: the sel words of the pixel's image row; `s`: the D sums of the pixel. */
BBD_HD int bbd_sgm_valid(const uint32_t* sel_row, int x) {
  const uint32_t w = sel_row[x];
  const int dl = (int)(w & 255u);
  if ((w >> 16) & 1u || x - dl < 0) return 0;
  const int dr = (int)((sel_row[x - dl] >> 8) & 255u);
  return dr - dl <= 1 && dl - dr <= 1;
}
BBD_HD int bbd_sgm_disp16(const uint16_t* s, int d, int D) {
  if (d == 0 || d == D - 1) return 16 * d;
  const int a = s[d - 1], c = s[d + 1], mid = s[d];
  const int den = a + c - 2 * mid > 1 ? a + c - 2 * mid : 1;
  return 16 * d + ((a - c) * 16 + 33 * den) / (2 * den) - 16;
}

#endif /* BBD_SGM_MATH_H */
