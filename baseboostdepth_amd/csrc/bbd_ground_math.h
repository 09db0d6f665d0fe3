/* bbd_ground_math.h - everything of bbd_ground_scale that is not launch geometry, shared by bbd_ground.hip and its host
 * port (tests/host_port/bbd_ground_port.cpp): the argument rules, the depth of a pixel, the ground test of an interior
 * pixel and the output row.  Compiled with -ffp-contract=off: every product, sum, quotient and square root below is one
 * IEEE float32 operation, rounded where it is written.
 *
 *   depth   d = pred, or d = 1.0f / pred (BBD_EVAL_PRED_IS_DISP); valid when d > 0 and finite
 *   point   P = bbd_syns_backproject(inv_K[i], y * w + x, h, w, 1, d)             (bbd_syns_math.h; bbd_ground_point)
 *   candidate  interior pixel (1 <= x <= w-2, 1 <= y <= h-2) whose nine pixels are all valid
 *   normal  v_k = P_k - P_c over the ring (x+1,y) (x+1,y+1) (x,y+1) (x-1,y+1) (x-1,y) (x-1,y-1) (x,y-1) (x+1,y-1)
 *           c_k = v_k x v_(k+1) mod 8;  N = ((((((c_0 + c_1) + c_2) + c_3) + c_4) + c_5) + c_6) + c_7
 *           (for flat ground under a camera with x right, y down, z forward, N points to +y)
 *   ground  n2 = (N.x*N.x + N.y*N.y) + N.z*N.z;  len = sqrtf(n2);  cosv = N.y / len
 *           ht = ((N.x*P.x + N.y*P.y) + N.z*P.z) / len
 *           ground when len > 0 and finite, cosv > cos_threshold, P.y > 0, ht > 0 and finite
 *   code    what the first launch leaves in the scratch map: ht at a ground pixel, zero elsewhere - the zero of a
 *           candidate that is not ground carries the sign bit (-0.0f), so that the select launch counts the candidates
 *           in the sweep it makes anyway and never reads the prediction
 *   row     [0] median, [1] count, [2] candidates, [7] camera_height / median, others 0; [0] and [7] are the quiet NaN
 *           0x7fc00000 where count < max(min_count, 1)
 */
#ifndef BBD_GROUND_MATH_H
#define BBD_GROUND_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_syns_math.h"

#define BBD_GROUND_FLAGS BBD_EVAL_PRED_IS_DISP
#define BBD_GROUND_CODE_CANDIDATE 0x80000000u /* bits of -0.0f */
#define BBD_GROUND_NAN 0x7fc00000u

/* Status of a call's arguments: 0, BBD_E_BADARG or BBD_E_TOOMANY. */
BBD_HD int bbd_ground_args_status(const void* pred, const void* inv_K, const void* rows, const void* scratch, int n,
                                  int h, int w, double camera_height, double cos_threshold, int min_count, int flags) {
  if (!pred || !inv_K || !rows || !scratch) return BBD_E_BADARG;
  if (n < 1 || h < 1 || w < 1) return BBD_E_BADARG;
  if (!(camera_height > 0.0)) return BBD_E_BADARG;                       /* a NaN is refused as well */
  if (!(cos_threshold > 0.0 && cos_threshold <= 1.0)) return BBD_E_BADARG;
  if (min_count < 0 || (flags & ~BBD_GROUND_FLAGS)) return BBD_E_BADARG;
  if (n > 65535 || (long)h * (long)w > 0x7fffffffL) return BBD_E_TOOMANY;
  return 0;
}

/* Floats of the scratch map of a call: n * h * w, or the status above for sizes no call takes. */
BBD_HD long bbd_ground_scratch_floats(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return BBD_E_BADARG;
  if (n > 65535 || (long)h * (long)w > 0x7fffffffL) return BBD_E_TOOMANY;
  return (long)n * (long)h * (long)w;
}

BBD_HD uint32_t bbd_ground_float_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}
BBD_HD float bbd_ground_bits_float(uint32_t b) {
  float v;
  memcpy(&v, &b, 4);
  return v;
}

BBD_HD float bbd_ground_depth(float pred, int flags) { return (flags & BBD_EVAL_PRED_IS_DISP) ? 1.0f / pred : pred; }

BBD_HD int bbd_ground_finite(float v) { return (bbd_ground_float_bits(v) & 0x7f800000u) != 0x7f800000u; }

BBD_HD int bbd_ground_valid(float d) { return d > 0.0f && bbd_ground_finite(d); }

/* bbd_syns_backproject(iK, y * w + x, h, w, 1, d, p) operation for operation, without the division that takes the flat
 * index apart again. */
BBD_HD void bbd_ground_point(const float* iK, int x, int y, float d, float* p) {
  const float u = (float)x, v = (float)y;
  for (int j = 0; j < 3; ++j) p[j] = ((iK[3 * j] * u + iK[3 * j + 1] * v) + iK[3 * j + 2]) * d;
}

/* The scratch code of interior pixel (x, y): dc its depth, dr the depths of its ring in the order above. */
BBD_HD float bbd_ground_code(const float* iK, int x, int y, float dc, const float dr[8], float cos_threshold) {
  const int rx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, ry[8] = {0, 1, 1, 1, 0, -1, -1, -1};
  int valid = bbd_ground_valid(dc);
  for (int k = 0; k < 8; ++k) valid &= bbd_ground_valid(dr[k]);
  if (!valid) return 0.0f;
  const float not_ground = bbd_ground_bits_float(BBD_GROUND_CODE_CANDIDATE);
  float P[3], v[8][3];
  bbd_ground_point(iK, x, y, dc, P);
  for (int k = 0; k < 8; ++k) {
    float q[3];
    bbd_ground_point(iK, x + rx[k], y + ry[k], dr[k], q);
    v[k][0] = q[0] - P[0];
    v[k][1] = q[1] - P[1];
    v[k][2] = q[2] - P[2];
  }
  float N[3] = {0.0f, 0.0f, 0.0f};
  for (int k = 0; k < 8; ++k) {
    const float* a = v[k];
    const float* b = v[(k + 1) & 7];
    const float cx = a[1] * b[2] - a[2] * b[1];
    const float cy = a[2] * b[0] - a[0] * b[2];
    const float cz = a[0] * b[1] - a[1] * b[0];
    if (k == 0) {
      N[0] = cx; N[1] = cy; N[2] = cz;
    } else {
      N[0] = N[0] + cx; N[1] = N[1] + cy; N[2] = N[2] + cz;
    }
  }
  const float n2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
  const float len = sqrtf(n2);
  const float cosv = N[1] / len;
  const float ht = ((N[0] * P[0] + N[1] * P[1]) + N[2] * P[2]) / len;
  const int ground = len > 0.0f && bbd_ground_finite(len) && cosv > cos_threshold && P[1] > 0.0f && ht > 0.0f &&
                     bbd_ground_finite(ht);
  return ground ? ht : not_ground;
}

/* The BBD_EVAL_OUT columns of an image: `median_bits` is the bit pattern of the element of rank (count - 1) / 2 of its
 * ascending heights (unread where count is 0). */
BBD_HD float bbd_ground_row(int column, uint32_t median_bits, uint32_t count, uint32_t candidates, int min_count,
                            float camera_height) {
  const uint32_t need = min_count > 1 ? (uint32_t)min_count : 1u;
  const float median = bbd_ground_bits_float(count < need ? BBD_GROUND_NAN : median_bits);
  switch (column) {
    case 0: return median;
    case 1: return (float)count;
    case 2: return (float)candidates;
    case 7: return count < need ? median : camera_height / median;
    default: return 0.0f;
  }
}

#endif /* BBD_GROUND_MATH_H */
