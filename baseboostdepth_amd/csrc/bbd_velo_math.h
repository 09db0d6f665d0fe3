/* bbd_velo_math.h - per-point arithmetic of the Velodyne depth maps (bbd_velo.hip), shared with the host port of the
 * test tier (tests/host_port/bbd_velo_port.cpp).  Restates kitti_utils.py:64-96 for one point p = (x, y, z, 1):
 *
 *   keep      x >= 0 in float32                               (-0.0 passes, NaN does not)
 *   q         = P p, P float64 [3,4], p widened to float64
 *   u, v      = rint(q0 / q2) - 1, rint(q1 / q2) - 1          np.round: half to even
 *   depth     = x (vel_depth) or q2
 *   valid     0 <= u < w and 0 <= v < h, compared in float64  (NaN and inf fall out before any integer conversion)
 *   pixel     v * w + u
 *   key       v * (w - 1) + u - 1                             sub2ind of kitti_utils.py:39-43, see bbd_velo_key
 *
 * Order of the fp64 operations, chosen here and the same on both sides: each q_i is the left-to-right sum
 * ((P[i][0] * x + P[i][1] * y) + P[i][2] * z) + P[i][3], four roundings of products that are rounded on their own (no
 * FMA), the homogeneous 1 not multiplied.  numpy hands the same product to BLAS, whose order (and use of FMA) is its
 * own: q can differ from the reference in the last bits, which moves a pixel only when q0/q2 or q1/q2 sits within
 * about 1e-13 of a half-integer, and the recorded depth q2 by at most one float32 ulp after the cast.
 * Compile with -ffp-contract=off. */
#ifndef BBD_VELO_MATH_H
#define BBD_VELO_MATH_H

#include <math.h>
#include <stdint.h>

#include "bbd_viz_math.h" /* bbd_viz_float_bits, bbd_viz_order_key, bbd_viz_key_value */

typedef struct bbd_velo_hit {
  int32_t pixel; /* v * w + u */
  int32_t key;   /* sub2ind + 1, in [0, h * w - h] */
  float depth;   /* float32 image of the float64 depth, see bbd_velo_depth32 */
} bbd_velo_hit_t;

BBD_HD double bbd_velo_row(const double* r, double x, double y, double z) {
  const double a = r[0] * x;
  const double b = r[1] * y;
  const double c = r[2] * z;
  double s = a + b;
  s = s + c;
  return s + r[3];
}

/* The reference keeps depths in float64, takes minima there, zeroes what is negative and only then casts to float32
 * (export_gt_depth.py:77).  Rounding is monotone, so the minimum and the "last write" commute with the cast; the sign
 * test does not where a negative float64 underflows to -0.0f.  Such a value is moved to the smallest negative
 * subnormal, which keeps the map monotone and the sign test exact. */
BBD_HD float bbd_velo_depth32(double d) {
  const float f = (float)d;
  return (d < 0.0 && !(f < 0.0f)) ? bbd_viz_bits_float(0x80000001u) : f;
}

/* depth[depth < 0] = 0 (kitti_utils.py:96): -0.0 stays what it is, as in the reference. */
BBD_HD float bbd_velo_finish(float d) { return d < 0.0f ? 0.0f : d; }

/* sub2ind(matrixSize, rowSub, colSub) = rowSub * (n - 1) + colSub - 1 (kitti_utils.py:39-43) multiplies the row by
 * w - 1, not w, so it is NOT a unique pixel index: (r, w - 1) and (r + 1, 0) share one.  That collision is part of the
 * ground truth every user of the reference evaluates against and is reproduced on purpose.  Shifted by one so that the
 * smallest key, -1 at pixel (0, 0), indexes a table. */
BBD_HD int32_t bbd_velo_key(int32_t v, int32_t u, int32_t w) { return v * (w - 1) + u; }

/* One point against one frame; returns 0 when the point leaves no trace. */
BBD_HD int bbd_velo_project(const double* P, float x, float y, float z, int h, int w, int vel_depth, bbd_velo_hit_t* hit) {
  if (!(x >= 0.0f)) return 0;
  const double dx = (double)x, dy = (double)y, dz = (double)z;
  const double q0 = bbd_velo_row(P, dx, dy, dz);
  const double q1 = bbd_velo_row(P + 4, dx, dy, dz);
  const double q2 = bbd_velo_row(P + 8, dx, dy, dz);
  const double u = rint(q0 / q2) - 1.0;
  const double v = rint(q1 / q2) - 1.0;
  if (!(u >= 0.0 && v >= 0.0 && u < (double)w && v < (double)h)) return 0;
  const int32_t ui = (int32_t)u, vi = (int32_t)v;
  hit->pixel = vi * w + ui;
  hit->key = bbd_velo_key(vi, ui, w);
  hit->depth = bbd_velo_depth32(vel_depth ? dx : q2);
  return 1;
}

#endif /* BBD_VELO_MATH_H */
