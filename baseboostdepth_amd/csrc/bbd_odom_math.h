/* bbd_odom_math.h - arithmetic of the KITTI odometry evaluation (bbd_odom.hip), shared with the host port of the test
 * tier (tests/host_port/bbd_odom_port.cpp).  Restates evaluate_pose.py:18-41, :101-116 and :125-159.
 *
 *   chained     T = eye; for step in steps[::-1]: T = T @ step, float32: T = step_{S-1} @ ... @ step_0, multiplied left to
 *               right, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 like torch.matmul on the CPU (mul4 of bbd_pose.hip);
 *               eye @ X is X exactly, so the first factor is copied
 *   gt_local    inv(inv(G[j]) . G[j+S]) in float64, G = the 3x4 row of the poses file over (0 0 0 1).  The inverse is the
 *               GENERAL one (Gauss-Jordan, partial pivoting): the file's rotations are printed to 7 digits and are not
 *               orthonormal, and the reference calls np.linalg.inv
 *   track       dump_xyz + compute_ate for n poses: cam_to_world accumulated in float64 (a float32 prediction is widened
 *               first), xyz_0 = 0, offset = gt_xyz[0] - pred_xyz[0], scale = sum(gt * pred) / sum(pred^2),
 *               ate = sqrt(sum((pred * scale - gt)^2)) / (n + 1); 0 / 0 stays NaN
 *   summary     np.mean and np.std (population) of a row of ATEs: BBD_ODOM_LANES strided partial sums, then a halving tree
 *
 * Every sum is sequential in the order written here and every product is rounded on its own (compile with
 * -ffp-contract=off), the same on both sides.  numpy hands its 4x4 products to BLAS and sums pairwise: the reference's
 * float64 results differ from these in the last bits (DESIGN.md 6d has the bound the tests use).  A NaN is written as
 * the one quiet NaN 0x7ff8000000000000, whatever sign or payload the hardware's 0 / 0 has. */
#ifndef BBD_ODOM_MATH_H
#define BBD_ODOM_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "bbd_math.h" /* BBD_HD */

#define BBD_ODOM_LANES 256 /* partial sums of the summary: a power of two */

/* Any NaN -> the quiet NaN 0x7ff8000000000000.  Done on the bits: a compiler may fold `v != v ? NaN : v` to v. */
BBD_HD double bbd_odom_canon(double v) {
  uint64_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = (uint64_t)__double_as_longlong(v);
#else
  memcpy(&b, &v, 8);
#endif
  if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)b);
#else
  memcpy(&v, &b, 8);
  return v;
#endif
}

/* r = a @ b, float32, the rounding order of mul4 in bbd_pose.hip; r may not alias a or b */
BBD_HD void bbd_odom_mul4f(const float* a, const float* b, float* r) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      float acc = a[i * 4 + 0] * b[j];
      acc = acc + a[i * 4 + 1] * b[4 + j];
      acc = acc + a[i * 4 + 2] * b[8 + j];
      acc = acc + a[i * 4 + 3] * b[12 + j];
      r[i * 4 + j] = acc;
    }
}

/* poses [1+S, N, 16]: the chained pose of window i from its S single steps (sections 1 .. S) */
BBD_HD void bbd_odom_chain(const float* poses, int N, int S, int i, float* out) {
  float t[16], u[16];
  const float* last = poses + ((size_t)S * N + i) * 16;
  for (int e = 0; e < 16; ++e) t[e] = last[e];
  for (int k = S - 2; k >= 0; --k) {
    bbd_odom_mul4f(t, poses + ((size_t)(1 + k) * N + i) * 16, u);
    for (int e = 0; e < 16; ++e) t[e] = u[e];
  }
  for (int e = 0; e < 16; ++e) out[e] = t[e];
}

/* r = a @ b, float64, np.dot's result up to the summation order; r may not alias a or b */
BBD_HD void bbd_odom_mul4d(const double* a, const double* b, double* r) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = a[i * 4 + 0] * b[j];
      acc = acc + a[i * 4 + 1] * b[4 + j];
      acc = acc + a[i * 4 + 2] * b[8 + j];
      acc = acc + a[i * 4 + 3] * b[12 + j];
      r[i * 4 + j] = acc;
    }
}

/* General 4x4 inverse: Gauss-Jordan on [a | I], the pivot of a column is its largest remaining |entry| (the first of
 * equals).  A singular matrix gives inf / NaN entries (np.linalg.inv raises). */
BBD_HD void bbd_odom_inv4(const double* a, double* r) {
  double m[4][8];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      m[i][j] = a[i * 4 + j];
      m[i][4 + j] = (i == j) ? 1.0 : 0.0;
    }
  for (int col = 0; col < 4; ++col) {
    int p = col;
    double best = fabs(m[col][col]);
    for (int row = col + 1; row < 4; ++row) {
      const double v = fabs(m[row][col]);
      if (v > best) {
        best = v;
        p = row;
      }
    }
    for (int row = col + 1; row < 4; ++row)
      if (row == p)
        for (int j = 0; j < 8; ++j) {
          const double t = m[col][j];
          m[col][j] = m[row][j];
          m[row][j] = t;
        }
    const double pivot = m[col][col];
    for (int j = 0; j < 8; ++j) m[col][j] = m[col][j] / pivot;
    for (int row = 0; row < 4; ++row) {
      if (row == col) continue;
      const double f = m[row][col];
      for (int j = 0; j < 8; ++j) m[row][j] = m[row][j] - f * m[col][j];
    }
  }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) r[i * 4 + j] = m[i][4 + j];
}

/* gt [M, 12]: the local ground-truth pose of frames (j, j + S) */
BBD_HD void bbd_odom_gt_local(const double* gt, int j, int S, double* out) {
  double a[16], b[16], ia[16], prod[16];
  const double* ga = gt + (size_t)j * 12;
  const double* gb = gt + (size_t)(j + S) * 12;
  for (int e = 0; e < 12; ++e) {
    a[e] = ga[e];
    b[e] = gb[e];
  }
  for (int e = 12; e < 16; ++e) a[e] = b[e] = (e == 15) ? 1.0 : 0.0;
  bbd_odom_inv4(a, ia);
  bbd_odom_mul4d(ia, b, prod);
  bbd_odom_inv4(prod, out);
}

BBD_HD void bbd_odom_eye(double* m) {
  for (int e = 0; e < 16; ++e) m[e] = (e % 5 == 0) ? 1.0 : 0.0;
}

/* One pass over a track of n poses (pred float32 [n,16], gt_local float64 [n,16], both starting at the track's first
 * window).  pass 0: *a = sum(gt * pred), *b = sum(pred^2); pass 1: *a = sum((pred * scale - gt)^2).  The sums run over
 * the flat [n+1, 3] arrays in order; their first row is xyz_0 = 0 on both sides and adds exact zeros. */
BBD_HD void bbd_odom_track_pass(const float* pred, const double* gt_local, int n, int pass, double scale, double* a,
                                double* b) {
  double P[16], G[16], T[16], next[16];
  bbd_odom_eye(P);
  bbd_odom_eye(G);
  const double off = 0.0 - 0.0; /* gt_xyz[0] - pred_xyz[0], every coordinate */
  double s0 = 0.0, s1 = 0.0;
  for (int k = 0; k < n; ++k) {
    for (int e = 0; e < 16; ++e) T[e] = (double)pred[(size_t)k * 16 + e];
    bbd_odom_mul4d(P, T, next);
    for (int e = 0; e < 16; ++e) P[e] = next[e];
    bbd_odom_mul4d(G, gt_local + (size_t)k * 16, next);
    for (int e = 0; e < 16; ++e) G[e] = next[e];
    for (int c = 0; c < 3; ++c) {
      const double p = P[c * 4 + 3] + off, g = G[c * 4 + 3];
      if (pass == 0) {
        s0 = s0 + g * p;
        s1 = s1 + p * p;
      } else {
        const double err = p * scale - g;
        s0 = s0 + err * err;
      }
    }
  }
  *a = s0;
  *b = s1;
}

BBD_HD double bbd_odom_ate(const float* pred, const double* gt_local, int n) {
  double sgp, spp, se, unused;
  bbd_odom_track_pass(pred, gt_local, n, 0, 0.0, &sgp, &spp);
  const double scale = sgp / spp;
  bbd_odom_track_pass(pred, gt_local, n, 1, scale, &se, &unused);
  return bbd_odom_canon(sqrt(se) / (double)(n + 1));
}

/* lane t of BBD_ODOM_LANES: x[t] + x[t + LANES] + ...; with `centre` the squares of |x - mean| (np.std) */
BBD_HD double bbd_odom_partial(const double* x, int count, int t, int centre, double mean) {
  double s = 0.0;
  for (int k = t; k < count; k += BBD_ODOM_LANES) {
    double v = x[k];
    if (centre) {
      v = v - mean;
      v = v * v;
    }
    s = s + v;
  }
  return s;
}

#endif
