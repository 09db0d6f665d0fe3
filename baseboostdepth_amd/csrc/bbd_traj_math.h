/* bbd_traj_math.h - arithmetic of the full-trajectory KITTI odometry scores (bbd_traj.hip): the predicted trajectory
 * chained from the pose network's single steps, its alignment to ground truth, the absolute trajectory error of the
 * aligned trajectory and the devkit's sub-sequence errors t_rel / r_rel (calcSequenceErrors).  Shared with the host port
 * of the test tier (tests/host_port/bbd_traj_port.cpp).  DESIGN.md 6d has the definitions; this header fixes the ORDER
 * of every sum and product, so that the device, the host port and a second call give the same bytes.
 *
 *   trajectory  C_0 = I, C_{j+1} = C_j . inv(double(steps[j])), general inverse (bbd_odom_inv4), products left to right.
 *               This is a true camera-to-first-frame trajectory.  The reference's dump_xyz is NOT used: it multiplies
 *               the steps themselves left to right, T_0 T_1 .., and the inverse of a product reverses the order, so it
 *               telescopes over one step only (its snippets are 1..5 poses long; a sequence is not).
 *               Blocked scan over BBD_TRAJ_LANES = 256 lanes, lane t owning the steps [t k, min(t k + k, J)),
 *               k = ceil(J / 256):  (1) Q_t = I . inv_a . inv_{a+1} ... of its chunk, left to right (I for an empty
 *               chunk);  (2) inclusive scan of the Q_t by doubling: for d = 1, 2, 4 .. 128, all lanes at once,
 *               Q_t <- Q_{t-d} . Q_t for t >= d;  (3) replay: X = Q_{t-1} (I for lane 0), then X <- X . inv_j, C_{j+1} = X
 *               along the chunk.  Every product is bbd_odom_mul4d.
 *   gt          G^_j = inv(G_0) . G_j, G = the file row over (0 0 0 1); g_j = G^_j[:3,3]
 *   dist        s_j = |g_j - g_{j-1}| = sqrt((dx dx + dy dy) + dz dz), j = 1 .. J, in the same chunks (segment j belongs
 *               to step j - 1): local_j = the running sum of the chunk's segments from 0.0, total_t its last value,
 *               off_0 = 0, off_{t+1} = off_t + total_t (sequential), dist_j = off_t + local_j; dist_0 = 0.  Rounding is
 *               monotone, so dist is non-decreasing whatever the chunking and the binary search below is valid.
 *   means       every mean / moment over the F = J + 1 frames: lane t of 256 adds its terms j = t, t + 256, .. in order
 *               (the pattern of bbd_odom_partial), the 256 partial sums go through the halving tree
 *               (s = 128, 64 .. 1: x_t += x_{t+s}), the total is divided by the count
 *   alignment   of p_j = C_j[:3,3] to g_j, giving (c, R, t):
 *                 sim3   Umeyama: mu_p, mu_g; sigma_p^2 = mean |p - mu_p|^2; Sigma = mean (g - mu_g)(p - mu_p)^T (each
 *                        term one product of two differences); Sigma = U D V^T by bbd_traj_svd3; R = U S V^T with
 *                        S = diag(1, 1, +-1), -1 when det U det V < 0; c = ((d0 + d1) + S33 d2) / sigma_p^2;
 *                        t = mu_g - c (R mu_p)
 *                 se3    the same with c = 1
 *                 scale  R = I, t = 0, c = sum g.p / sum p.p (terms (gx px + gy py) + gz pz per frame): the reference's
 *                        compute_ate scale over the whole sequence
 *                 none   c = 1, R = I, t = 0
 *               Sigma exactly zero gives R = I.  sigma_p^2 = 0 or sum p.p = 0 makes c = 0 / 0 = NaN, and with it t, the
 *               aligned translations, the ATE figures and every sub-sequence error (the general inverse spreads a NaN
 *               translation over the whole error matrix, so r_err is NaN too).
 *   svd3        one-sided Jacobi (Hestenes) in float64, one lane: W = Sigma, V = I; a sweep visits the column pairs
 *               (0,1), (0,2), (1,2) in that order; a pair with |w_p.w_q| > 2^-52 sqrt((w_p.w_p)(w_q.w_q)) is rotated
 *               (zeta = (beta - alpha) / (2 gamma), tan = sign(zeta) / (|zeta| + sqrt(1 + zeta^2))), W and V alike.
 *               Stop after the first sweep that rotates nothing, or after BBD_TRAJ_SWEEPS = 30 sweeps.  d_i = |w_i|,
 *               sorted descending by the exchanges (0,1), (0,2), (1,2) (columns of W and V go along).  u0 = w0 / d0;
 *               u1 = w1 / d1, or for d1 = 0 the unit vector e_k - u0[k] u0 normalised, k the first smallest |u0[k]|;
 *               the third column of U S is sign(det V) (u0 x u1) - the same matrix as the textbook's for rank >= 2,
 *               and defined for every rank; S33 = sign(w2 . (u0 x u1)) sign(det V), a zero counting as positive.
 *   aligned     C'_j = [R R_j | c (R p_j) + t] over (0 0 0 1), three-term sums left to right;
 *               e_j = |p'_j - g_j|; ate_rmse = sqrt(mean e^2), ate_mean = mean e, ate_max = max e (NaN if any e is)
 *   pairs       first = 0, step, 2 step .. < F, every length L: last = the first i >= first with dist_i > dist_first + L
 *               (binary search on [first, F)); none: the pair is skipped (last = -1, errors NaN).  Else
 *               dG = inv(G^_first) G^_last, dP = inv(C'_first) C'_last, E = inv(dP) dG, t_err = |E[:3,3]| / L,
 *               r_err = acos(clamp(0.5 (((E00 + E11) + E22) - 1), -1, 1)) / L.
 *               dP is [R_f^T R_l | c R_f^T (p_l - p_f)]: the relative poses depend on the alignment ONLY through c.
 *   summary     t_rel, r_rel = the means of t_err, r_err over the valid pairs in flat (first, length) order, per length
 *               over that length's firsts; no valid pair gives 0 / 0 = NaN
 *
 * Every product is rounded on its own (compile with -ffp-contract=off).  A NaN is written as 0x7ff8000000000000
 * (bbd_odom_canon).  acos is the one call whose result may differ between the device's and the host's libm. */
#ifndef BBD_TRAJ_MATH_H
#define BBD_TRAJ_MATH_H

#include "bbd_odom_math.h"

#define BBD_TRAJ_LANES 256 /* the scan's lanes and the means' partial sums: a power of two, = BBD_ODOM_LANES */
#define BBD_TRAJ_SWEEPS 30
#define BBD_TRAJ_MAX_LENGTHS 8

#define BBD_TRAJ_MODE_SIM3 0
#define BBD_TRAJ_MODE_SE3 1
#define BBD_TRAJ_MODE_SCALE 2
#define BBD_TRAJ_MODE_NONE 3

typedef struct {
  double v[BBD_TRAJ_MAX_LENGTHS];
} bbd_traj_lengths_t;

typedef struct {
  double c, R[9], t[3];
} bbd_traj_align_t;

BBD_HD int bbd_traj_chunk(int J) { return (J + BBD_TRAJ_LANES - 1) / BBD_TRAJ_LANES; }

/* the argument checks of bbd_pose_trajectory that need no device: 0 or a BBD_E_* code (-1 BADARG, -2 TOOMANY) */
BBD_HD int bbd_traj_check(int J, int M, const double* lengths, int n_len, int step, int mode) {
  if (J < 1 || M < 1 || M - 1 < J || n_len < 1 || n_len > BBD_TRAJ_MAX_LENGTHS || step < 1 || !lengths) return -1;
  if (mode < BBD_TRAJ_MODE_SIM3 || mode > BBD_TRAJ_MODE_NONE) return -1;
  for (int l = 0; l < n_len; ++l) {
    if (!(lengths[l] > 0.0) || lengths[l] > 1.7976931348623157e308) return -1;
    if (l > 0 && !(lengths[l] > lengths[l - 1])) return -1;
  }
  if (M > 0x7fffffff / 16) return -2;
  return 0;
}

/* row j of the poses file over (0 0 0 1) */
BBD_HD void bbd_traj_gt4(const double* gt, int j, double* G) {
  for (int e = 0; e < 12; ++e) G[e] = gt[(size_t)j * 12 + e];
  G[12] = 0.0;
  G[13] = 0.0;
  G[14] = 0.0;
  G[15] = 1.0;
}

/* G^_j = inv(G_0) . G_j */
BBD_HD void bbd_traj_gt_rel(const double* gt, int j, double* out) {
  double G0[16], Gj[16], inv0[16];
  bbd_traj_gt4(gt, 0, G0);
  bbd_traj_gt4(gt, j, Gj);
  bbd_odom_inv4(G0, inv0);
  bbd_odom_mul4d(inv0, Gj, out);
}

/* inv(double(steps[j])) */
BBD_HD void bbd_traj_step_inv(const float* steps, int j, double* out) {
  double T[16];
  for (int e = 0; e < 16; ++e) T[e] = (double)steps[(size_t)j * 16 + e];
  bbd_odom_inv4(T, out);
}

/* x <- x . m */
BBD_HD void bbd_traj_mul_into(double* x, const double* m) {
  double r[16];
  bbd_odom_mul4d(x, m, r);
  for (int e = 0; e < 16; ++e) x[e] = r[e];
}

/* Stage (1) of the scan, lane t: Q_t from the inverses, which lie in rows 1 .. J of traj [F,16] (row j + 1 = inv_j). */
BBD_HD void bbd_traj_chunk_product(const double* traj, int J, int t, double* Q) {
  const int k = bbd_traj_chunk(J), a = t * k;
  const int b = a + k < J ? a + k : J;
  bbd_odom_eye(Q);
  for (int j = a; j < b; ++j) bbd_traj_mul_into(Q, traj + (size_t)(j + 1) * 16);
}

/* Stage (3), lane t: X = the product of every earlier chunk on entry; rows a + 1 .. b of traj turn from inv_j into C_{j+1} */
BBD_HD void bbd_traj_replay(double* traj, int J, int t, double* X) {
  const int k = bbd_traj_chunk(J), a = t * k;
  const int b = a + k < J ? a + k : J;
  for (int j = a; j < b; ++j) {
    double* row = traj + (size_t)(j + 1) * 16;
    bbd_traj_mul_into(X, row);
    for (int e = 0; e < 16; ++e) row[e] = X[e];
  }
}

/* s_j, j >= 1, from gt_traj [F,16] */
BBD_HD double bbd_traj_segment(const double* gt_traj, int j) {
  const double* a = gt_traj + (size_t)(j - 1) * 16;
  const double* b = a + 16;
  const double dx = b[3] - a[3], dy = b[7] - a[7], dz = b[11] - a[11];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

/* lane t: total_t (write = 0, off unused) or dist_j = off + local_j along the chunk (write = 1); returns total_t */
BBD_HD double bbd_traj_dist_chunk(const double* gt_traj, double* dist, int J, int t, int write, double off) {
  const int k = bbd_traj_chunk(J), a = t * k;
  const int b = a + k < J ? a + k : J;
  double local = 0.0;
  for (int j = a; j < b; ++j) {
    local = local + bbd_traj_segment(gt_traj, j + 1);
    if (write) dist[j + 1] = off + local;
  }
  return local;
}

/* The terms of the means.  `what` selects the term of frame j; mu = (mu_p, mu_g) where it is needed. */
#define BBD_TRAJ_T_P 0      /* + axis: p_j[axis] */
#define BBD_TRAJ_T_G 3      /* + axis: g_j[axis] */
#define BBD_TRAJ_T_VAR 6    /* |p_j - mu_p|^2 */
#define BBD_TRAJ_T_SIGMA 7  /* + 3 r + s: (g_j - mu_g)[r] (p_j - mu_p)[s] */
#define BBD_TRAJ_T_GP 16    /* g_j . p_j */
#define BBD_TRAJ_T_PP 17    /* p_j . p_j */
#define BBD_TRAJ_T_ESQ 18   /* e_j^2 (p = the aligned trajectory) */
#define BBD_TRAJ_T_E 19     /* e_j */

BBD_HD double bbd_traj_term(const double* p, const double* g, int what, const double* mu) {
  if (what < BBD_TRAJ_T_G) return p[4 * what + 3];
  if (what < BBD_TRAJ_T_VAR) return g[4 * (what - BBD_TRAJ_T_G) + 3];
  if (what == BBD_TRAJ_T_VAR) {
    const double dx = p[3] - mu[0], dy = p[7] - mu[1], dz = p[11] - mu[2];
    return (dx * dx + dy * dy) + dz * dz;
  }
  if (what < BBD_TRAJ_T_GP) {
    const int r = (what - BBD_TRAJ_T_SIGMA) / 3, s = (what - BBD_TRAJ_T_SIGMA) % 3;
    return (g[4 * r + 3] - mu[3 + r]) * (p[4 * s + 3] - mu[s]);
  }
  if (what == BBD_TRAJ_T_GP) return (g[3] * p[3] + g[7] * p[7]) + g[11] * p[11];
  if (what == BBD_TRAJ_T_PP) return (p[3] * p[3] + p[7] * p[7]) + p[11] * p[11];
  const double dx = p[3] - g[3], dy = p[7] - g[7], dz = p[11] - g[11];
  const double sq = (dx * dx + dy * dy) + dz * dz;
  return what == BBD_TRAJ_T_ESQ ? sq : sqrt(sq);
}

/* lane t of BBD_TRAJ_LANES: the terms of frames t, t + 256, .. added in order */
BBD_HD double bbd_traj_partial(const double* P, const double* G, int F, int t, int what, const double* mu) {
  double s = 0.0;
  for (int j = t; j < F; j += BBD_TRAJ_LANES) s = s + bbd_traj_term(P + (size_t)j * 16, G + (size_t)j * 16, what, mu);
  return s;
}

/* The same for the n <= 10 consecutive terms first, first + 1, ..: one pass over the frames, every sum in the order of
 * bbd_traj_partial (the device takes the moments in three such passes instead of eighteen) */
BBD_HD void bbd_traj_partials(const double* P, const double* G, int F, int t, int first, int n, const double* mu,
                              double* s) {
  for (int i = 0; i < n; ++i) s[i] = 0.0;
  for (int j = t; j < F; j += BBD_TRAJ_LANES)
    for (int i = 0; i < n; ++i) s[i] = s[i] + bbd_traj_term(P + (size_t)j * 16, G + (size_t)j * 16, first + i, mu);
}

/* lane t: the largest e_j of its frames (0 for none); NaNs are not seen here, the caller takes them from the sum */
BBD_HD double bbd_traj_partial_max(const double* P, const double* G, int F, int t) {
  double m = 0.0;
  for (int j = t; j < F; j += BBD_TRAJ_LANES) {
    const double e = bbd_traj_term(P + (size_t)j * 16, G + (size_t)j * 16, BBD_TRAJ_T_E, 0);
    m = e > m ? e : m;
  }
  return m;
}

/* One Jacobi rotation of the columns (p, q) of W and V (3x3, row-major); returns 1 if it rotated. */
BBD_HD int bbd_traj_jacobi_pair(double* W, double* V, int p, int q) {
  const double alpha = (W[p] * W[p] + W[3 + p] * W[3 + p]) + W[6 + p] * W[6 + p];
  const double beta = (W[q] * W[q] + W[3 + q] * W[3 + q]) + W[6 + q] * W[6 + q];
  const double gamma = (W[p] * W[q] + W[3 + p] * W[3 + q]) + W[6 + p] * W[6 + q];
  if (!(fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha * beta))) return 0;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double tn = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
  for (int r = 0; r < 3; ++r) {
    const double wp = W[3 * r + p], wq = W[3 * r + q];
    W[3 * r + p] = cs * wp - sn * wq;
    W[3 * r + q] = sn * wp + cs * wq;
    const double vp = V[3 * r + p], vq = V[3 * r + q];
    V[3 * r + p] = cs * vp - sn * vq;
    V[3 * r + q] = sn * vp + cs * vq;
  }
  return 1;
}

BBD_HD void bbd_traj_swap_cols(double* W, double* V, double* d, int p, int q) {
  if (!(d[p] < d[q])) return;
  double x = d[p];
  d[p] = d[q];
  d[q] = x;
  for (int r = 0; r < 3; ++r) {
    x = W[3 * r + p];
    W[3 * r + p] = W[3 * r + q];
    W[3 * r + q] = x;
    x = V[3 * r + p];
    V[3 * r + p] = V[3 * r + q];
    V[3 * r + q] = x;
  }
}

/* Sigma (row-major 3x3) -> R = U S V^T and tr(D S).  Sigma exactly zero: R = I, trace 0. */
BBD_HD void bbd_traj_svd3(const double* Sigma, double* R, double* trace) {
  double W[9], V[9], d[3];
  for (int e = 0; e < 9; ++e) {
    W[e] = Sigma[e];
    V[e] = (e % 4 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < BBD_TRAJ_SWEEPS; ++sweep) {
    int rotated = bbd_traj_jacobi_pair(W, V, 0, 1);
    rotated += bbd_traj_jacobi_pair(W, V, 0, 2);
    rotated += bbd_traj_jacobi_pair(W, V, 1, 2);
    if (!rotated) break;
  }
  for (int i = 0; i < 3; ++i) d[i] = sqrt((W[i] * W[i] + W[3 + i] * W[3 + i]) + W[6 + i] * W[6 + i]);
  bbd_traj_swap_cols(W, V, d, 0, 1);
  bbd_traj_swap_cols(W, V, d, 0, 2);
  bbd_traj_swap_cols(W, V, d, 1, 2);
  if (!(d[0] > 0.0)) { /* Sigma = 0 (or NaN): no rotation can be told from another */
    for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
    *trace = d[0]; /* 0, or NaN for a NaN Sigma */
    return;
  }
  double u0[3], u1[3], u2[3];
  for (int r = 0; r < 3; ++r) u0[r] = W[3 * r] / d[0];
  if (d[1] > 0.0) {
    for (int r = 0; r < 3; ++r) u1[r] = W[3 * r + 1] / d[1];
  } else {
    int k = 0;
    if (fabs(u0[1]) < fabs(u0[k])) k = 1;
    if (fabs(u0[2]) < fabs(u0[k])) k = 2;
    const double uk = k == 0 ? u0[0] : (k == 1 ? u0[1] : u0[2]);
    for (int r = 0; r < 3; ++r) u1[r] = (r == k ? 1.0 : 0.0) - uk * u0[r];
    const double n = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    for (int r = 0; r < 3; ++r) u1[r] = u1[r] / n;
  }
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
  u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
  u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  const double detV = (V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6])) +
                      V[2] * (V[3] * V[7] - V[4] * V[6]);
  const double sV = detV < 0.0 ? -1.0 : 1.0;
  const double w2u2 = (W[2] * u2[0] + W[5] * u2[1]) + W[8] * u2[2];
  const double s33 = (w2u2 < 0.0 ? -1.0 : 1.0) * sV;
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) R[3 * r + s] = (u0[r] * V[3 * s] + u1[r] * V[3 * s + 1]) + (sV * u2[r]) * V[3 * s + 2];
  *trace = (d[0] + d[1]) + s33 * d[2];
}

/* m [20] = the means of the terms 0 .. 17 that the mode needs (others unread): mu_p, mu_g, sigma_p^2, Sigma | sums
 * g.p, p.p (NOT divided) */
BBD_HD void bbd_traj_align(const double* m, int mode, bbd_traj_align_t* out) {
  for (int e = 0; e < 9; ++e) out->R[e] = (e % 4 == 0) ? 1.0 : 0.0;
  out->t[0] = out->t[1] = out->t[2] = 0.0;
  out->c = 1.0;
  if (mode == BBD_TRAJ_MODE_SCALE) out->c = bbd_odom_canon(m[BBD_TRAJ_T_GP] / m[BBD_TRAJ_T_PP]);
  if (mode == BBD_TRAJ_MODE_SIM3 || mode == BBD_TRAJ_MODE_SE3) {
    double trace;
    bbd_traj_svd3(m + BBD_TRAJ_T_SIGMA, out->R, &trace);
    if (mode == BBD_TRAJ_MODE_SIM3) out->c = bbd_odom_canon(trace / m[BBD_TRAJ_T_VAR]);
    for (int r = 0; r < 3; ++r) {
      const double Rmu = (out->R[3 * r] * m[0] + out->R[3 * r + 1] * m[1]) + out->R[3 * r + 2] * m[2];
      out->t[r] = bbd_odom_canon(m[BBD_TRAJ_T_G + r] - out->c * Rmu);
    }
  }
}

/* C'_j from C_j (both 16 doubles; may not alias) */
BBD_HD void bbd_traj_apply(const bbd_traj_align_t* al, const double* C, double* out) {
  for (int r = 0; r < 3; ++r) {
    for (int s = 0; s < 3; ++s)
      out[4 * r + s] = (al->R[3 * r] * C[s] + al->R[3 * r + 1] * C[4 + s]) + al->R[3 * r + 2] * C[8 + s];
    const double Rp = (al->R[3 * r] * C[3] + al->R[3 * r + 1] * C[7]) + al->R[3 * r + 2] * C[11];
    out[4 * r + 3] = bbd_odom_canon(al->c * Rp + al->t[r]);
  }
  out[12] = 0.0;
  out[13] = 0.0;
  out[14] = 0.0;
  out[15] = 1.0;
}

/* One (first, L) pair: out[4] = (last or -1, t_err, r_err, 0) */
BBD_HD void bbd_traj_pair(const double* gt_traj, const double* aligned, const double* dist, int F, int first, double L,
                          double* out) {
  const double target = dist[first] + L;
  int lo = first, hi = F;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (dist[mid] > target)
      hi = mid;
    else
      lo = mid + 1;
  }
  out[3] = 0.0;
  if (lo >= F) {
    out[0] = -1.0;
    out[1] = out[2] = bbd_odom_canon(0.0 / (double)(F - lo)); /* 0 / 0 */
    return;
  }
  double inv[16], dG[16], dP[16], E[16];
  bbd_odom_inv4(gt_traj + (size_t)first * 16, inv);
  bbd_odom_mul4d(inv, gt_traj + (size_t)lo * 16, dG);
  bbd_odom_inv4(aligned + (size_t)first * 16, inv);
  bbd_odom_mul4d(inv, aligned + (size_t)lo * 16, dP);
  bbd_odom_inv4(dP, inv);
  bbd_odom_mul4d(inv, dG, E);
  double cosv = 0.5 * (((E[0] + E[5]) + E[10]) - 1.0);
  cosv = cosv < -1.0 ? -1.0 : (cosv > 1.0 ? 1.0 : cosv);
  out[0] = (double)lo;
  out[1] = bbd_odom_canon(sqrt((E[3] * E[3] + E[7] * E[7]) + E[11] * E[11]) / L);
  out[2] = bbd_odom_canon(acos(cosv) / L);
}

/* lane t: s[0 .. 2] = the count, the sum of t_err and the sum of r_err of the valid pairs k = t, t + 256, .. < count of
 * pairs [.., 4], taken with `stride` rows between them (1: all pairs flat; n_len: one length's firsts) */
BBD_HD void bbd_traj_pair_partials(const double* pairs, int count, int stride, int t, double* s) {
  s[0] = s[1] = s[2] = 0.0;
  for (int k = t; k < count; k += BBD_TRAJ_LANES) {
    const double* row = pairs + (size_t)k * stride * 4;
    if (row[0] >= 0.0) {
      s[0] = s[0] + 1.0;
      s[1] = s[1] + row[1];
      s[2] = s[2] + row[2];
    }
  }
}

#endif
