// Host port of bbd_traj.hip for the CPU test tier: the same arithmetic (bbd_traj_math.h) and the same four stages, the
// lanes run serially; the doubling scan reads every lane's partner before any lane writes, as the device's barrier makes
// it.  Same C signature as bbd_pose_trajectory minus `stream`.
//
// hp_gather_pairs and hp_pose_matrix_fwd are stand-ins, not ports: they let `evaluation.evaluate_pose` run on the CPU
// tier, where the test only needs SOME deterministic pose matrix per frame pair (tests/traj_port.py).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_traj_math.h"

namespace {

constexpr int NT = BBD_TRAJ_LANES;

template <typename Partial>
double tree_sum(Partial partial) {
  double red[NT];
  for (int t = 0; t < NT; ++t) red[t] = partial(t);
  for (int s = NT / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] = red[t] + red[t + s];
  return red[0];
}

}  // namespace

extern "C" int hp_pose_trajectory(const float* steps, const double* gt, const double* lengths, double* traj, double* gt_traj,
                                  double* aligned, double* transform, double* dist, double* pairs, double* per_length,
                                  double* summary, int J, int M, int n_len, int step, int mode) {
  if (!steps || !gt || !traj || !gt_traj || !aligned || !transform || !dist || !pairs || !per_length || !summary)
    return BBD_E_BADARG;
  if (int rc = bbd_traj_check(J, M, lengths, n_len, step, mode)) return rc;
  const int F = J + 1, n_first = (F + step - 1) / step;
  if ((long)n_first * n_len > 0x7fffffffL / 4) return BBD_E_TOOMANY;
  // 1. the matrices
  for (int j = 0; j <= J; ++j) {
    bbd_traj_gt_rel(gt, j, gt_traj + (size_t)j * 16);
    if (j < J) bbd_traj_step_inv(steps, j, traj + (size_t)(j + 1) * 16);
  }
  // 2. the scan ...
  std::vector<double> Q((size_t)NT * 16), next((size_t)NT * 16);
  for (int t = 0; t < NT; ++t) bbd_traj_chunk_product(traj, J, t, &Q[(size_t)t * 16]);
  for (int d = 1; d < NT; d <<= 1) {
    next = Q;
    for (int t = d; t < NT; ++t) bbd_odom_mul4d(&Q[(size_t)(t - d) * 16], &Q[(size_t)t * 16], &next[(size_t)t * 16]);
    Q.swap(next);
  }
  bbd_odom_eye(traj);
  for (int t = 0; t < NT; ++t) {
    double X[16];
    if (t == 0)
      bbd_odom_eye(X);
    else
      for (int e = 0; e < 16; ++e) X[e] = Q[(size_t)(t - 1) * 16 + e];
    bbd_traj_replay(traj, J, t, X);
  }
  // ... the path length ...
  double off[NT], run = 0.0;
  for (int t = 0; t < NT; ++t) {
    off[t] = run;
    run = run + bbd_traj_dist_chunk(gt_traj, dist, J, t, 0, 0.0);
  }
  dist[0] = 0.0;
  for (int t = 0; t < NT; ++t) bbd_traj_dist_chunk(gt_traj, dist, J, t, 1, off[t]);
  // ... the moments and the alignment ...
  double m[20];
  for (int e = 0; e < 20; ++e) m[e] = 0.0;
  auto moment = [&](const double* P, int what) {
    return tree_sum([&](int t) { return bbd_traj_partial(P, gt_traj, F, t, what, m); });
  };
  if (mode == BBD_TRAJ_MODE_SIM3 || mode == BBD_TRAJ_MODE_SE3) {
    for (int w = 0; w < BBD_TRAJ_T_GP; ++w) m[w] = moment(traj, w) / (double)F;
  } else if (mode == BBD_TRAJ_MODE_SCALE) {
    m[BBD_TRAJ_T_GP] = moment(traj, BBD_TRAJ_T_GP);
    m[BBD_TRAJ_T_PP] = moment(traj, BBD_TRAJ_T_PP);
  }
  bbd_traj_align_t al;
  bbd_traj_align(m, mode, &al);
  for (int r = 0; r < 3; ++r) {
    for (int s = 0; s < 3; ++s) transform[4 * r + s] = al.R[3 * r + s];
    transform[4 * r + 3] = al.t[r];
  }
  transform[12] = transform[13] = transform[14] = 0.0;
  transform[15] = 1.0;
  // ... the aligned poses and the ATE figures
  for (int j = 0; j < F; ++j) bbd_traj_apply(&al, traj + (size_t)j * 16, aligned + (size_t)j * 16);
  const double sq = moment(aligned, BBD_TRAJ_T_ESQ), se = moment(aligned, BBD_TRAJ_T_E);
  double mx = 0.0;
  for (int t = 0; t < NT; ++t) {
    const double v = bbd_traj_partial_max(aligned, gt_traj, F, t);
    mx = v > mx ? v : mx;
  }
  summary[3] = bbd_odom_canon(std::sqrt(sq / (double)F));
  summary[4] = bbd_odom_canon(se / (double)F);
  summary[5] = bbd_odom_canon(sq != sq ? sq : mx);
  summary[6] = al.c;
  summary[7] = (double)F;
  // 3. the pairs
  for (int k = 0; k < n_first * n_len; ++k)
    bbd_traj_pair(gt_traj, aligned, dist, F, (k / n_len) * step, lengths[k % n_len], pairs + (size_t)k * 4);
  // 4. the means
  for (int l = -1; l < n_len; ++l) {
    const double* base = l < 0 ? pairs : pairs + (size_t)l * 4;
    const int count = l < 0 ? n_first * n_len : n_first, stride = l < 0 ? 1 : n_len;
    auto column = [&](int col) {
      return tree_sum([&](int t) {
        double s3[3];
        bbd_traj_pair_partials(base, count, stride, t, s3);
        return s3[col];
      });
    };
    const double n = column(0), te = column(1), re = column(2);
    double* o = l < 0 ? summary : per_length + (size_t)l * 3;
    o[0] = bbd_odom_canon(te / n);
    o[1] = bbd_odom_canon(re / n);
    o[2] = n;
  }
  return 0;
}

// ---- stand-ins for the two launches between the frame pool and the pose buffer
extern "C" int hp_gather_pairs(const float* pool, const int32_t* idx_a, const int32_t* idx_b, float* out, int R, long chw,
                               double sub, double mul) {
  for (int r = 0; r < R; ++r)
    for (int half = 0; half < 2; ++half) {
      const float* src = pool + (size_t)(half ? idx_b[r] : idx_a[r]) * chw;
      float* dst = out + ((size_t)2 * r + half) * chw;
      for (long i = 0; i < chw; ++i) dst[i] = (src[i] - (float)sub) * (float)mul;
    }
  return 0;
}

extern "C" int hp_pose_matrix_fwd(const float* aa, const float* tr, float* M, int n, int invert, const int32_t* invert_rows) {
  if (invert || invert_rows) return BBD_E_BADARG;
  for (int i = 0; i < n; ++i) {  // Rodrigues' formula in float64, rounded once: any fixed function of the row will do
    const double x = aa[3 * i], y = aa[3 * i + 1], z = aa[3 * i + 2];
    const double th = std::sqrt(x * x + y * y + z * z), k = th > 0.0 ? 1.0 / th : 0.0;
    const double a[3] = {x * k, y * k, z * k}, c = std::cos(th), s = std::sin(th), C = 1.0 - c;
    const double R[9] = {a[0] * a[0] * C + c,        a[0] * a[1] * C - a[2] * s, a[0] * a[2] * C + a[1] * s,
                         a[0] * a[1] * C + a[2] * s, a[1] * a[1] * C + c,        a[1] * a[2] * C - a[0] * s,
                         a[0] * a[2] * C - a[1] * s, a[1] * a[2] * C + a[0] * s, a[2] * a[2] * C + c};
    float* m = M + (size_t)i * 16;
    for (int r = 0; r < 3; ++r) {
      for (int q = 0; q < 3; ++q) m[4 * r + q] = (float)R[3 * r + q];
      m[4 * r + 3] = tr[3 * i + r];
    }
    m[12] = m[13] = m[14] = 0.0f;
    m[15] = 1.0f;
  }
  return 0;
}
