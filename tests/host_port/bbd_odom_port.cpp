// Host port of bbd_odom.hip for the CPU test tier: the same arithmetic (bbd_odom_math.h) and the same three stages, the
// "threads" run serially; the summary's BBD_ODOM_LANES partial sums and halving tree are those of the device's block.
// Same C signature as bbd_pose_ate minus `stream`.
#include <cmath>
#include <cstddef>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_odom_math.h"

namespace {

double lanes_sum(const double* x, int count, int centre, double mean) {
  double red[BBD_ODOM_LANES];
  for (int t = 0; t < BBD_ODOM_LANES; ++t) red[t] = bbd_odom_partial(x, count, t, centre, mean);
  for (int s = BBD_ODOM_LANES / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] = red[t] + red[t + s];
  return red[0];
}

}  // namespace

extern "C" int hp_pose_ate(const float* poses, const double* gt, float* chained, double* gt_local, double* ates,
                           double* summary, int N, int M, int S, int L) {
  if (S < 1 || L < 1 || N < 0 || M < S || N > M - S || !summary) return BBD_E_BADARG;
  if ((1 + (long)S) * N > 0x7fffffffL / 16 || M > 0x7fffffff / 16) return BBD_E_TOOMANY;
  const int NG = M - S, tracks = N > S ? N - S : 0;
  if ((N > 0 && (!poses || !chained)) || (NG > 0 && (!gt || !gt_local)) || (tracks > 0 && !ates)) return BBD_E_BADARG;
  for (int i = 0; i < N; ++i) bbd_odom_chain(poses, N, S, i, chained + (size_t)i * 16);
  for (int j = 0; j < NG; ++j) bbd_odom_gt_local(gt, j, S, gt_local + (size_t)j * 16);
  for (int t = 0; t < 2 * tracks; ++t) {
    const int row = t / tracks, i = t - row * tracks;
    const int n = L < N - i ? L : N - i;
    ates[t] = bbd_odom_ate((row == 0 ? poses : chained) + (size_t)i * 16, gt_local + (size_t)i * 16, n);
  }
  for (int row = 0; row < 2; ++row) {
    const double* x = ates + (size_t)row * tracks;
    const double mean = lanes_sum(x, tracks, 0, 0.0) / (double)tracks;
    const double var = lanes_sum(x, tracks, 1, mean) / (double)tracks;
    summary[row * 4 + 0] = bbd_odom_canon(mean);
    summary[row * 4 + 1] = bbd_odom_canon(std::sqrt(var));
    summary[row * 4 + 2] = (double)tracks;
    summary[row * 4 + 3] = 0.0;
  }
  return 0;
}
