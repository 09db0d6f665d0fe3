// bbd_odom.hip - KITTI odometry evaluation (evaluate_pose.py) on the device: chained poses, local ground-truth poses,
// the absolute trajectory error of every track and its mean / std, from the pose network's matrices as they lie in HBM.
//
// The reference copies every predicted pose to the host, builds the ground truth with numpy and scores ~1.6 k windows in
// a Python loop.  Here bbd_pose_ate enqueues three small launches and reads nothing back:
//   1. a thread per matrix: chained[i] for i < N, gt_local[j] for j < M - S (independent 4x4 chains: latency, not work)
//   2. a thread per (row, track): the two passes of compute_ate over min(L, N - i) poses, float64
//   3. a block per row of ATEs: BBD_ODOM_LANES strided partial sums and a halving tree in LDS, twice (mean, then the
//      squared deviations): a fixed order, no atomics, so identical calls give identical bytes
// The arithmetic is bbd_odom_math.h, which the host port of the test tier compiles too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_odom_math.h"

namespace {

constexpr int NT = 256;
static_assert(NT == BBD_ODOM_LANES, "the summary's tree is sized by the block");

__global__ __launch_bounds__(NT) void odom_matrices_kernel(const float* __restrict__ poses, const double* __restrict__ gt,
                                                           float* __restrict__ chained, double* __restrict__ gt_local,
                                                           int N, int NG, int S) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t < N) {
    float m[16];
    bbd_odom_chain(poses, N, S, t, m);
#pragma unroll
    for (int e = 0; e < 16; ++e) chained[(size_t)t * 16 + e] = m[e];
  } else if (t - N < NG) {
    const int j = t - N;
    double m[16];
    bbd_odom_gt_local(gt, j, S, m);
#pragma unroll
    for (int e = 0; e < 16; ++e) gt_local[(size_t)j * 16 + e] = m[e];
  }
}

// tracks = N - S > 0; row 0 scores the direct poses (section 0 of `poses`), row 1 the chained ones
__global__ __launch_bounds__(NT) void odom_tracks_kernel(const float* __restrict__ poses, const float* __restrict__ chained,
                                                         const double* __restrict__ gt_local, double* __restrict__ ates,
                                                         int N, int tracks, int L) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t >= 2 * tracks) return;
  const int row = t / tracks, i = t - row * tracks;
  const int n = min(L, N - i);
  const float* pred = (row == 0 ? poses : chained) + (size_t)i * 16;
  ates[t] = bbd_odom_ate(pred, gt_local + (size_t)i * 16, n);
}

__device__ __forceinline__ double block_sum(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = red[t] + red[t + s];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(NT) void odom_summary_kernel(const double* __restrict__ ates, double* __restrict__ summary,
                                                          int tracks) {
  __shared__ double red[NT];
  const int row = blockIdx.x, t = threadIdx.x;
  const double* x = ates + (size_t)row * tracks;
  const double mean = block_sum(red, bbd_odom_partial(x, tracks, t, 0, 0.0)) / (double)tracks;
  const double var = block_sum(red, bbd_odom_partial(x, tracks, t, 1, mean)) / (double)tracks;
  if (t == 0) {
    summary[row * 4 + 0] = bbd_odom_canon(mean);
    summary[row * 4 + 1] = bbd_odom_canon(sqrt(var));
    summary[row * 4 + 2] = (double)tracks;
    summary[row * 4 + 3] = 0.0;
  }
}

}  // namespace

extern "C" int bbd_pose_ate(const float* poses, const double* gt, float* chained, double* gt_local, double* ates,
                            double* summary, int N, int M, int S, int L, void* stream) {
  if (S < 1 || L < 1 || N < 0 || M < S || N > M - S || !summary) return BBD_E_BADARG;
  if ((1 + (long)S) * N > 0x7fffffffL / 16 || M > 0x7fffffff / 16) return BBD_E_TOOMANY;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int NG = M - S, tracks = N > S ? N - S : 0;
  // an output without elements (no window, no track) may be a null pointer
  if ((N > 0 && (!poses || !chained)) || (NG > 0 && (!gt || !gt_local)) || (tracks > 0 && !ates)) return BBD_E_BADARG;
  if (N + NG > 0) {
    hipLaunchKernelGGL(odom_matrices_kernel, dim3((unsigned)((N + NG + NT - 1) / NT)), dim3(NT), 0, st, poses, gt, chained,
                       gt_local, N, NG, S);
    if (int rc = launch_status()) return rc;
  }
  if (tracks > 0) {
    hipLaunchKernelGGL(odom_tracks_kernel, dim3((unsigned)((2 * tracks + NT - 1) / NT)), dim3(NT), 0, st, poses, chained,
                       gt_local, ates, N, tracks, L);
    if (int rc = launch_status()) return rc;
  }
  hipLaunchKernelGGL(odom_summary_kernel, dim3(2), dim3(NT), 0, st, ates, summary, tracks);
  return launch_status();
}
