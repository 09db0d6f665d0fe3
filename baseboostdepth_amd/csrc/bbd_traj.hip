// bbd_traj.hip - full-trajectory KITTI odometry scores on the device: the trajectory chained from the pose network's
// single steps, its alignment to ground truth (Umeyama / rigid / scale only / none), the ATE of the aligned trajectory
// and the devkit's sub-sequence errors t_rel and r_rel.  bbd_pose_trajectory enqueues four launches and
// reads nothing back:
//   1. a lane per frame: G^_j = inv(G_0) G_j into gt_traj, inv(steps[j]) into row j + 1 of traj (the scan's input)
//   2. ONE workgroup of 256: the blocked scan of the inverses into the trajectory (chunk products, a doubling scan of
//      the 256 chunk products in LDS, replay), the path length, the moments, the alignment (lane 0), the aligned poses
//      and the ATE figures
//   3. a lane per (first, length) pair: binary search for `last`, three 4x4 inverses and products, acos
//   4. one workgroup: the means over the valid pairs
// No atomics and no order that depends on the launch geometry: the arithmetic and its order are bbd_traj_math.h, which
// the host port of the test tier compiles too, so identical calls give identical bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_traj_math.h"

namespace {

constexpr int NT = BBD_TRAJ_LANES;
static_assert(BBD_TRAJ_MODE_SIM3 == BBD_TRAJ_SIM3 && BBD_TRAJ_MODE_SE3 == BBD_TRAJ_SE3 &&
                  BBD_TRAJ_MODE_SCALE == BBD_TRAJ_SCALE && BBD_TRAJ_MODE_NONE == BBD_TRAJ_NONE,
              "the modes of the header and of the arithmetic");
static_assert(BBD_TRAJ_MAX_LENGTHS == BBD_TRAJ_MAX_LEN, "the lengths of the header and of the arithmetic");

__global__ __launch_bounds__(NT) void traj_matrices_kernel(const float* __restrict__ steps, const double* __restrict__ gt,
                                                           double* __restrict__ traj, double* __restrict__ gt_traj, int J) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j > J) return;
  double m[16];
  bbd_traj_gt_rel(gt, j, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) gt_traj[(size_t)j * 16 + e] = m[e];
  if (j < J) {
    bbd_traj_step_inv(steps, j, m);
#pragma unroll
    for (int e = 0; e < 16; ++e) traj[(size_t)(j + 1) * 16 + e] = m[e];
  }
}

// the halving tree of the means for N sums at once (red: N rows of NT doubles); valid in every lane afterwards
template <int N>
__device__ __forceinline__ void tree_sums(double* red, double* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int e = 0; e < N; ++e) red[e * NT + t] = v[e];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int e = 0; e < N; ++e) red[e * NT + t] = red[e * NT + t] + red[e * NT + t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = red[e * NT];
  __syncthreads();
}

__device__ __forceinline__ double tree_max(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = red[t + s] > red[t] ? red[t + s] : red[t];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

// traj, gt_traj, aligned and dist are read back after they were written by other lanes of this workgroup: no
// __restrict__, and a __syncthreads() (workgroup-scope release / acquire) between the write and the read.
__global__ __launch_bounds__(NT) void traj_scan_kernel(double* traj, const double* gt_traj, double* aligned,
                                                       double* transform, double* dist, double* summary, int J, int mode) {
  __shared__ double lds[NT * 16];  // the scan's 256 matrices, then the rows of the means' trees
  __shared__ double red[NT];
  double(*Q)[16] = reinterpret_cast<double(*)[16]>(lds);
  __shared__ bbd_traj_align_t al;
  const int t = threadIdx.x, F = J + 1;

  // ---- the trajectory
  double own[16], other[16];
  bbd_traj_chunk_product(traj, J, t, own);
#pragma unroll
  for (int e = 0; e < 16; ++e) Q[t][e] = own[e];
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    if (t >= d) {
#pragma unroll
      for (int e = 0; e < 16; ++e) other[e] = Q[t - d][e];
    }
    __syncthreads();
    if (t >= d) {
      double r[16];
      bbd_odom_mul4d(other, own, r);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        own[e] = r[e];
        Q[t][e] = r[e];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    bbd_odom_eye(own);
#pragma unroll
    for (int e = 0; e < 16; ++e) traj[e] = own[e];
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) own[e] = Q[t - 1][e];
  }
  bbd_traj_replay(traj, J, t, own);

  // ---- the path length
  red[t] = bbd_traj_dist_chunk(gt_traj, dist, J, t, 0, 0.0);
  __syncthreads();
  if (t == 0) {
    double off = 0.0;
    for (int k = 0; k < NT; ++k) {
      const double total = red[k];
      red[k] = off;
      off = off + total;
    }
    dist[0] = 0.0;
  }
  __syncthreads();
  bbd_traj_dist_chunk(gt_traj, dist, J, t, 1, red[t]);
  __syncthreads();  // also publishes traj

  // ---- the moments and the alignment
  double m[20];
#pragma unroll
  for (int e = 0; e < 20; ++e) m[e] = 0.0;
  if (mode == BBD_TRAJ_MODE_SIM3 || mode == BBD_TRAJ_MODE_SE3) {
    bbd_traj_partials(traj, gt_traj, F, t, BBD_TRAJ_T_P, 6, m, m);  // the means first: the later terms are centred on them
    tree_sums<6>(lds, m);
#pragma unroll
    for (int w = 0; w < 6; ++w) m[w] = m[w] / (double)F;
    bbd_traj_partials(traj, gt_traj, F, t, BBD_TRAJ_T_VAR, 10, m, m + BBD_TRAJ_T_VAR);
    tree_sums<10>(lds, m + BBD_TRAJ_T_VAR);
#pragma unroll
    for (int w = BBD_TRAJ_T_VAR; w < BBD_TRAJ_T_GP; ++w) m[w] = m[w] / (double)F;
  } else if (mode == BBD_TRAJ_MODE_SCALE) {
    bbd_traj_partials(traj, gt_traj, F, t, BBD_TRAJ_T_GP, 2, m, m + BBD_TRAJ_T_GP);
    tree_sums<2>(lds, m + BBD_TRAJ_T_GP);
  }
  if (t == 0) {
    bbd_traj_align(m, mode, &al);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int s = 0; s < 3; ++s) transform[4 * r + s] = al.R[3 * r + s];
      transform[4 * r + 3] = al.t[r];
    }
    transform[12] = 0.0;
    transform[13] = 0.0;
    transform[14] = 0.0;
    transform[15] = 1.0;
  }
  __syncthreads();

  // ---- the aligned poses and the ATE figures
  for (int j = t; j < F; j += NT) {
    double C[16], out[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) C[e] = traj[(size_t)j * 16 + e];
    bbd_traj_apply(&al, C, out);
#pragma unroll
    for (int e = 0; e < 16; ++e) aligned[(size_t)j * 16 + e] = out[e];
  }
  // each lane reads back only the rows it wrote (the same j = t, t + 256, ..)
  double e2[2];
  bbd_traj_partials(aligned, gt_traj, F, t, BBD_TRAJ_T_ESQ, 2, m, e2);
  tree_sums<2>(lds, e2);
  const double sq = e2[0], se = e2[1];
  const double mx = tree_max(red, bbd_traj_partial_max(aligned, gt_traj, F, t));
  if (t == 0) {
    summary[3] = bbd_odom_canon(sqrt(sq / (double)F));
    summary[4] = bbd_odom_canon(se / (double)F);
    summary[5] = bbd_odom_canon(sq != sq ? sq : mx);
    summary[6] = al.c;
    summary[7] = (double)F;
  }
}

__global__ __launch_bounds__(NT) void traj_pairs_kernel(const double* __restrict__ gt_traj, const double* __restrict__ aligned,
                                                        const double* __restrict__ dist, double* __restrict__ pairs,
                                                        bbd_traj_lengths_t lengths, int F, int n_first, int n_len, int step) {
  const int k = blockIdx.x * NT + threadIdx.x;
  if (k >= n_first * n_len) return;
  const int fi = k / n_len, l = k - fi * n_len;
  double L = lengths.v[0];
#pragma unroll
  for (int i = 1; i < BBD_TRAJ_MAX_LENGTHS; ++i) L = (i == l) ? lengths.v[i] : L;  // no indexed read of a kernel argument
  bbd_traj_pair(gt_traj, aligned, dist, F, fi * step, L, pairs + (size_t)k * 4);
}

__global__ __launch_bounds__(NT) void traj_summary_kernel(const double* __restrict__ pairs, double* __restrict__ per_length,
                                                          double* __restrict__ summary, int n_first, int n_len) {
  __shared__ double red[3 * NT];
  const int t = threadIdx.x;
  for (int l = -1; l < n_len; ++l) {  // -1: every pair, flat
    const double* base = l < 0 ? pairs : pairs + (size_t)l * 4;
    const int count = l < 0 ? n_first * n_len : n_first, stride = l < 0 ? 1 : n_len;
    double s3[3];
    bbd_traj_pair_partials(base, count, stride, t, s3);
    tree_sums<3>(red, s3);
    const double n = s3[0], te = s3[1], re = s3[2];
    if (t == 0) {
      double* o = l < 0 ? summary : per_length + (size_t)l * 3;
      o[0] = bbd_odom_canon(te / n);
      o[1] = bbd_odom_canon(re / n);
      o[2] = n;
    }
  }
}

}  // namespace

extern "C" int bbd_pose_trajectory(const float* steps, const double* gt, const double* lengths, double* traj, double* gt_traj,
                                   double* aligned, double* transform, double* dist, double* pairs, double* per_length,
                                   double* summary, int J, int M, int n_len, int step, int mode, void* stream) {
  if (!steps || !gt || !traj || !gt_traj || !aligned || !transform || !dist || !pairs || !per_length || !summary)
    return BBD_E_BADARG;
  if (int rc = bbd_traj_check(J, M, lengths, n_len, step, mode)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int F = J + 1, n_first = (F + step - 1) / step;
  if ((long)n_first * n_len > 0x7fffffffL / 4) return BBD_E_TOOMANY;
  bbd_traj_lengths_t len;
  for (int l = 0; l < BBD_TRAJ_MAX_LENGTHS; ++l) len.v[l] = l < n_len ? lengths[l] : 0.0;
  hipLaunchKernelGGL(traj_matrices_kernel, dim3((unsigned)((F + NT - 1) / NT)), dim3(NT), 0, st, steps, gt, traj, gt_traj, J);
  if (int rc = launch_status()) return rc;
  hipLaunchKernelGGL(traj_scan_kernel, dim3(1), dim3(NT), 0, st, traj, gt_traj, aligned, transform, dist, summary, J, mode);
  if (int rc = launch_status()) return rc;
  hipLaunchKernelGGL(traj_pairs_kernel, dim3((unsigned)((n_first * n_len + NT - 1) / NT)), dim3(NT), 0, st, gt_traj, aligned,
                     dist, pairs, len, F, n_first, n_len, step);
  if (int rc = launch_status()) return rc;
  hipLaunchKernelGGL(traj_summary_kernel, dim3(1), dim3(NT), 0, st, pairs, per_length, summary, n_first, n_len);
  return launch_status();
}
