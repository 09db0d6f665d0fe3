// bbd_align.hip - affine-invariant depth evaluation on the device: the scale AND shift of a relative-depth
// prediction (MiDaS, DPT, Depth Anything: disparity up to an unknown affine map) fitted to the ground truth by least
// squares in inverse-depth space, per image, then the seven metrics of bbd_depth_metrics, SILog and iRMSE.
//
// The launch geometry of bbd_depth_metrics: one 1024-thread workgroup owns one image of a ragged batch and sweeps the
// crop window three times, resampling the prediction on the fly at every scored pixel (never materialised):
//   sweep 1  sum x, sum t, N, min x, max x        -> the means
//   sweep 2  centred second moments               -> scale, shift
//   sweep 3  the aligned, capped, clamped depth   -> ten error sums
// Every sum is float64 in the order bbd_align_math.h writes down (strided partials, a pairwise tree in the wave, the
// waves in index order): no atomics, no scratch, identical calls give identical bytes.  LDS holds the wave sums only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_align_math.h"

namespace {

constexpr int AT = BBD_ALIGN_THREADS;
constexpr int AW = BBD_ALIGN_WAVES;
constexpr int AK = BBD_ALIGN_ERR_SUMS;   // the widest group of sums

struct AlignArgs {
  const float* pred;       // [n,h,w] disparity-like, any affine gauge
  const float* gt;         // ragged ground truth
  const int32_t* desc;     // [n, BBD_EVAL_DESC]
  double* out;             // [n, BBD_ALIGN_OUT]
  int h, w;
  double max_depth;
  float lo, hi;            // the depth range in float32
};

// K sums of one value per thread each, combined as bbd_align_combine does: wave_sum is its pairwise tree (lane 0), thread
// k adds the waves of sum k in index order; every thread holds the totals afterwards.
template <int K>
__device__ __forceinline__ void block_sums(double* v, double (*red)[AK], double* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll                           // v stays in registers: no dynamic index
  for (int k = 0; k < K; ++k) {
    const double r = wave_sum(v[k]);
    if (lane == 0) red[wave][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double s = 0.0;
    for (int wv = 0; wv < AW; ++wv) s += red[wv][threadIdx.x];
    total[threadIdx.x] = s;
  }
  __syncthreads();                       // red may be written again; total is read before the next call's first barrier
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = total[k];
}

__global__ __launch_bounds__(AT) void depth_metrics_affine_kernel(AlignArgs a) {
  __shared__ double red[AW][AK], total[AK];
  __shared__ float ext[AW][2];

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BbdUncertWindow win = bbd_uncert_window(a.desc, img);
  const float* gt = a.gt + win.off;
  const float* pr = a.pred + (size_t)img * a.h * a.w;
  double* out = a.out + (size_t)img * BBD_ALIGN_OUT;

  // ---- sweep 1: the means, the count and the spread
  double s1[3] = {0.0, 0.0, 0.0};
  float lo = INFINITY, hi = -INFINITY;
  for (long j = tid; j < win.area; j += AT) {
    const int y = win.r0 + (int)(j / win.ww), x = win.c0 + (int)(j % win.ww);
    const float g = gt[(size_t)y * win.GW + x];
    if (!bbd_uncert_valid(g, a.lo, a.hi)) continue;
    bbd_align_sample(bbd_eval_resample_linear(pr, a.h, a.w, y, x, win.GH, win.GW), g, s1, &lo, &hi);
    s1[2] += 1.0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if (lane == 0) { ext[wave][0] = lo; ext[wave][1] = hi; }
  block_sums<3>(s1, red, total);         // its barriers publish ext as well
  lo = ext[0][0]; hi = ext[0][1];
  for (int wv = 1; wv < AW; ++wv) {
    lo = ext[wv][0] < lo ? ext[wv][0] : lo;
    hi = ext[wv][1] > hi ? ext[wv][1] : hi;
  }
  const double N = s1[2];
  if (bbd_align_degenerate(N, lo, hi)) {  // uniform: every thread holds the same N, lo, hi
    if (tid == 0) bbd_align_empty(N, out);
    return;
  }

  // ---- sweep 2: the centred moments
  const double mx = s1[0] / N, mt = s1[1] / N;
  double s2[2] = {0.0, 0.0};
  for (long j = tid; j < win.area; j += AT) {
    const int y = win.r0 + (int)(j / win.ww), x = win.c0 + (int)(j % win.ww);
    const float g = gt[(size_t)y * win.GW + x];
    if (!bbd_uncert_valid(g, a.lo, a.hi)) continue;
    bbd_align_centred(bbd_eval_resample_linear(pr, a.h, a.w, y, x, win.GH, win.GW), g, mx, mt, s2);
  }
  block_sums<2>(s2, red, total);
  const BbdAlignFit fit = bbd_align_fit(s1[0], s1[1], s2[0], s2[1], N);

  // ---- sweep 3: the errors of the aligned depth
  double s3[AK];
  for (int k = 0; k < AK; ++k) s3[k] = 0.0;
  for (long j = tid; j < win.area; j += AT) {
    const int y = win.r0 + (int)(j / win.ww), x = win.c0 + (int)(j % win.ww);
    const float g = gt[(size_t)y * win.GW + x];
    if (!bbd_uncert_valid(g, a.lo, a.hi)) continue;
    const float v = bbd_eval_resample_linear(pr, a.h, a.w, y, x, win.GH, win.GW);
    bbd_align_errors(bbd_align_depth(v, fit, a.max_depth, a.lo, a.hi), g, s3);
  }
  block_sums<AK>(s3, red, total);
  if (tid == 0) bbd_align_finish(s3, N, fit, out);
}

}  // namespace

extern "C" int bbd_depth_metrics_affine(const float* pred, const float* gt, const int32_t* desc, double* out, int n,
                                        int h, int w, double min_depth, double max_depth, int flags, void* stream) {
  const int rc = bbd_align_status(pred, gt, desc, out, n, h, w, min_depth, max_depth, flags);
  if (rc) return rc;
  AlignArgs a;
  a.pred = pred; a.gt = gt; a.desc = desc; a.out = out; a.h = h; a.w = w;
  a.max_depth = max_depth; a.lo = (float)min_depth; a.hi = (float)max_depth;
  hipLaunchKernelGGL(depth_metrics_affine_kernel, dim3((unsigned)n), dim3(AT), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}
