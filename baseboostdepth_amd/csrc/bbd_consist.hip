// bbd_consist.hip - depth-pose geometric consistency: a pixel of a reference frame is back-projected with its depth,
// moved into a source frame with the relative pose, and the depth it should have there is compared with the depth the
// source frame predicts at that place (ops.depth_consistency, evaluate_pose.py --consistency / --map_consistent;
// DESIGN.md 6m).
//
// What a pair's transform is and what a pixel becomes is bbd_consist_math.h, shared with the host port.  What is here:
//
//   transforms  consist_transform_kernel  a lane per (frame, view): inv(P_src) . P_ref into the caller's `transforms`;
//                                         the same launch clears the call's counters
//   pixels      consist_pixel_kernel      a gather.  A work item is a run of RUN = 8 * 256 neighbouring pixels of ONE
//                                         frame, so the lanes of a workgroup share their V sources: the V transforms
//                                         and source indices are staged in LDS once per item, K is widened once per
//                                         lane.  A lane takes every 256th pixel of the run and loops over a pixel's
//                                         sources; the four taps of neighbouring lanes are neighbouring addresses of
//                                         the source frame.  Work items beyond the grid are reached by striding.  The
//                                         five counters are summed per lane over the run, then in the wave by
//                                         shuffles, then over the four waves through LDS: one 64-bit integer atomicAdd
//                                         per item and counter that is not zero.  (One add per wave and 256 pixels was
//                                         measured first: the waves in flight at any moment belong to three or four
//                                         frames, so their adds queued on three or four cache lines and the launch took
//                                         six times as long - profiles/consist/README.md.)
//
// Only integers are added, so the counters do not depend on the launch geometry or the order of arrival; every other
// output is written by exactly one lane.  Plain vector global atomics at agent scope; no inline assembly.
// No allocation, no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_consist_math.h"
#include "bbd_device_util.h"

namespace {

typedef unsigned long long u64;

constexpr int CT = 256;               // threads of the pixel kernel
constexpr int CW = CT / 64;
constexpr int PASSES = 8;             // pixels per lane and work item
constexpr int RUN = CT * PASSES;      // pixels of a work item
constexpr int TT = 64;                // threads of the transform kernel
constexpr long MAX_GRID = 65536;      // work items beyond this are reached by striding

struct ConsistCall {
  BbdConsistParams p;
  const double* poses;       // [n,16]
  const double* scale;       // one double, or NULL = 1
  const int32_t* sources;    // [n,V]
  double* transforms;        // [n,V,12]
  uint8_t* seen;             // [n,h,w]
  uint8_t* agree;            // [n,h,w]
  uint32_t* err;             // [n,h,w] float bits, or NULL
  float* filtered;           // [n,h,w], or NULL
  u64* counters;             // [n,BBD_CONSIST_COUNTERS]
};

__global__ __launch_bounds__(TT) void consist_transform_kernel(ConsistCall a) {
  const long pairs = (long)a.p.n * a.p.V;
  for (long g = blockIdx.x * (long)TT + threadIdx.x; g < pairs; g += (long)gridDim.x * TT) {
    const int i = (int)(g / a.p.V), v = (int)(g - (long)i * a.p.V);
    bbd_consist_transform(a.poses, i, bbd_consist_source(a.sources, a.p.n, a.p.V, i, v), a.transforms + 12 * g);
    for (int c = v; c < BBD_CONSIST_COUNTERS; c += a.p.V) a.counters[(size_t)i * BBD_CONSIST_COUNTERS + c] = 0;
  }
}

__device__ __forceinline__ u64 wave_total(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(CT) void consist_pixel_kernel(ConsistCall a) {
  __shared__ double M[BBD_CONSIST_MAX_VIEWS * 12];
  __shared__ int src[BBD_CONSIST_MAX_VIEWS];
  __shared__ u64 part[CW][BBD_CONSIST_COUNTERS];
  const double scale = a.scale ? *a.scale : 1.0;
  double K9[9];
  for (int e = 0; e < 9; ++e) K9[e] = (double)a.p.K[e];
  const int plane = a.p.h * a.p.w;                                  // n h w <= INT_MAX
  const long per_frame = (plane + RUN - 1) / RUN, items = (long)a.p.n * per_frame;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {   // uniform over the workgroup
    const int i = (int)(item / per_frame);
    const long k0 = (item - (long)i * per_frame) * RUN + threadIdx.x;
    if (threadIdx.x < a.p.V * 12) M[threadIdx.x] = a.transforms[(size_t)i * a.p.V * 12 + threadIdx.x];
    if (threadIdx.x < a.p.V) src[threadIdx.x] = bbd_consist_source(a.sources, a.p.n, a.p.V, i, (int)threadIdx.x);
    __syncthreads();
    u64 sum[BBD_CONSIST_COUNTERS] = {0, 0, 0, 0, 0};
    for (int pass = 0; pass < PASSES; ++pass) {
      const long k = k0 + (long)pass * CT;
      if (k >= plane) break;
      BbdConsistPixel px;
      bbd_consist_pixel(&a.p, scale, K9, src, M, i, (int)k, &px);
      const size_t at = (size_t)i * plane + (size_t)k;              // < n h w
      a.seen[at] = (uint8_t)px.seen;
      a.agree[at] = (uint8_t)px.agree;
      if (a.err) a.err[at] = px.err_bits;
      if (a.filtered) a.filtered[at] = px.filtered;
      sum[0] += (u64)px.valid; sum[1] += (u64)px.seen; sum[2] += (u64)px.agree; sum[3] += (u64)px.err_sum;
      sum[4] += (u64)px.kept;
    }
    for (int c = 0; c < BBD_CONSIST_COUNTERS; ++c) {
      const u64 total = wave_total(sum[c]);
      if (lane == 0) part[wave][c] = total;
    }
    __syncthreads();
    if (threadIdx.x < BBD_CONSIST_COUNTERS) {
      u64 total = 0;
      for (int wv = 0; wv < CW; ++wv) total += part[wv][threadIdx.x];
      if (total) atomicAdd(a.counters + (size_t)i * BBD_CONSIST_COUNTERS + threadIdx.x, total);
    }
    __syncthreads();                                                // the next item restages M, src and part
  }
}

unsigned grid_for(long items, long most) {
  return (unsigned)(items < 1 ? 1 : items < most ? items : most);
}

}  // namespace

extern "C" int bbd_depth_consistency(const float* disp, const double* poses, const double* scale, const float* K,
                                     const float* inv_K, const int32_t* sources, double* transforms, uint8_t* seen,
                                     uint8_t* agree, float* err, float* filtered, int64_t* counters, int n, int h, int w,
                                     int V, double threshold, int min_views, int flags, void* stream) {
  const int rc = bbd_consist_status(disp, poses, K, inv_K, sources, transforms, seen, agree, counters, n, h, w, V,
                                    threshold, min_views, flags);
  if (rc) return rc;
  ConsistCall a;
  a.p.disp = disp; a.p.K = K; a.p.inv_K = inv_K;
  a.p.n = n; a.p.h = h; a.p.w = w; a.p.V = V; a.p.flags = flags; a.p.min_views = min_views; a.p.threshold = threshold;
  a.poses = poses; a.scale = scale; a.sources = sources; a.transforms = transforms;
  a.seen = seen; a.agree = agree; a.err = reinterpret_cast<uint32_t*>(err); a.filtered = filtered;
  a.counters = reinterpret_cast<u64*>(counters);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long pairs = (long)n * V, items = (long)n * (((long)h * w + RUN - 1) / RUN);
  hipLaunchKernelGGL(consist_transform_kernel, dim3(grid_for((pairs + TT - 1) / TT, MAX_GRID)), dim3(TT), 0, st, a);
  hipLaunchKernelGGL(consist_pixel_kernel, dim3(grid_for(items, MAX_GRID)), dim3(CT), 0, st, a);
  return launch_status();
}
