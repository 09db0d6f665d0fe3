// bbd_geo.hip - the geometry-consistency loss for training (ops.geometry_consistency, --geometry_consistency;
// DESIGN.md 6o; Bian et al., NeurIPS 2019): a target pixel is back-projected with its inverse depth, moved into a source
// frame with the predicted pose and its depth there is compared with the inverse depth the network predicts for that
// frame, e = |z s - 1| / (z s + 1).  Forward and backward, gradients to both inverse-depth maps and to the pose.
//
// What a sample is, its derivatives, the fixed points and the order of every addition is bbd_geo_math.h, shared with
// the host port.  What is here:
//
//   forward   geo_fwd_kernel     a work item is a run of BBD_GEO_RUN = 8 * 256 neighbouring pixels of ONE sample; a lane
//                                takes every 256th pixel of the run, for each of the V sources in turn (source outer,
//                                pixel inner, so one pair's twelve pose floats and one pair's sums are live at a time).
//                                err and code are written by the pixel's lane; the item's integer sum of e and its count
//                                go to its own slot of the scratch [B, items, V, 2]
//             geo_fwd_finish     a lane per pair adds the pair's slots (integers) -> pair_sum, pair_count
//   backward  geo_clear_kernel   zeroes the tap sums [V,B,H,W] of the scratch
//             geo_bwd_kernel     the same walk: recomputes the sample, adds the four tap values as 64-bit integers with
//                                vector atomics at agent scope, sums the pixel's grad_q_tgt over its sources in the lane,
//                                and reduces the pair's twelve pose sums in float64 in the fixed order of the header
//                                into the item's slot [B, items, V, 12]
//             geo_bwd_finish     a lane per source pixel: tap sum -> grad_q_src; the first V * B * 12 lanes also add a
//                                pair's item slots in index order -> grad_T
//
// Only integers are added atomically, every float64 sum has one written order, every output element is stored by one
// lane: identical calls give identical bytes, and the port gives the device's bytes.  Plain C++, vector stores, no
// inline assembly.  No allocation, no host synchronisation; the upstream gradient g is read on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_geo_math.h"

namespace {

typedef unsigned long long u64;

constexpr int GT = BBD_GEO_LANES;     // threads of the pixel kernels
constexpr int GW = GT / 64;
constexpr int FT = 256;               // threads of the clear and finish kernels
constexpr long MAX_GRID = 65536;      // work beyond this is reached by striding

struct GeoCall {
  const float* q_tgt;   // [B,H,W]
  const float* q_src;   // [V,B,H,W]
  const float* T;       // [V,B,12]
  const float* K;       // [B,16]
  const float* inv_K;   // [B,16]
  int B, H, W, V;
  long items;           // work items of one sample
};

__device__ __forceinline__ u64 wave_total(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(GT) void geo_fwd_kernel(GeoCall a, float* err, uint8_t* code, int64_t* slots) {
  __shared__ u64 part[GW][2];
  const int plane = a.H * a.W;                                       // V B H W <= INT_MAX
  const long total = (long)a.B * a.items;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long item = blockIdx.x; item < total; item += gridDim.x) {    // uniform over the workgroup
    const int b = (int)(item / a.items);
    const long k0 = (item - (long)b * a.items) * BBD_GEO_RUN + threadIdx.x;
    BbdGeoCamera cam;
    bbd_geo_camera(a.K, a.inv_K, b, &cam);
    for (int v = 0; v < a.V; ++v) {
      const size_t pair = (size_t)v * a.B + b;
      float T[12];
      for (int e = 0; e < 12; ++e) T[e] = a.T[pair * 12 + e];
      const float* src = a.q_src + pair * plane;
      u64 sum = 0, count = 0;
      for (int pass = 0; pass < BBD_GEO_PASSES; ++pass) {
        const long k = k0 + (long)pass * GT;
        if (k >= plane) break;
        const int y = (int)(k / a.W), x = (int)(k - (long)y * a.W);
        float p[3];
        BbdGeoSample s;
        const int vis = bbd_geo_point(&cam, a.q_tgt[(size_t)b * plane + k], x, y, p) &&
                        bbd_geo_sample(&cam, p, T, src, a.H, a.W, &s);
        if (err) err[pair * plane + k] = vis ? s.e : 0.0f;
        if (code) code[pair * plane + k] = (uint8_t)(vis ? bbd_geo_code(&s) : 0);
        if (vis) {
          sum += (u64)bbd_geo_fixed(s.e, BBD_GEO_SUM_ONE);
          count += 1;
        }
      }
      sum = wave_total(sum);
      count = wave_total(count);
      if (lane == 0) { part[wave][0] = sum; part[wave][1] = count; }
      __syncthreads();
      if (threadIdx.x < 2) {
        u64 t = 0;
        for (int wv = 0; wv < GW; ++wv) t += part[wv][threadIdx.x];
        slots[((size_t)item * a.V + v) * 2 + threadIdx.x] = (int64_t)t;
      }
      __syncthreads();                                               // the next source reuses part
    }
  }
}

__global__ __launch_bounds__(FT) void geo_fwd_finish(GeoCall a, const int64_t* slots, double* pair_sum,
                                                     int64_t* pair_count) {
  const long pairs = (long)a.V * a.B;
  for (long g = blockIdx.x * (long)FT + threadIdx.x; g < pairs; g += (long)gridDim.x * FT) {
    const int v = (int)(g / a.B), b = (int)(g - (long)v * a.B);
    int64_t sum = 0, count = 0;
    for (long it = 0; it < a.items; ++it) {
      const int64_t* s = slots + (((size_t)b * a.items + it) * a.V + v) * 2;
      sum += s[0];
      count += s[1];
    }
    pair_sum[g] = bbd_geo_pair_sum(sum);
    pair_count[g] = count;
  }
}

__global__ __launch_bounds__(FT) void geo_clear_kernel(u64* taps, long n) {
  for (long g = blockIdx.x * (long)FT + threadIdx.x; g < n; g += (long)gridDim.x * FT) taps[g] = 0;
}

__global__ __launch_bounds__(GT) void geo_bwd_kernel(GeoCall a, const double* g, float* grad_q_tgt, u64* taps,
                                                     double* slots) {
  __shared__ double part[GW][12];
  const int plane = a.H * a.W;
  const long total = (long)a.B * a.items;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long item = blockIdx.x; item < total; item += gridDim.x) {
    const int b = (int)(item / a.items);
    const long k0 = (item - (long)b * a.items) * BBD_GEO_RUN + threadIdx.x;
    BbdGeoCamera cam;
    bbd_geo_camera(a.K, a.inv_K, b, &cam);
    double gq[BBD_GEO_PASSES];
#pragma unroll
    for (int pass = 0; pass < BBD_GEO_PASSES; ++pass) gq[pass] = 0.0;
    for (int v = 0; v < a.V; ++v) {
      const size_t pair = (size_t)v * a.B + b;
      float T[12];
      for (int e = 0; e < 12; ++e) T[e] = a.T[pair * 12 + e];
      const float* src = a.q_src + pair * plane;
      u64* dst = taps + pair * plane;
      const double up = g[pair];
      double acc[12];
      for (int e = 0; e < 12; ++e) acc[e] = 0.0;
#pragma unroll
      for (int pass = 0; pass < BBD_GEO_PASSES; ++pass) {
        const long k = k0 + (long)pass * GT;
        if (k < plane) {
          const int y = (int)(k / a.W), x = (int)(k - (long)y * a.W);
          const float q = a.q_tgt[(size_t)b * plane + k];
          float p[3];
          BbdGeoSample s;
          if (bbd_geo_point(&cam, q, x, y, p) && bbd_geo_sample(&cam, p, T, src, a.H, a.W, &s)) {
            BbdGeoGrad d;
            bbd_geo_sample_grad(&cam, p, q, T, &s, &d);
            u64* r0 = dst + (size_t)s.y0 * a.W + s.x0;               // the cell lies inside the plane: x0 <= W-2, y0 <= H-2
            atomicAdd(r0, (u64)bbd_geo_fixed(d.tap[0], BBD_GEO_TAP_ONE));
            atomicAdd(r0 + 1, (u64)bbd_geo_fixed(d.tap[1], BBD_GEO_TAP_ONE));
            atomicAdd(r0 + a.W, (u64)bbd_geo_fixed(d.tap[2], BBD_GEO_TAP_ONE));
            atomicAdd(r0 + a.W + 1, (u64)bbd_geo_fixed(d.tap[3], BBD_GEO_TAP_ONE));
            gq[pass] += up * (double)d.gq;
            bbd_geo_pose_add(p, &d, acc);
          }
        }
      }
      for (int e = 0; e < 12; ++e) {
        const double r = wave_sum(acc[e]);
        if (lane == 0) part[wave][e] = r;
      }
      __syncthreads();
      if (threadIdx.x < 12) {
        double t = part[0][threadIdx.x];
        for (int wv = 1; wv < GW; ++wv) t += part[wv][threadIdx.x];
        slots[((size_t)item * a.V + v) * 12 + threadIdx.x] = t;
      }
      __syncthreads();
    }
#pragma unroll
    for (int pass = 0; pass < BBD_GEO_PASSES; ++pass) {
      const long k = k0 + (long)pass * GT;
      if (k < plane) grad_q_tgt[(size_t)b * plane + k] = (float)gq[pass];
    }
  }
}

__global__ __launch_bounds__(FT) void geo_bwd_finish(GeoCall a, const double* g, const int64_t* taps, const double* slots,
                                                     float* grad_q_src, float* grad_T) {
  const int plane = a.H * a.W;
  const long n = (long)a.V * a.B * plane, poses = (long)a.V * a.B * 12;
  const long most = n > poses ? n : poses;                           // a map of fewer than 12 pixels has more pose entries
  for (long i = blockIdx.x * (long)FT + threadIdx.x; i < most; i += (long)gridDim.x * FT) {
    if (i < n) grad_q_src[i] = bbd_geo_tap_value(taps[i], g[i / plane]);
    if (i < poses) {
      const long pair = i / 12;
      const int e = (int)(i - pair * 12), v = (int)(pair / a.B), b = (int)(pair - (long)v * a.B);
      double t = 0.0;
      for (long it = 0; it < a.items; ++it) t += slots[(((size_t)b * a.items + it) * a.V + v) * 12 + e];
      grad_T[i] = (float)(g[pair] * t);
    }
  }
}

unsigned grid_for(long items, long most) {
  return (unsigned)(items < 1 ? 1 : items < most ? items : most);
}

GeoCall geo_call(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K, int B, int H,
                 int W, int V) {
  GeoCall a;
  a.q_tgt = q_tgt; a.q_src = q_src; a.T = T; a.K = K; a.inv_K = inv_K;
  a.B = B; a.H = H; a.W = W; a.V = V;
  a.items = bbd_geo_items(H, W);
  return a;
}

}  // namespace

extern "C" int bbd_geo_fwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                           double* pair_sum, int64_t* pair_count, float* err, uint8_t* code, int64_t* scratch,
                           long scratch_words, int B, int H, int W, int V, void* stream) {
  const int rc = bbd_geo_fwd_status(q_tgt, q_src, T, K, inv_K, pair_sum, pair_count, scratch, scratch_words, B, H, W, V);
  if (rc) return rc;
  const GeoCall a = geo_call(q_tgt, q_src, T, K, inv_K, B, H, W, V);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(geo_fwd_kernel, dim3(grid_for((long)B * a.items, MAX_GRID)), dim3(GT), 0, st, a, err, code, scratch);
  hipLaunchKernelGGL(geo_fwd_finish, dim3(grid_for(((long)V * B + FT - 1) / FT, MAX_GRID)), dim3(FT), 0, st, a, scratch,
                     pair_sum, pair_count);
  return launch_status();
}

extern "C" int bbd_geo_bwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                           const double* g, float* grad_q_tgt, float* grad_q_src, float* grad_T, int64_t* scratch,
                           long scratch_words, int B, int H, int W, int V, void* stream) {
  const int rc = bbd_geo_bwd_status(q_tgt, q_src, T, K, inv_K, g, grad_q_tgt, grad_q_src, grad_T, scratch, scratch_words,
                                    B, H, W, V);
  if (rc) return rc;
  const GeoCall a = geo_call(q_tgt, q_src, T, K, inv_K, B, H, W, V);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long n = (long)V * B * H * W;
  u64* taps = reinterpret_cast<u64*>(scratch);
  double* slots = reinterpret_cast<double*>(scratch + n);
  const unsigned flat = grid_for((n + FT - 1) / FT, MAX_GRID);
  hipLaunchKernelGGL(geo_clear_kernel, dim3(flat), dim3(FT), 0, st, taps, n);
  hipLaunchKernelGGL(geo_bwd_kernel, dim3(grid_for((long)B * a.items, MAX_GRID)), dim3(GT), 0, st, a, g, grad_q_tgt, taps,
                     slots);
  hipLaunchKernelGGL(geo_bwd_finish, dim3(flat), dim3(FT), 0, st, a, g, scratch, slots, grad_q_src, grad_T);
  return launch_status();
}
