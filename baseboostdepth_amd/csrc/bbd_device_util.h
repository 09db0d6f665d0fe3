// bbd_device_util.h - device-side pieces the evaluation and picture kernels share (bbd_eval, bbd_syns, bbd_viz,
// bbd_panel, bbd_compare, ...): wave and workgroup reductions in a fixed order, LUT staging, the packed RGB store and
// the status every entry point returns.  Device code only; arithmetic the host ports share lives in the *_math.h files.
#ifndef BBD_DEVICE_UTIL_H
#define BBD_DEVICE_UTIL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bbd_panel_math.h"
#include "bbd_ragged_math.h"

constexpr int BBD_EXTREMA_PARTS = 16;   // partial (minimum, maximum) pairs per plane

// Status of the launches an entry point has just queued: 0, or the HIP error.
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Sum of one value per thread over a workgroup of THREADS threads, in a fixed order (wave sums, then the waves in
// index order); valid in every thread afterwards.  `red` is THREADS / 64 + 1 doubles of LDS.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* red) {
  constexpr int WAVES = THREADS / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double r = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int wv = 0; wv < WAVES; ++wv) s += red[wv];
    red[WAVES] = s;
  }
  __syncthreads();
  return red[WAVES];
}

__device__ __forceinline__ uint32_t wave_max(uint32_t k) {
  for (int o = 32; o > 0; o >>= 1) k = max(k, (uint32_t)__shfl_down(k, o, 64));
  return k;
}

// Workgroup blockIdx.x of BBD_EXTREMA_PARTS reduces its strided share of value(0 .. npx-1) to (~minimum key, maximum
// key) - bbd_panel_minmax_update: NaNs skipped - and stores the pair at `pair`.  Plain stores, nothing to zero.
template <int THREADS, typename F>
__device__ __forceinline__ void extrema_part(uint32_t npx, F value, uint32_t* pair) {
  constexpr int WAVES = THREADS / 64;
  __shared__ uint32_t sh[2 * WAVES];
  const int tid = threadIdx.x;
  uint32_t inv_min = 0u, max_key = 0u;
  for (uint32_t i = blockIdx.x * (uint32_t)THREADS + tid; i < npx; i += (uint32_t)BBD_EXTREMA_PARTS * THREADS)
    bbd_panel_minmax_update(value(i), &inv_min, &max_key);
  for (int o = 32; o > 0; o >>= 1) {
    inv_min = max(inv_min, (uint32_t)__shfl_down(inv_min, o, 64));
    max_key = max(max_key, (uint32_t)__shfl_down(max_key, o, 64));
  }
  if ((tid & 63) == 0) { sh[2 * (tid >> 6)] = inv_min; sh[2 * (tid >> 6) + 1] = max_key; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w) { inv_min = max(inv_min, sh[2 * w]); max_key = max(max_key, sh[2 * w + 1]); }
    pair[0] = inv_min; pair[1] = max_key;
  }
}

// The BBD_EXTREMA_PARTS pairs of one plane -> its minimum and maximum (NaN for both where the plane has no value).
__device__ __forceinline__ void extrema_combine(const uint32_t* pairs, float* vmin, float* vmax) {
  uint32_t inv_min = 0u, max_key = 0u;
  for (int p = 0; p < BBD_EXTREMA_PARTS; ++p) { inv_min = max(inv_min, pairs[2 * p]); max_key = max(max_key, pairs[2 * p + 1]); }
  bbd_panel_minmax_values(inv_min, max_key, vmin, vmax);
}

// A [ROWS,3] uint8 LUT into LDS as packed colours; stage_lut ends in the barrier that publishes it.
template <int ROWS, int THREADS>
__device__ __forceinline__ void fill_lut(uint32_t* lut, const uint8_t* src) {
  for (int i = threadIdx.x; i < ROWS; i += THREADS) lut[i] = bbd_pack_rgb(src + 3 * i);
}
template <int ROWS, int THREADS>
__device__ __forceinline__ void stage_lut(uint32_t* lut, const uint8_t* src) {
  fill_lut<ROWS, THREADS>(lut, src);
  __syncthreads();
}

// Colours c[0 .. cnt-1] of `cnt` <= 4 neighbouring pixels to `o`: 12 bytes per lane, contiguous across the wave, where
// `o` is 4-byte aligned (`aligned`) and the quad is whole; bytes otherwise.
__device__ __forceinline__ void store_quad(uint8_t* o, bool aligned, uint32_t cnt, const uint32_t c[4]) {
  if (aligned && cnt == 4u) {
    uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
    o32[0] = c[0] | (c[1] << 24);
    o32[1] = (c[1] >> 8) | (c[2] << 16);
    o32[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (uint32_t k = 0; k < cnt; ++k) bbd_put_rgb(o + 3 * k, c[k]);
  }
}

#endif  // BBD_DEVICE_UTIL_H
