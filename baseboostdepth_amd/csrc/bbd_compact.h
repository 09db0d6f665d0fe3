// bbd_compact.h - the deterministic stream compaction bbd_cloud.hip and bbd_map.hip share: kept items go, in index order
// and without gaps, to the start of a region.  Three launches in the caller's kernels:
//
//   count  every chunk (one item per lane of a workgroup) counts its kept lanes: compact_ballot, a barrier, compact_total
//   scan   one workgroup turns a table of chunk totals into exclusive prefixes in place: compact_scan
//   write  the same lanes decide again; a kept lane's slot is compact_slot after compact_ballot and a barrier
//
// Integer sums only, no atomics: the result depends on nothing but which items are kept.  Device code only.
#ifndef BBD_COMPACT_H
#define BBD_COMPACT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// 64-bit ballot of `keep` over the wave; lane 0 leaves the wave's count in wave_kept[wave].  The caller's barrier
// publishes it.
__device__ __forceinline__ unsigned long long compact_ballot(bool keep, int* wave_kept) {
  const unsigned long long mask = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_kept[threadIdx.x >> 6] = __popcll(mask);
  return mask;
}

// Kept lanes of the whole chunk, waves added in index order.
template <int WAVES>
__device__ __forceinline__ int compact_total(const int* wave_kept) {
  int s = 0;
  for (int wv = 0; wv < WAVES; ++wv) s += wave_kept[wv];
  return s;
}

// Slot of a kept lane: the chunk's prefix + kept lanes of the waves before it + kept lanes below it in its wave.
__device__ __forceinline__ int compact_slot(int chunk_prefix, unsigned long long mask, const int* wave_kept) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int slot = chunk_prefix;
  for (int wv = 0; wv < wave; ++wv) slot += wave_kept[wv];
  return slot + __popcll(mask & ((1ull << lane) - 1ull));
}

// Exclusive prefix sum of table[0 .. n_chunks-1] in place, by one workgroup of THREADS threads; *total = the sum.  A
// lane owns a contiguous run of the table, runs are combined with a shuffle scan in the wave and a serial sum over the
// waves.  `wave_total` is THREADS / 64 ints of LDS.
template <int THREADS>
__device__ __forceinline__ void compact_scan(int32_t* table, int n_chunks, int* wave_total, int32_t* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int run = (n_chunks + THREADS - 1) / THREADS, j0 = min(tid * run, n_chunks), j1 = min(j0 + run, n_chunks);
  int s = 0;
  for (int j = j0; j < j1; ++j) s += table[j];
  int incl = s;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int before = 0;
  for (int wv = 0; wv < wave; ++wv) before += wave_total[wv];
  int prefix = before + incl - s;                                    // kept items before this lane's run
  for (int j = j0; j < j1; ++j) {
    const int t = table[j];
    table[j] = prefix;
    prefix += t;
  }
  if (tid == THREADS - 1) *total = before + incl;
}

#endif  // BBD_COMPACT_H
