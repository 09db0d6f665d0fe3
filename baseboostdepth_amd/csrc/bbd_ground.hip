// bbd_ground.hip - metric scale of a monocular prediction from the height of the camera above the road (DNet's "dense
// geometrical constraint"; ops.ground_scale).  What a ground pixel is and what goes into the output row is
// bbd_ground_math.h, shared with the host port.  What is here is two launches:
//
//   heights  ground_heights_kernel  (tiles, image): a tile is GT_W x GT_H = 64 x 16 pixels and 256 threads, four rows per
//                                   thread.  The depths of the tile and of a one-pixel halo are staged in LDS - every
//                                   depth is read from HBM once, halo pixels come from L2 - and every pixel's nine depths
//                                   are read from there.  Per pixel one float goes to the scratch map (the height of a
//                                   ground pixel, +0 or -0 elsewhere: bbd_ground_code) and, where asked for, one mask byte.
//   select   ground_select_kernel   one 1024-thread workgroup per image: the element of rank (count - 1) / 2 of the
//                                   image's heights by the exact 11+11+10-bit radix select of bbd_eval.hip on the bit
//                                   patterns (positive floats are ordered by their bits), one query, one 2048-bin LDS
//                                   histogram; the first sweep also counts the candidates.  Then the row.
//
// Integer counts only: nothing depends on launch geometry or scheduling; identical calls give identical bytes.  No
// allocation, no host synchronisation; the scratch map needs no initialisation (the first launch writes all of it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_ground_math.h"

namespace {

constexpr int GT_W = 64, GT_H = 16;            // pixels of a tile
constexpr int GT_THREADS = 256;                // 64 x 4: a thread takes rows ty, ty + 4, ty + 8, ty + 12 of its column
constexpr int GT_ROWS = GT_THREADS / GT_W;
constexpr int LW = GT_W + 2, LH = GT_H + 2;    // the staged tile: 66 floats a row, so a wave's row reads hit 64 banks
constexpr int MAX_GRID_X = 8192;               // tiles beyond this are reached by striding
constexpr int ST = 1024;                       // threads of the select kernel
constexpr int NBIN = 2048;
constexpr int SU = 8;                          // loads in flight per thread of the select kernel

struct GroundCall {
  const float* pred;     // [n,h,w]
  const float* inv_K;    // [n,3,3]
  float* rows;           // [n, BBD_EVAL_OUT]
  uint8_t* mask;         // [n,h,w] or NULL
  float* scratch;        // [n,h,w]
  int h, w, tiles_x, n_tiles, min_count, flags;
  float camera_height, cos_threshold;
};

__global__ __launch_bounds__(GT_THREADS) void ground_heights_kernel(GroundCall a) {
  __shared__ float tile[LH][LW];
  const int img = blockIdx.y, tid = threadIdx.x, tx = tid & (GT_W - 1), ty = tid >> 6;
  const int h = a.h, w = a.w;
  const size_t plane = (size_t)img * (size_t)h * (size_t)w;
  const float* pred = a.pred + plane;
  float iK[9];
  for (int j = 0; j < 9; ++j) iK[j] = a.inv_K[(size_t)img * 9 + j];
  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {                 // uniform over the workgroup
    const int y0 = (t / a.tiles_x) * GT_H, x0 = (t % a.tiles_x) * GT_W;
    for (int i = tid; i < LH * LW; i += GT_THREADS) {
      const int ly = i / LW, lx = i - ly * LW;
      const int dy = ly - 1, dx = lx - 1;                                   // compared before they are added: no sum
      const bool inside = dy < h - y0 && dx < w - x0 && y0 + dy >= 0 && x0 + dx >= 0;      // passes INT_MAX
      // outside the image: not a depth, and read by no candidate (a candidate's ring lies inside the image)
      tile[ly][lx] = inside ? bbd_ground_depth(pred[(size_t)(y0 + dy) * w + (x0 + dx)], a.flags) : 0.0f;
    }
    __syncthreads();
    const int x = x0 + tx;
    for (int r = 0; r < GT_H / GT_ROWS; ++r) {
      const int ly = ty + GT_ROWS * r, y = y0 + ly;
      if (tx < w - x0 && ly < h - y0) {
        float code = 0.0f;
        if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
          const float* c = &tile[ly + 1][tx + 1];
          const float ring[8] = {c[1], c[LW + 1], c[LW], c[LW - 1], c[-1], c[-LW - 1], c[-LW], c[-LW + 1]};
          code = bbd_ground_code(iK, x, y, c[0], ring, a.cos_threshold);
        }
        const size_t k = plane + (size_t)y * w + x;                         // < n * h * w: the size of both maps
        a.scratch[k] = code;
        if (a.mask) a.mask[k] = code > 0.0f ? 1 : 0;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(ST) void ground_select_kernel(GroundCall a) {
  __shared__ uint32_t hist[NBIN];
  __shared__ uint32_t s_prefix, s_rank, s_count, s_candidates;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t npx = (uint32_t)a.h * (uint32_t)a.w;                       // <= INT_MAX
  const uint32_t* codes = reinterpret_cast<const uint32_t*>(a.scratch) + (size_t)img * npx;
  if (tid == 0) { s_prefix = 0u; s_rank = 0u; s_count = 0u; s_candidates = 0u; }

  for (int level = 0; level < 3; ++level) {
    const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
    const int prev_shift = level == 1 ? 21 : 10;
    const uint32_t bin_mask = level == 2 ? 1023u : 2047u;
    for (int i = tid; i < NBIN; i += ST) hist[i] = 0u;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    uint32_t candidates = 0u;
    // SU loads are in flight per thread before the first is used: one workgroup of 16 waves cannot hide the latency of
    // its loads otherwise - the map was written by workgroups on other dies, so it comes from beyond this die's L2
    // (measured for 192 x 640: 94 us with one load per trip, 51 us with eight).  The heights of a
    // road crowd into a bin or two at the upper levels; adding once per wave for the lanes that share a bin (ballot,
    // shuffle, population count) was measured slower than the LDS atomics it saves, 65 us.
    for (uint32_t base = 0; base < npx; base += SU * ST) {
      uint32_t b[SU];
#pragma unroll
      for (int k = 0; k < SU; ++k) {
        const uint32_t i = base + (uint32_t)k * ST + tid;                   // < npx + SU * ST: no wrap
        b[k] = i < npx ? codes[i] : 0u;
      }
#pragma unroll
      for (int k = 0; k < SU; ++k) {
        const bool height = b[k] != 0u && b[k] != BBD_GROUND_CODE_CANDIDATE;
        candidates += b[k] != 0u ? 1u : 0u;
        if (height && (level == 0 || (b[k] >> prev_shift) == prefix)) atomicAdd(&hist[(b[k] >> shift) & bin_mask], 1u);
      }
    }
    if (level == 0) {
      for (int o = 32; o > 0; o >>= 1) candidates += __shfl_down(candidates, o, 64);
      if (lane == 0) atomicAdd(&s_candidates, candidates);
    }
    __syncthreads();
    if (wave == 0) {                    // one query: one wave resolves it
      constexpr int per = NBIN / 64;
      uint32_t mine = 0;
      for (int j = 0; j < per; ++j) mine += hist[lane * per + j];
      uint32_t incl = mine;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const uint32_t total = __shfl(incl, 63, 64);
      uint32_t rank = s_rank;
      if (level == 0) {
        rank = total ? (total - 1u) / 2u : 0u;
        if (lane == 0) s_count = total;
      }
      const uint32_t before = incl - mine;
      if (total > 0 && rank >= before && rank < incl) {
        uint32_t cum = before;
        int b = lane * per;
        for (; b < lane * per + per; ++b) {
          const uint32_t c = hist[b];
          if (rank < cum + c) break;
          cum += c;
        }
        s_prefix = (level == 0 ? 0u : (prefix << (level == 2 ? 10 : 11))) | (uint32_t)b;
        s_rank = rank - cum;
      }
    }
    __syncthreads();
  }
  if (tid < BBD_EVAL_OUT)
    a.rows[(size_t)img * BBD_EVAL_OUT + tid] =
        bbd_ground_row(tid, s_prefix, s_count, s_candidates, a.min_count, a.camera_height);
}

}  // namespace

extern "C" long bbd_ground_scale_scratch_floats(int n, int h, int w) { return bbd_ground_scratch_floats(n, h, w); }

extern "C" int bbd_ground_scale(const float* pred, const float* inv_K, float* rows, uint8_t* mask, float* scratch, int n,
                                int h, int w, double camera_height, double cos_threshold, int min_count, int flags,
                                void* stream) {
  const int rc = bbd_ground_args_status(pred, inv_K, rows, scratch, n, h, w, camera_height, cos_threshold, min_count,
                                        flags);
  if (rc) return rc;
  GroundCall a;
  a.pred = pred; a.inv_K = inv_K; a.rows = rows; a.mask = mask; a.scratch = scratch;
  a.h = h; a.w = w; a.min_count = min_count; a.flags = flags;
  a.camera_height = (float)camera_height; a.cos_threshold = (float)cos_threshold;
  a.tiles_x = (w - 1) / GT_W + 1;
  const long n_tiles = (long)a.tiles_x * (long)((h - 1) / GT_H + 1);       // < h * w / 1024 + h / 16 + w / 64 + 2
  a.n_tiles = (int)n_tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(n_tiles < MAX_GRID_X ? n_tiles : MAX_GRID_X), (unsigned)n);
  hipLaunchKernelGGL(ground_heights_kernel, grid, dim3(GT_THREADS), 0, st, a);
  hipLaunchKernelGGL(ground_select_kernel, dim3((unsigned)n), dim3(ST), 0, st, a);
  return launch_status();
}
