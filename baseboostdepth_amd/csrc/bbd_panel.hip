// bbd_panel.hip - the training log's picture, rendered on the device (reference trainer.py:678-772 logs the target, the
// source, the warp and the colour-mapped disparity per frame id through the host).
//
// The fused forward never writes its warps (unless asked to), and under --rand the step is a graph replay on static
// buffers - so the panel is rendered afterwards from what the step leaves behind: depth, pose rows, frames, the arg-min
// and minimum-loss maps.  A WARP tile runs the per-pixel functions of bbd_math.h exactly as warp_into_lds does for
// `warped_out`: the panel shows the warp the loss saw.
//
//   launch 1  per SCALAR tile, PARTS workgroups each reduce a strided share of the plane to (minimum, maximum) as order
//             keys (NaNs skipped) and store the pair in scratch - plain stores, nothing to zero, no atomics
//   launch 2  one column of workgroups per grid cell: finds the cell's tile in the descriptor table, combines the PARTS
//             pairs, renders four pixels of a row per thread (12-byte packed stores where the address allows, bytes
//             otherwise: W*3 need not be a multiple of 4); cells without a tile are zero-filled
//
// bbd_argmin_hist: per-sample histogram of the arg-min ids, LDS counters spread over 32 copies, integer atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_viz_math.h"
#include "bbd_panel_math.h"
#include "bbd_device_util.h"

namespace {

constexpr int PT = 256;              // threads per workgroup
constexpr int PARTS = BBD_EXTREMA_PARTS;   // partial extrema per SCALAR tile
constexpr int MAX_GX = 1024;         // workgroups per cell at most (grid-stride beyond)

struct PanelArgs {
  const int32_t* desc;      // [n_tiles, BBD_PANEL_DESC]
  const float* pose;        // [NP, BBD_POSE_STRIDE]
  const uint8_t* lut;       // [BBD_PANEL_LUT_ROWS, 3]
  uint8_t* out;             // [rows*H, cols*W, 3]
  float* stats;             // [n_tiles, 2]
  uint32_t* scratch;        // [n_tiles, PARTS, 2]  ~minimum key, maximum key
  int n_tiles, NP, rows, cols;
  BbdDims dm;
};

struct Tile {
  int kind, cell, p0, p1;
  const void* src;
  const void* aux;
};

__device__ __forceinline__ const void* address(int32_t lo, int32_t hi) {
  return reinterpret_cast<const void*>(bbd_join64(lo, hi));
}

__device__ __forceinline__ Tile load_tile(const PanelArgs& a, int t) {
  const int32_t* d = a.desc + (size_t)t * BBD_PANEL_DESC;
  Tile tl;
  tl.kind = d[0]; tl.cell = d[1];
  tl.src = address(d[2], d[3]);
  tl.aux = address(d[4], d[5]);
  tl.p0 = d[6]; tl.p1 = d[7];
  return tl;
}

__global__ __launch_bounds__(PT) void panel_extrema_kernel(PanelArgs a) {
  const int t = blockIdx.y;
  const Tile tl = load_tile(a, t);
  if (tl.kind != BBD_PANEL_SCALAR || tl.src == nullptr) return;            // uniform
  const float* plane = static_cast<const float*>(tl.src);
  extrema_part<PT>((uint32_t)a.dm.H * (uint32_t)a.dm.W, [&](uint32_t i) { return plane[i]; },
                   a.scratch + ((size_t)t * PARTS + blockIdx.x) * 2);
}

__global__ __launch_bounds__(PT) void panel_render_kernel(PanelArgs a) {
  __shared__ uint32_t lut[BBD_PANEL_LUT_ROWS];                     // r | g << 8 | b << 16
  const int cell = blockIdx.y, tid = threadIdx.x;
  const int H = a.dm.H, W = a.dm.W;
  int t = -1;
  for (int i = 0; i < a.n_tiles; ++i)                             // uniform: scalar loads; the last tile of a cell wins
    if (a.desc[(size_t)i * BBD_PANEL_DESC + 1] == cell) t = i;
  Tile tl;
  tl.kind = -1; tl.cell = cell; tl.p0 = tl.p1 = 0; tl.src = tl.aux = nullptr;
  if (t >= 0) tl = load_tile(a, t);
  int kind = tl.src != nullptr ? tl.kind : -1;
  if (kind == BBD_PANEL_WARP && (tl.aux == nullptr || tl.p0 < 0 || tl.p0 >= a.NP || H < 2 || W < 2)) kind = -1;

  float vmin = 0.0f, vmax = 0.0f;
  float pj[21];
  if (kind == BBD_PANEL_SCALAR || kind == BBD_PANEL_ARGMIN) stage_lut<BBD_PANEL_LUT_ROWS, PT>(lut, a.lut);   // uniform
  if (kind == BBD_PANEL_SCALAR) {
    extrema_combine(a.scratch + (size_t)t * PARTS * 2, &vmin, &vmax);
    if (blockIdx.x == 0 && tid == 0) { a.stats[(size_t)t * 2] = vmin; a.stats[(size_t)t * 2 + 1] = vmax; }
  }
  if (kind == BBD_PANEL_WARP) bbd_make_proj(a.pose + (size_t)tl.p0 * BBD_POSE_STRIDE, pj);

  const size_t hw = (size_t)H * (size_t)W;
  const uint32_t gw = ((uint32_t)W + 3u) / 4u, ngroups = (uint32_t)H * gw;
  const int row = cell / a.cols, col = cell - row * a.cols;
  const size_t out_row = (size_t)a.cols * (size_t)W;               // pixels per output row
  const uint32_t* lut_sel = lut + (tl.p0 == 1 ? 256 : 0);
  for (uint32_t g = blockIdx.x * PT + tid; g < ngroups; g += gridDim.x * PT) {
    const int y = (int)(g / gw), x0 = (int)(g - (uint32_t)y * gw) * 4;
    const int cnt = W - x0 < 4 ? W - x0 : 4;
    const size_t i0 = (size_t)y * W + x0;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= cnt) break;
      if (kind == BBD_PANEL_COLOR) {
        c[k] = bbd_panel_color(static_cast<const float*>(tl.src), hw, i0 + k);
      } else if (kind == BBD_PANEL_WARP) {
        float val[3];
        c[k] = bbd_panel_warp(static_cast<const float*>(tl.src), static_cast<const float*>(tl.aux), pj, a.dm, x0 + k, y, val);
      } else if (kind == BBD_PANEL_SCALAR) {
        c[k] = lut_sel[bbd_viz_lut_index(static_cast<const float*>(tl.src)[i0 + k], vmin, vmax)];
      } else if (kind == BBD_PANEL_ARGMIN) {
        c[k] = bbd_panel_argmin_colour(lut + 512, static_cast<const uint8_t*>(tl.src)[i0 + k], tl.p0, tl.p1);
      }
    }
    uint8_t* o = a.out + (((size_t)row * H + y) * out_row + (size_t)col * W + x0) * 3;
    store_quad(o, (((uintptr_t)o) & 3u) == 0, (uint32_t)cnt, c);
  }
}

constexpr int HC = 32;               // copies of every counter in LDS (lanes l and l + 32 share one)

__global__ __launch_bounds__(PT) void argmin_hist_kernel(const uint8_t* __restrict__ argmin, int32_t* __restrict__ counts,
                                                         uint32_t n_px) {
  __shared__ uint32_t hist[BBD_MAX_CAND][HC];
  const int b = blockIdx.y, tid = threadIdx.x, copy = tid & (HC - 1);
  for (int i = tid; i < BBD_MAX_CAND * HC; i += PT) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const uint8_t* p = argmin + (size_t)b * n_px;
  // aligned 4-byte words in the middle, the (at most 3 + 3) bytes around them one by one
  const uint32_t head0 = (uint32_t)((4u - ((uintptr_t)p & 3u)) & 3u), head = head0 < n_px ? head0 : n_px;
  const uint32_t nwords = (n_px - head) / 4u, tail0 = head + nwords * 4u;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(p + head);
  for (uint32_t i = blockIdx.x * PT + tid; i < nwords; i += gridDim.x * PT) {
    const uint32_t w = words[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t id = (w >> (8 * k)) & 0xffu;
      if (id < BBD_MAX_CAND) atomicAdd(&hist[id][copy], 1u);
    }
  }
  if (blockIdx.x == 0) {
    const uint32_t nrest = head + (n_px - tail0);                  // <= 6
    if ((uint32_t)tid < nrest) {
      const uint32_t id = p[(uint32_t)tid < head ? (uint32_t)tid : tail0 + ((uint32_t)tid - head)];
      if (id < BBD_MAX_CAND) atomicAdd(&hist[id][copy], 1u);
    }
  }
  __syncthreads();
  if (tid < BBD_MAX_CAND) {
    uint32_t s = 0u;
    for (int k = 0; k < HC; ++k) s += hist[tid][(k + tid) & (HC - 1)];
    if (s) atomicAdd(counts + (size_t)b * BBD_MAX_CAND + tid, (int32_t)s);
  }
}

}  // namespace

extern "C" int bbd_train_panel_scratch_ints(int n_tiles) { return n_tiles > 0 && n_tiles <= 65535 ? n_tiles * PARTS * 2 : 0; }

extern "C" int bbd_train_panel(const int32_t* desc, const float* pose, const uint8_t* lut, uint8_t* out, float* stats,
                               int32_t* scratch, int n_tiles, int NP, int H, int W, int rows, int cols, void* stream) {
  if (!desc || !pose || !lut || !out || !stats || !scratch) return BBD_E_BADARG;
  if (n_tiles < 1 || NP < 1 || H < 1 || W < 1 || rows < 1 || cols < 1) return BBD_E_BADARG;
  const long long lim = 0x7fffffffLL;
  if ((long long)H * W > lim || (long long)rows * H > lim || (long long)cols * W > lim) return BBD_E_BADARG;
  if ((long long)rows * cols > 65535 || n_tiles > 65535) return BBD_E_BADARG;
  PanelArgs a;
  a.desc = desc; a.pose = pose; a.lut = lut; a.out = out; a.stats = stats;
  a.scratch = reinterpret_cast<uint32_t*>(scratch);
  a.n_tiles = n_tiles; a.NP = NP; a.rows = rows; a.cols = cols;
  a.dm = bbd_dims(H, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(panel_extrema_kernel, dim3(PARTS, (unsigned)n_tiles), dim3(PT), 0, st, a);
  const unsigned ngroups = (unsigned)H * (((unsigned)W + 3u) / 4u);
  const unsigned gx = (ngroups + PT - 1) / PT;
  hipLaunchKernelGGL(panel_render_kernel, dim3(gx < (unsigned)MAX_GX ? gx : (unsigned)MAX_GX, (unsigned)(rows * cols)), dim3(PT),
                     0, st, a);
  return launch_status();
}

extern "C" int bbd_argmin_hist(const uint8_t* argmin, int32_t* counts, int B, int n_px, void* stream) {
  if (!argmin || !counts || B < 1 || B > 65535 || n_px < 1) return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * BBD_MAX_CAND * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  const unsigned per = PT * 4 * 8;                                // pixels a workgroup takes per round, eight rounds
  unsigned gx = ((unsigned)n_px + per - 1) / per;
  gx = gx < 1u ? 1u : (gx > 256u ? 256u : gx);
  hipLaunchKernelGGL(argmin_hist_kernel, dim3(gx, (unsigned)B), dim3(PT), 0, st, argmin, counts, (uint32_t)n_px);
  return launch_status();
}
