// bbd_compare.hip - the two pictures of the checkpoint comparison sheets that had no kernel (validation.py): the
// colour-mapped ground truth (validation.py:250-254) and a per-pixel error map of one model against it.
//
// Both work on a ragged batch described by BBD_EVAL_DESC rows (the rows evaluation.GroundTruthSet keeps): picture i is
// written at 3x the element offset of map i, so the maps' packing is the pictures' packing.
//
//   bbd_gt_viz     launch 1  per map, PARTS workgroups each reduce a strided share of v = 1 / g (cut at max_inv) to
//                            (minimum, maximum) as order keys (NaNs skipped) and store the pair in scratch - plain
//                            stores, nothing to zero, no atomics
//                  launch 2  combines the PARTS pairs, colours four pixels per thread (12-byte packed stores where the
//                            picture starts on a 4-byte boundary, bytes otherwise)
//   bbd_error_map  one launch: every output pixel GATHERS the maximum abs_rel summand of the valid ground-truth pixels
//                  within `radius` (at most 81 taps of an L2-resident sparse map; the prediction is resampled only at
//                  the valid ones, ~5 % of a LiDAR map), so nothing scatters and nothing depends on order
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_viz_math.h"
#include "bbd_panel_math.h"
#include "bbd_compare_math.h"
#include "bbd_device_util.h"

namespace {

constexpr int CT = 256;              // threads per workgroup
constexpr int PARTS = BBD_EXTREMA_PARTS;   // partial extrema per map
constexpr int CTILES = 128;          // workgroups per map in the colouring launches (grid-stride beyond)

struct Map : BbdEvalRow {
  uint32_t npx;
};

__device__ __forceinline__ Map load_map(const int32_t* desc, int i) {
  Map m;
  static_cast<BbdEvalRow&>(m) = bbd_eval_row(desc, i);
  m.npx = m.GH > 0 && m.GW > 0 ? (uint32_t)m.GH * (uint32_t)m.GW : 0u;
  return m;
}

struct GtArgs {
  const float* gt;
  const int32_t* desc;     // [n, BBD_EVAL_DESC]
  const uint8_t* lut;      // [256,3]
  uint8_t* out;            // picture i at out + 3 * offset_i
  float* stats;            // [n,2] vmin, vmax
  uint32_t* scratch;       // [n, PARTS, 2]  ~minimum key, maximum key
  float max_inv;
};

__global__ __launch_bounds__(CT) void gt_extrema_kernel(GtArgs a) {
  const int img = blockIdx.y;
  const Map m = load_map(a.desc, img);
  const float* gt = a.gt + m.off;
  extrema_part<CT>(m.npx, [&](uint32_t i) { return bbd_compare_gt_inverse(gt[i], a.max_inv); },
                   a.scratch + ((size_t)img * PARTS + blockIdx.x) * 2);
}

__global__ __launch_bounds__(CT) void gt_colour_kernel(GtArgs a) {
  __shared__ uint32_t lut[256];
  const int img = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const Map m = load_map(a.desc, img);
  const uint32_t nquad = (m.npx + 3u) / 4u;
  if (tile > 0 && (uint64_t)tile * CT >= nquad) return;      // uniform: no pixel here (tile 0 still writes the stats)
  stage_lut<256, CT>(lut, a.lut);
  float vmin, vmax;
  extrema_combine(a.scratch + (size_t)img * PARTS * 2, &vmin, &vmax);
  if (tile == 0 && tid == 0) { a.stats[(size_t)img * 2] = vmin; a.stats[(size_t)img * 2 + 1] = vmax; }
  const float* gt = a.gt + m.off;
  uint8_t* out = a.out + 3 * m.off;
  const bool packed = (((uintptr_t)out) & 3u) == 0;
  for (uint32_t qd = (uint32_t)tile * CT + tid; qd < nquad; qd += (uint32_t)CTILES * CT) {
    const uint32_t i0 = qd * 4u, cnt = m.npx - i0 < 4u ? m.npx - i0 : 4u;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < cnt; ++k)
      c[k] = lut[bbd_viz_lut_index(bbd_compare_gt_inverse(gt[i0 + k], a.max_inv), vmin, vmax)];
    store_quad(out + (size_t)i0 * 3, packed, cnt, c);
  }
}

struct ErrArgs {
  const float* pred;       // [n,h,w] scaled disparity
  const float* gt;
  const int32_t* desc;     // [n, BBD_EVAL_DESC]
  const float* rows;       // [n, BBD_EVAL_OUT] of bbd_depth_metrics
  const uint8_t* images;   // picture i (uint8 HWC, ground-truth size) at images + 3 * offset_i, or NULL
  const uint8_t* lut;
  uint8_t* out;            // picture i at out + 3 * offset_i
  float* out_float;        // plane i at out_float + offset_i, or NULL
  int h, w, radius, flags;
  float min_depth, max_depth, scale_factor, err_max;
};

__global__ __launch_bounds__(CT) void error_map_kernel(ErrArgs a) {
  __shared__ uint32_t lut[256];
  const int img = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const Map m = load_map(a.desc, img);
  const uint32_t nquad = (m.npx + 3u) / 4u;
  if ((uint64_t)tile * CT >= nquad) return;                  // uniform
  stage_lut<256, CT>(lut, a.lut);
  const float* row = a.rows + (size_t)img * BBD_EVAL_OUT;
  const bool scored = row[10] != 0.0f;                       // count == 0: nothing was scored, all background
  BbdCompareMap cm;
  cm.gt = a.gt + m.off;
  cm.pred = a.pred + (size_t)img * a.h * a.w;
  cm.GH = m.GH; cm.GW = m.GW; cm.r0 = m.r0; cm.r1 = m.r1; cm.c0 = m.c0; cm.c1 = m.c1; cm.h = a.h; cm.w = a.w;
  cm.min_depth = a.min_depth; cm.max_depth = a.max_depth; cm.scale_factor = a.scale_factor; cm.ratio = row[7];
  cm.flags = a.flags; cm.radius = a.radius;
  const uint8_t* pic = a.images ? a.images + 3 * m.off : nullptr;
  uint8_t* out = a.out + 3 * m.off;
  float* outf = a.out_float ? a.out_float + m.off : nullptr;
  const bool packed = (((uintptr_t)out) & 3u) == 0;
  for (uint32_t qd = (uint32_t)tile * CT + tid; qd < nquad; qd += (uint32_t)CTILES * CT) {
    const uint32_t i0 = qd * 4u, cnt = m.npx - i0 < 4u ? m.npx - i0 : 4u;
    int y = (int)(i0 / (uint32_t)m.GW), x = (int)(i0 - (uint32_t)y * (uint32_t)m.GW);
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint32_t i = i0 + k;
      float e = 0.0f, own = 0.0f;
      const bool any = scored && bbd_compare_error_max(cm, y, x, &e);
      if (outf) {
        const bool valid = scored && bbd_compare_error_at(cm, y, x, &own);
        outf[i] = valid ? own : bbd_viz_bits_float(BBD_COMPARE_NAN_BITS);
      }
      if (any) c[k] = lut[bbd_viz_lut_index(e, 0.0f, a.err_max)];
      else if (pic) c[k] = bbd_compare_grey(pic + (size_t)i * 3);
      if (++x == m.GW) { x = 0; ++y; }
    }
    store_quad(out + (size_t)i0 * 3, packed, cnt, c);
  }
}

}  // namespace

extern "C" int bbd_gt_viz_scratch_ints(int n) { return n > 0 && n <= 65535 ? n * PARTS * 2 : 0; }

extern "C" int bbd_gt_viz(const float* gt, const int32_t* desc, const uint8_t* lut, uint8_t* out_u8, float* stats,
                          int32_t* scratch, int n, double max_inv, void* stream) {
  if (!gt || !desc || !lut || !out_u8 || !stats || !scratch || n < 1 || n > 65535) return BBD_E_BADARG;
  GtArgs a;
  a.gt = gt; a.desc = desc; a.lut = lut; a.out = out_u8; a.stats = stats;
  a.scratch = reinterpret_cast<uint32_t*>(scratch); a.max_inv = (float)max_inv;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gt_extrema_kernel, dim3(PARTS, (unsigned)n), dim3(CT), 0, st, a);
  hipLaunchKernelGGL(gt_colour_kernel, dim3(CTILES, (unsigned)n), dim3(CT), 0, st, a);
  return launch_status();
}

extern "C" int bbd_error_map(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                             const uint8_t* images, const uint8_t* lut, uint8_t* out_u8, float* out_float, int n, int h,
                             int w, double min_depth, double max_depth, double scale_factor, double err_max, int radius,
                             int flags, void* stream) {
  if (!pred || !gt || !desc || !rows || !lut || !out_u8 || n < 1 || n > 65535 || h < 1 || w < 1) return BBD_E_BADARG;
  if (radius < 0 || radius > BBD_ERROR_MAP_MAX_RADIUS || (flags & ~BBD_EVAL_NO_MEDIAN_SCALING)) return BBD_E_BADARG;
  ErrArgs a;
  a.pred = pred; a.gt = gt; a.desc = desc; a.rows = rows; a.images = images; a.lut = lut; a.out = out_u8;
  a.out_float = out_float; a.h = h; a.w = w; a.radius = radius; a.flags = flags;
  a.min_depth = (float)min_depth; a.max_depth = (float)max_depth; a.scale_factor = (float)scale_factor;
  a.err_max = (float)err_max;
  hipLaunchKernelGGL(error_map_kernel, dim3(CTILES, (unsigned)n), dim3(CT), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}
