// bbd_viz.hip - colour-mapped disparity of single-image prediction on the device (test_simple.py:135-148).
//
// The reference upsamples the network's disparity to the original image size, copies it to the host, sorts it for
// np.percentile(., 95), normalises with matplotlib and looks the magma colours up in float64 - per image.  Here the
// upsampled map is never materialised (unless the caller asks for it): four launches over (tile, image) workgroups
// recompute the scaled disparity s on the fly from the L2-resident h x w network output.
//
//   sweep 0  histogram of the top 11 bits of the order key of s; minimum of s (atomic max on the inverted key)
//   sweep 1  every workgroup resolves level 0 itself from the image's 2048-bin histogram (two ranks: the order
//            statistics that bracket numpy's virtual index), then histograms the next 11 bits under those prefixes
//   sweep 2  resolves levels 0-1, histograms the last 10 bits
//   colour   resolves levels 0-2 -> both order statistics exactly, vmax by numpy's float32 interpolation, then
//            normalise, LUT, packed u8 stores (and s itself when out_float is given)
//
// Histograms are integer counts (LDS atomics per workgroup, then one pass of global vector atomics over the non-empty
// bins), so every result is independent of launch geometry and of the order the atomics land in.  Nothing spins on
// another workgroup and nothing synchronises with the host: the stream orders the sweeps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h"
#include "bbd_viz_math.h"
#include "bbd_device_util.h"

namespace {

constexpr int VT = 256;              // threads per workgroup
constexpr int VW = VT / 64;          // waves
constexpr int VTILES = 256;          // workgroups per image (one per CU of an MI355X)
constexpr int NBIN = 2048;
// per-image scratch (uint32): level 0 | level 1 lower, upper | level 2 lower, upper | inverted minimum key + padding
constexpr int SC_L0 = 0, SC_L1 = NBIN, SC_L2 = 3 * NBIN, SC_MIN = 5 * NBIN, SC_STRIDE = 5 * NBIN + 64;

struct VizArgs {
  const float* disp;       // [n,h,w]
  const int32_t* desc;     // [n, BBD_VIZ_DESC] pixel offset lo, hi | H0 | W0
  const uint8_t* lut;      // [256,3]
  uint8_t* out_u8;         // image i at out_u8 + 3 * offset_i
  float* out_float;        // image i at out_float + offset_i, or NULL
  float* stats;            // [n,4] vmin, vmax, lower, upper order statistic
  uint32_t* scratch;       // [n, SC_STRIDE], zero on entry of sweep 0
  int h, w;
  float lo, span, q;
};

struct Image {
  size_t off;
  int H0, W0;
  uint32_t npx;
  const float* src;
};

__device__ __forceinline__ Image load_image(const VizArgs& a, int img) {
  const int32_t* d = a.desc + (size_t)img * BBD_VIZ_DESC;
  Image im;
  im.off = bbd_join64(d[0], d[1]);
  im.H0 = d[2];
  im.W0 = d[3];
  im.npx = (uint32_t)im.H0 * (uint32_t)im.W0;
  im.src = a.disp + (size_t)img * a.h * a.w;
  return im;
}

// F.interpolate(disp, (H0, W0), bilinear, align_corners=False) at (y, x), then layers.disp_to_depth's scaling.
__device__ __forceinline__ float scaled_at(const VizArgs& a, const Image& im, int y, int x) {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  bbd_viz_up_src(y, a.h, im.H0, &y0, &y1, &ly0, &ly1);
  bbd_viz_up_src(x, a.w, im.W0, &x0, &x1, &lx0, &lx1);
  const float* r0 = im.src + (size_t)y0 * a.w;
  const float* r1 = im.src + (size_t)y1 * a.w;
  const float d = bbd_up_blend(r0[x0], r0[x1], r1[x0], r1[x1], ly0, ly1, lx0, lx1, im.H0 + im.W0 <= 128);
  return bbd_viz_scaled(d, a.lo, a.span);
}

// Bin of `hist[0..NBIN)` that holds rank `rank` (0-based, rank < total) and the rank inside that bin; every thread of
// the workgroup returns the same pair.  `sh` is 2 + VW words of LDS.
__device__ __forceinline__ void resolve(const uint32_t* hist, uint32_t rank, uint32_t* sh, uint32_t* bin, uint32_t* within) {
  constexpr int PER = NBIN / VT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t c[PER], mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = hist[tid * PER + j];
    mine += c[j];
  }
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                       // previous use of sh is over
  if (lane == 63) sh[2 + wave] = incl;
  __syncthreads();
  uint32_t base = 0;
  for (int wv = 0; wv < wave; ++wv) base += sh[2 + wv];
  const uint32_t before = base + incl - mine;
  if (rank >= before && rank < before + mine) {      // exactly one thread
    uint32_t cum2 = before;
    int bb = 0;
    for (; bb < PER - 1; ++bb) {                     // stops at the first bin with rank < cum2 + c[bb]
      if (rank < cum2 + c[bb]) break;
      cum2 += c[bb];
    }
    sh[0] = (uint32_t)(tid * PER + bb);
    sh[1] = rank - cum2;
  }
  __syncthreads();
  *bin = sh[0];
  *within = sh[1];
}

struct Select {
  uint32_t prefix[2];   // key bits resolved so far, lower / upper order statistic
  uint32_t rank[2];     // rank inside the bins of `prefix`
  float gamma;
};

// Resolves `levels` (0..3) levels of the radix select for both order statistics.
__device__ __forceinline__ Select resolve_levels(const VizArgs& a, const Image& im, const uint32_t* sc, int levels,
                                                 uint32_t* sh) {
  Select s;
  bbd_viz_ranks(im.npx, a.q, &s.rank[0], &s.rank[1], &s.gamma);
  s.prefix[0] = s.prefix[1] = 0u;
  for (int level = 0; level < levels; ++level) {
    for (int k = 0; k < 2; ++k) {
      const uint32_t* hist = sc + (level == 0 ? SC_L0 : (level == 1 ? SC_L1 : SC_L2) + k * NBIN);
      uint32_t bin, within;
      resolve(hist, s.rank[k], sh, &bin, &within);
      s.prefix[k] = level == 0 ? bin : ((s.prefix[k] << (level == 2 ? 10 : 11)) | bin);
      s.rank[k] = within;
    }
  }
  return s;
}

template <int LEVEL>
__global__ __launch_bounds__(VT) void viz_hist_kernel(VizArgs a) {
  __shared__ uint32_t hist[2][NBIN];
  __shared__ uint32_t sh[2 + VW];
  const int img = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const Image im = load_image(a, img);
  uint32_t* sc = a.scratch + (size_t)img * SC_STRIDE;
  if ((uint64_t)tile * VT >= im.npx) return;            // uniform: this workgroup owns no pixel

  Select sel;
  if (LEVEL > 0) sel = resolve_levels(a, im, sc, LEVEL, sh);
  for (int i = tid; i < 2 * NBIN; i += VT) (&hist[0][0])[i] = 0u;
  __syncthreads();

  constexpr int shift = LEVEL == 0 ? 21 : (LEVEL == 1 ? 10 : 0);
  constexpr int prev_shift = LEVEL == 1 ? 21 : 10;
  constexpr uint32_t mask = LEVEL == 2 ? 1023u : 2047u;
  uint32_t inv_min = 0u;
  for (uint32_t i = (uint32_t)tile * VT + tid; i < im.npx; i += (uint32_t)VTILES * VT) {
    const int y = (int)(i / (uint32_t)im.W0), x = (int)(i - (uint32_t)y * (uint32_t)im.W0);
    const uint32_t key = bbd_viz_order_key(scaled_at(a, im, y, x));
    if (LEVEL == 0) {
      atomicAdd(&hist[0][key >> 21], 1u);
      inv_min = max(inv_min, ~key);
    } else {
      if ((key >> prev_shift) == sel.prefix[0]) atomicAdd(&hist[0][(key >> shift) & mask], 1u);
      if ((key >> prev_shift) == sel.prefix[1]) atomicAdd(&hist[1][(key >> shift) & mask], 1u);
    }
  }
  __syncthreads();
  uint32_t* g = sc + (LEVEL == 0 ? SC_L0 : (LEVEL == 1 ? SC_L1 : SC_L2));
  for (int i = tid; i < (LEVEL == 0 ? NBIN : 2 * NBIN); i += VT) {
    const uint32_t c = (&hist[0][0])[i];
    if (c) atomicAdd(g + i, c);
  }
  if (LEVEL == 0) {
    inv_min = wave_max(inv_min);
    if ((tid & 63) == 0) atomicMax(sc + SC_MIN, inv_min);
  }
}

__device__ __forceinline__ uint32_t colour_of(const VizArgs& a, const Image& im, const uint32_t* lut, float* outf,
                                              uint32_t i, int y, int x, float vmin, float vmax) {
  const float s = scaled_at(a, im, y, x);
  if (outf) outf[i] = s;
  return lut[bbd_viz_lut_index(s, vmin, vmax)];
}

__global__ __launch_bounds__(VT) void viz_colour_kernel(VizArgs a) {
  __shared__ uint32_t sh[2 + VW];
  __shared__ uint32_t lut[256];                          // r | g << 8 | b << 16
  const int img = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const Image im = load_image(a, img);
  const uint32_t* sc = a.scratch + (size_t)img * SC_STRIDE;
  const uint32_t nquad = (im.npx + 3u) / 4u;
  if ((uint64_t)tile * VT >= nquad) return;
  fill_lut<256, VT>(lut, a.lut);                         // published by the barriers of resolve_levels

  const Select sel = resolve_levels(a, im, sc, 3, sh);
  const float lower = bbd_viz_key_value(sel.prefix[0]), upper = bbd_viz_key_value(sel.prefix[1]);
  const float vmax = bbd_viz_lerp(lower, upper, sel.gamma);
  const float vmin = bbd_viz_key_value(~sc[SC_MIN]);
  if (tile == 0 && tid == 0) {
    float* st = a.stats + (size_t)img * 4;
    st[0] = vmin; st[1] = vmax; st[2] = lower; st[3] = upper;
  }
  uint8_t* out = a.out_u8 + 3 * im.off;
  float* outf = a.out_float ? a.out_float + im.off : nullptr;
  const bool packed = (((uintptr_t)out) & 3u) == 0;
  for (uint32_t qd = (uint32_t)tile * VT + tid; qd < nquad; qd += (uint32_t)VTILES * VT) {
    const uint32_t i0 = qd * 4u;
    int y = (int)(i0 / (uint32_t)im.W0), x = (int)(i0 - (uint32_t)y * (uint32_t)im.W0);
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    const uint32_t cnt = im.npx - i0 < 4u ? im.npx - i0 : 4u;
    for (uint32_t k = 0; k < cnt; ++k) {
      c[k] = colour_of(a, im, lut, outf, i0 + k, y, x, vmin, vmax);
      if (++x == im.W0) { x = 0; ++y; }
    }
    store_quad(out + (size_t)i0 * 3, packed, cnt, c);
  }
}

}  // namespace

extern "C" int bbd_disp_viz_scratch_ints(int n) { return n > 0 ? n * SC_STRIDE : 0; }

extern "C" int bbd_disp_viz(const float* disp, const int32_t* desc, const uint8_t* lut, uint8_t* out_u8, float* out_float,
                            float* stats, int32_t* scratch, int n, int h, int w, double min_disp, double max_disp,
                            double percentile, void* stream) {
  if (!disp || !desc || !lut || !out_u8 || !stats || !scratch || n <= 0 || n > 65535 || h < 1 || w < 1) return BBD_E_BADARG;
  if (!(percentile > 0.0 && percentile <= 100.0)) return BBD_E_BADARG;
  VizArgs a;
  a.disp = disp; a.desc = desc; a.lut = lut; a.out_u8 = out_u8; a.out_float = out_float; a.stats = stats;
  a.scratch = reinterpret_cast<uint32_t*>(scratch); a.h = h; a.w = w;
  a.lo = (float)min_disp; a.span = (float)(max_disp - min_disp);      // Python doubles meeting an fp32 tensor
  a.q = bbd_viz_quantile(percentile);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(scratch, 0, (size_t)n * SC_STRIDE * sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(VTILES, (unsigned)n), block(VT);
  hipLaunchKernelGGL(viz_hist_kernel<0>, grid, block, 0, st, a);
  hipLaunchKernelGGL(viz_hist_kernel<1>, grid, block, 0, st, a);
  hipLaunchKernelGGL(viz_hist_kernel<2>, grid, block, 0, st, a);
  hipLaunchKernelGGL(viz_colour_kernel, grid, block, 0, st, a);
  return launch_status();
}
