// bbd_stemconv.hip - the encoder stems' conv1 (7x7, stride 2, pad 3, C = 3 or 6 -> 64, no bias) and its weight
// gradient on v_mfma_f32_16x16x4_f32, straight from the NCHW tensors (include/bbd_hip.h, bbd_stem_conv7s2_*; the index
// arithmetic, the LDS tile and the layout of a scratch record: bbd_stemconv_math.h).
//
// Both launches stage a tile of the input in LDS with its zero border written out and with even and odd columns in two
// planes, so that the inner loops carry no bounds test and the stride-2 reads of neighbouring pixels are neighbouring
// words.  `normalize` applies the encoder's (x - 0.45) / 0.225 on the way into LDS, as bbd_gather_pairs evaluates it:
// subtract, then multiply by the float reciprocal (the border stays zero: it pads the normalised image).
//
// Forward: a workgroup per tile of 8 x 32 output pixels; wave kb holds the weights of its 16 output channels in
// registers (14 C of them) and reads one word of LDS per MFMA at an immediate offset.  Four accumulator tiles (two rows
// x two groups of 16 pixels) are in flight; the taps of one input channel are one fma chain, and the C chains are added
// in fp32 (a shorter chain carries less rounding error than one over all C * 49 taps).
//
// Weight gradient: 8 waves, each with its own block of 16 output channels and its own half of the C * 49 patch columns;
// a workgroup walks neighbouring tiles.  The MFMA is an exact fp32 fma chain, so an accumulator that has taken
// BBD_WGRAD_RUN products is added to the lane's own double; the workgroup's doubles go to `scratch` and a second launch
// adds the workgroups in a fixed order.  No atomics, no zero-fill: equal bits from call to call.
#include <hip/hip_runtime.h>

#include "../../include/bbd_hip.h"
#include "../../include/bbd_stemconv.h"
#include "bbd_stemconv_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static_assert(BBD_STEM_RUN_STRIPS * 16 == BBD_WGRAD_RUN, "an fp32 run is BBD_WGRAD_RUN products");
static_assert(BBD_STEM_PW >= BBD_STEM_TW + 3 && BBD_STEM_PITCH >= 2 * BBD_STEM_TW + 6, "the planes hold every tap's word");
static_assert(BBD_STEM_STRIPS % BBD_STEM_RUN_STRIPS == 0 && BBD_STEM_TW == 32 && BBD_STEM_TH % 2 == 0, "tile");

constexpr float NORM_SUB = 0.45f, NORM_MUL = 1.0f / 0.225f;

int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };     // four floats at float alignment

// A thread's share of part `part` of the PARTS parts of a tile: every load is issued before the first value is used, so a
// part costs one trip to memory, and the values can wait in registers while the tile before is still being read.
template <int C, int THREADS, int PARTS>
struct TileRegs {
  static constexpr int WORDS = C * BBD_STEM_ROWS * BBD_STEM_PITCH, PER = (WORDS + THREADS * PARTS - 1) / (THREADS * PARTS);
  float v[PER];

  __device__ __forceinline__ void load(const float* __restrict__ x, const bbd_stem_plan& p, const bbd_stem_tile& t,
                                       int normalize, int part = 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + (part * PER + i) * THREADS;
      int c, ly, lx;
      bbd_stem_fill_decode(e < WORDS ? e : 0, &c, &ly, &lx);
      const long from = bbd_stem_fill_src(&p, &t, c, ly, lx);
      const float raw = x[from >= 0 ? from : 0];                // (element 0 exists: the load needs no branch)
      const float val = normalize ? (raw - NORM_SUB) * NORM_MUL : raw;
      v[i] = from >= 0 ? val : 0.f;
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ tile, int part = 0) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + (part * PER + i) * THREADS;
      int c, ly, lx;
      bbd_stem_fill_decode(e, &c, &ly, &lx);
      if (e < WORDS) tile[bbd_stem_lds_index(c, ly, lx)] = v[i];
    }
  }
};

// ------------------------------------------------------------------------------------------------------------ forward
template <int C>
__global__ __launch_bounds__(BBD_STEM_FWD_WAVES * 64) void stem_fwd_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ w,
                                                                          float* __restrict__ out, bbd_stem_plan p,
                                                                          int normalize) {
  __shared__ float tile[C * BBD_STEM_ROWS * BBD_STEM_PITCH];
  const int lane = threadIdx.x & 63;
  const int kb = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bbd_stem_tile t = bbd_stem_decode(&p, blockIdx.x);

  float wr[C][7][2];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const int at = bbd_stem_fwd_w_index(C, kb, lane, c, r, par);
        wr[c][r][par] = at >= 0 ? w[at] : 0.f;
      }

  TileRegs<C, BBD_STEM_FWD_WAVES * 64, 4> staged;
#pragma unroll 1
  for (int part = 0; part < 4; ++part) {
    staged.load(x, p, t, normalize, part);
    staged.store(tile, part);
  }
  __syncthreads();

  const float* mine = tile + bbd_stem_fwd_b_lane(lane);
  const int ox = t.ox0 + (lane & 15);
#pragma unroll 1
  for (int pair = 0; pair < BBD_STEM_TH / 2; ++pair) {
    const int oyl = 2 * pair;
    if (t.oy0 + oyl >= p.Ho) break;
    f32x4 acc[2][2];                                 // the sum over the input channels of ...
    const float* rows = mine + bbd_stem_fwd_b_tap(0, 0, 0, oyl, 0);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      f32x4 chain[2][2];                             // ... one fma chain over the taps of a channel
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g = 0; g < 2; ++g) chain[a][g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              const float b = rows[bbd_stem_fwd_b_tap(c, r, par, a, g)];
              chain[a][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[c][r][par], b, chain[a][g], 0, 0, 0);
            }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[a][g] = c ? acc[a][g] + chain[a][g] : chain[a][g];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int oy = t.oy0 + oyl + a;
      if (oy >= p.Ho) continue;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (ox + 16 * g >= p.Wo) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          out[bbd_stem_out_offset(&p, t.n, kb * 16 + 4 * (lane >> 4) + reg, oy, ox + 16 * g)] = acc[a][g][reg];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- weight gradient
__device__ __forceinline__ void load_go(float (&g)[4], const float* __restrict__ go, const bbd_stem_plan& p,
                                        const bbd_stem_tile& t, int st, int kb, int lane) {
  const int pixels = bbd_stem_go_pixels(&p, &t, st, lane);
  const float* src = go + bbd_stem_go_offset(&p, &t, st, kb, lane);
  if (pixels == 4) {
    const F4U v = *reinterpret_cast<const F4U*>(src);
    g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = j < pixels ? src[j] : 0.f;
  }
}

template <int C, int NCT>
__global__ __launch_bounds__(BBD_STEM_WGRAD_WAVES * 64) void stem_wgrad_kernel(const float* __restrict__ x,
                                                                              const float* __restrict__ go,
                                                                              double* __restrict__ scratch,
                                                                              bbd_stem_plan p, int normalize) {
  __shared__ float tile[C * BBD_STEM_ROWS * BBD_STEM_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kb = wave & 3;

  int b_lane[NCT];
  f32x4 acc[NCT];
  double total[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    b_lane[ct] = bbd_stem_wgrad_b_lane(&p, bbd_stem_wave_ctile(&p, wave, ct), lane);
    acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) total[ct][reg] = 0.0;
  }

  int first, last;
  bbd_stem_group_range(&p, blockIdx.x, &first, &last);
  TileRegs<C, BBD_STEM_WGRAD_WAVES * 64, 1> staged;
  if (first < last) staged.load(x, p, bbd_stem_decode(&p, first), normalize);
  for (int id = first; id < last; ++id) {
    const bbd_stem_tile t = bbd_stem_decode(&p, id);
    __syncthreads();                                 // the tile before has been read
    staged.store(tile);
    float cur[4], nxt[4];
    load_go(cur, go, p, t, 0, kb, lane);
    __syncthreads();
    if (id + 1 < last) staged.load(x, p, bbd_stem_decode(&p, id + 1), normalize);    // in flight under this tile's MFMAs
#pragma unroll 1
    for (int st = 0; st < BBD_STEM_STRIPS; ++st) {
      if (st + 1 < BBD_STEM_STRIPS) load_go(nxt, go, p, t, st + 1, kb, lane);
      // (a pixel outside the image: grad_out 0 times a word of the tile, which is finite)
      const float* strip = tile + bbd_stem_wgrad_b_strip(st);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        if (bbd_stem_wave_ctile(&p, wave, ct) >= p.ctiles) continue;          // one value per wave
        const float* b = strip + b_lane[ct];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[j], b[j], acc[ct], 0, 0, 0);
      }
      if ((st + 1) % BBD_STEM_RUN_STRIPS == 0) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) total[ct][reg] += (double)acc[ct][reg];
          acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
  }
  double* rec = scratch + bbd_stem_record_offset(&p, blockIdx.x);
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) rec[bbd_stem_record_index(&p, wave, ct, lane, reg)] = total[ct][reg];
}

// Workgroup b: the BBD_STEM_FINAL_E record elements from b * 16 on.  Thread (slice, e) adds the groups slice, slice +
// 16, ... in that order, then thread e adds the 16 slices in order.
__global__ __launch_bounds__(BBD_STEM_FINAL_E * BBD_STEM_FINAL_G) void stem_wgrad_final_kernel(
    const double* __restrict__ scratch, float* __restrict__ gw, bbd_stem_plan p) {
  __shared__ double part[BBD_STEM_FINAL_G][BBD_STEM_FINAL_E];
  const int e16 = threadIdx.x & (BBD_STEM_FINAL_E - 1), slice = threadIdx.x / BBD_STEM_FINAL_E;
  const int e = blockIdx.x * BBD_STEM_FINAL_E + e16;
  double v = 0.0;
  for (int g = slice; g < p.groups; g += BBD_STEM_FINAL_G) v += scratch[bbd_stem_record_offset(&p, g) + e];
  part[slice][e16] = v;
  __syncthreads();
  if (slice == 0) {
    double sum = 0.0;
    for (int q = 0; q < BBD_STEM_FINAL_G; ++q) sum += part[q][e16];
    const int at = bbd_stem_record_to_weight(&p, e);
    if (at >= 0) gw[at] = (float)sum;
  }
}

}  // namespace

extern "C" {

int bbd_stem_conv7s2_supported(int N, int C, int K, int H, int W, int R, int S) {
  bbd_stem_plan p;
  return bbd_stem_make_plan(N, C, K, H, W, R, S, &p);
}

int bbd_stem_conv7s2_wgrad_scratch_doubles(int N, int C, int K, int H, int W, int R, int S) {
  bbd_stem_plan p;
  return bbd_stem_make_plan(N, C, K, H, W, R, S, &p) ? bbd_stem_plan_scratch_doubles(&p) : 0;
}

int bbd_stem_conv7s2_fwd(const float* x, const float* w, float* out, int N, int C, int K, int H, int W, int normalize,
                         void* stream) {
  bbd_stem_plan p;
  if (!x || !w || !out || !bbd_stem_make_plan(N, C, K, H, W, 7, 7, &p)) return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)p.tiles), block(BBD_STEM_FWD_WAVES * 64);
  if (C == 3) hipLaunchKernelGGL(stem_fwd_kernel<3>, grid, block, 0, st, x, w, out, p, normalize);
  else hipLaunchKernelGGL(stem_fwd_kernel<6>, grid, block, 0, st, x, w, out, p, normalize);
  return status();
}

int bbd_stem_conv7s2_wgrad(const float* x, const float* grad_out, float* grad_w, double* scratch, int scratch_doubles,
                           int N, int C, int K, int H, int W, int normalize, void* stream) {
  bbd_stem_plan p;
  if (!x || !grad_out || !grad_w || !scratch || !bbd_stem_make_plan(N, C, K, H, W, 7, 7, &p) ||
      scratch_doubles < bbd_stem_plan_scratch_doubles(&p))
    return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)p.groups), block(BBD_STEM_WGRAD_WAVES * 64);
  if (C == 3) hipLaunchKernelGGL((stem_wgrad_kernel<3, 5>), grid, block, 0, st, x, grad_out, scratch, p, normalize);
  else hipLaunchKernelGGL((stem_wgrad_kernel<6, 10>), grid, block, 0, st, x, grad_out, scratch, p, normalize);
  hipLaunchKernelGGL(stem_wgrad_final_kernel, dim3((unsigned)(p.record / BBD_STEM_FINAL_E)),
                     dim3(BBD_STEM_FINAL_E * BBD_STEM_FINAL_G), 0, st, scratch, grad_w, p);
  return status();
}

}  // extern "C"
