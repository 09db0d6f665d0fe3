// bbd_conv1x1.hip - the ResNet shortcut convolution (1x1, stride 2, no padding, no bias; layer{2,3,4}.0.downsample.0 of
// both encoders) in its three directions on v_mfma_f32_16x16x4_f32, straight from the NCHW tensors (include/bbd_hip.h,
// bbd_conv1x1s2_*; the index arithmetic, the LDS tile and the layout of a scratch record: bbd_conv1x1_math.h).
//
// A 1x1 convolution in NCHW is a GEMM per sample with the pixels contiguous, so there is no layout to change: output
// pixels are numbered flat over the batch and every launch cuts that one range.
//
// Forward: a workgroup per tile of 64 pixels and 64 output channels.  The even rows of x come in 16-byte loads at
// 4-byte alignment, the odd columns are dropped on the way into LDS, an odd row is never touched.  Wave `wave` holds
// four accumulator tiles (16 channels x 16 pixels each); a lane loads 16 bytes of its weight row per four MFMAs.
// The reduction is staged BBD_C1_RC rows at a time; a round's loads (tile and weights) are issued together, one round ahead.
// Data gradient: the same GEMM with dy staged and w read transposed; plain mode writes every element of dx once - a pair
// of neighbouring pixels is one 16-byte store (v, 0, v', 0) of the even lane and one of zeros, a row below, of the odd
// lane - accumulate mode adds into the even positions of an existing tensor and touches nothing else.
// Weight gradient: no LDS; a lane loads its four pixels of two blocks of dy (16 bytes each) and of two blocks of x (32
// bytes each, every other word used), the next strip's loads in flight under this strip's 16 MFMAs.  An accumulator that
// has taken BBD_WGRAD_RUN products is added to the lane's own double; the workgroup's doubles go to `scratch` and a
// second launch adds the records in a fixed order.  No atomics, no zero-fill: equal bits from call to call.
#include <hip/hip_runtime.h>

#include "../../include/bbd_conv1x1.h"
#include "../../include/bbd_hip.h"
#include "bbd_conv1x1_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static_assert(BBD_C1_RUN_STRIPS * 16 == BBD_WGRAD_RUN, "an fp32 run is BBD_WGRAD_RUN products");
static_assert(BBD_C1_PITCH % 16 == 4 && BBD_C1_PITCH >= BBD_C1_TP && BBD_C1_TP == 64 && BBD_C1_RC % 16 == 0, "tile");
static_assert(BBD_C1_WAVES == 4, "four waves: 64 channels, or 2 x 2 wave tiles of 32 x 32");

constexpr int THREADS = BBD_C1_WAVES * 64;

int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };     // four floats at float alignment

// ------------------------------------------------------------------------------------------------------------ forward
constexpr int STEPS = BBD_C1_RC / 16;                // MFMA steps of 16 reduction rows in a round

__global__ __launch_bounds__(THREADS) void conv1x1s2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                float* __restrict__ y, bbd_c1_plan p) {
  __shared__ __attribute__((aligned(16))) float tile[BBD_C1_RC * BBD_C1_PITCH];
  constexpr int PER = BBD_C1_RC * 32 / THREADS;      // pairs of pixels a thread stages in a round
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mb = blockIdx.y * BBD_C1_WAVES + wave;
  const bool active = mb * 16 < p.K;
  const int g0 = blockIdx.x * BBD_C1_TP;

  f32x4 acc[4];
#pragma unroll
  for (int pg = 0; pg < 4; ++pg) acc[pg] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the pair of pixels this thread stages in every channel it is dealt
  const int pr = threadIdx.x & 31, g = g0 + 2 * pr;
  const bbd_c1_pixel q0 = bbd_c1_decode(&p, g < p.pixels ? g : 0), q1 = bbd_c1_decode(&p, g + 1 < p.pixels ? g + 1 : 0);
  const bool run = bbd_c1_x_run(&p, g, &q0, 2), has0 = g < p.pixels, has1 = g + 1 < p.pixels;
  const float* mine = tile + bbd_c1_b_lane(lane);

  // A round's loads - the thread's share of the tile and the lane's weights - are all issued before the first is used, and
  // the next round's are in flight under this round's MFMAs: one trip to memory per round, hidden after the first.
  float2 staged[PER];
  float4 wr[STEPS];
  auto load = [&](int c0) {
    const int rc = bbd_c1_round_rows(p.C, c0);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int cc = (threadIdx.x >> 5) + i * (THREADS / 32);
      float v0 = 0.f, v1 = 0.f;
      if (cc < rc) {
        if (run) {
          const F4U t = *reinterpret_cast<const F4U*>(x + bbd_c1_x_offset(&p, &q0, c0 + cc));
          v0 = t.x; v1 = t.z;
        } else {
          if (has0) v0 = x[bbd_c1_x_offset(&p, &q0, c0 + cc)];
          if (has1) v1 = x[bbd_c1_x_offset(&p, &q1, c0 + cc)];
        }
      }
      staged[i] = float2{v0, v1};
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
      if (active && 16 * st < rc) wr[st] = *reinterpret_cast<const float4*>(w + bbd_c1_w_fwd(&p, mb, lane, c0, 16 * st));
  };

  load(0);
  for (int c0 = 0; c0 < p.C; c0 += BBD_C1_RC) {
    const int rc = bbd_c1_round_rows(p.C, c0);
    __syncthreads();                                 // the round before has been read
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int cc = (threadIdx.x >> 5) + i * (THREADS / 32);
      if (cc < rc) *reinterpret_cast<float2*>(tile + bbd_c1_lds_index(cc, 2 * pr)) = staged[i];
    }
    float4 wc[STEPS];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) wc[st] = wr[st];
    __syncthreads();
    if (c0 + BBD_C1_RC < p.C) load(c0 + BBD_C1_RC);
    if (active) {
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        if (16 * st >= rc) break;
        const float a[4] = {wc[st].x, wc[st].y, wc[st].z, wc[st].w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int pg = 0; pg < 4; ++pg)
            acc[pg] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], mine[bbd_c1_b_step(16 * st, j, pg)], acc[pg], 0, 0, 0);
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int pg = 0; pg < 4; ++pg) {
    const int go = bbd_c1_out_pixel(blockIdx.x, pg, lane);
    if (go >= p.pixels) continue;
    const bbd_c1_pixel q = bbd_c1_decode(&p, go);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) y[bbd_c1_y_offset(&p, &q, bbd_c1_out_channel(mb, lane, reg))] = acc[pg][reg];
  }
}

// ------------------------------------------------------------------------------------------------------ data gradient
template <bool ACCUMULATE>
__global__ __launch_bounds__(THREADS) void conv1x1s2_bwd_data_kernel(const float* __restrict__ dy,
                                                                     const float* __restrict__ w,
                                                                     float* __restrict__ dx, bbd_c1_plan p) {
  __shared__ __attribute__((aligned(16))) float tile[BBD_C1_RC * BBD_C1_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mb = blockIdx.y * BBD_C1_WAVES + wave;
  const bool active = mb * 16 < p.C;
  const int g0 = blockIdx.x * BBD_C1_TP;

  f32x4 acc[4];
#pragma unroll
  for (int pg = 0; pg < 4; ++pg) acc[pg] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the four pixels this thread stages in every row of dy it is dealt
  constexpr int PER = BBD_C1_RC * 16 / THREADS;
  const int qd = threadIdx.x & 15, g = g0 + 4 * qd;
  bbd_c1_pixel qs[4];
  bool has[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    has[j] = g + j < p.pixels;
    qs[j] = bbd_c1_decode(&p, has[j] ? g + j : 0);
  }
  const bool run = bbd_c1_y_run(&p, g, &qs[0]);
  const float* mine = tile + bbd_c1_b_lane(lane);

  // as in the forward: a round's loads are issued together, the next round's are in flight under this round's MFMAs
  float4 staged[PER];
  float wr[STEPS][4];
  auto load = [&](int k0) {
    const int rk = bbd_c1_round_rows(p.K, k0);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int kk = (threadIdx.x >> 4) + i * (THREADS / 16);
      float4 v = float4{0.f, 0.f, 0.f, 0.f};
      if (kk < rk) {
        if (run) {
          const F4U t = *reinterpret_cast<const F4U*>(dy + bbd_c1_y_offset(&p, &qs[0], k0 + kk));
          v = float4{t.x, t.y, t.z, t.w};
        } else {
          if (has[0]) v.x = dy[bbd_c1_y_offset(&p, &qs[0], k0 + kk)];
          if (has[1]) v.y = dy[bbd_c1_y_offset(&p, &qs[1], k0 + kk)];
          if (has[2]) v.z = dy[bbd_c1_y_offset(&p, &qs[2], k0 + kk)];
          if (has[3]) v.w = dy[bbd_c1_y_offset(&p, &qs[3], k0 + kk)];
        }
      }
      staged[i] = v;
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
      if (active && 16 * st < rk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) wr[st][j] = w[bbd_c1_w_bwd(&p, mb, lane, k0, 16 * st, j)];
      }
  };

  load(0);
  for (int k0 = 0; k0 < p.K; k0 += BBD_C1_RC) {
    const int rk = bbd_c1_round_rows(p.K, k0);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int kk = (threadIdx.x >> 4) + i * (THREADS / 16);
      if (kk < rk) *reinterpret_cast<float4*>(tile + bbd_c1_lds_index(kk, 4 * qd)) = staged[i];
    }
    float wc[STEPS][4];
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
      for (int j = 0; j < 4; ++j) wc[st][j] = wr[st][j];
    __syncthreads();
    if (k0 + BBD_C1_RC < p.K) load(k0 + BBD_C1_RC);
    if (active) {
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        if (16 * st >= rk) break;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int pg = 0; pg < 4; ++pg)
            acc[pg] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[st][j], mine[bbd_c1_b_step(16 * st, j, pg)], acc[pg], 0, 0, 0);
      }
    }
  }
  if (!active) return;                               // (one value per wave: the shuffles below see whole waves)
  const long plane = (long)p.H * p.W;
#pragma unroll
  for (int pg = 0; pg < 4; ++pg) {
    const int go = bbd_c1_out_pixel(blockIdx.x, pg, lane);
    const bool exists = go < p.pixels;
    const bbd_c1_pixel q = bbd_c1_decode(&p, exists ? go : 0);
    const long at = bbd_c1_x_offset(&p, &q, bbd_c1_out_channel(mb, lane, 0));
    if (ACCUMULATE) {
      if (exists) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) dx[at + reg * plane] += acc[pg][reg];
      }
      continue;
    }
    // the pair (even lane, odd lane) = pixels (go & ~1, that + 1): the even one decides for both
    const int pair_run = exists && bbd_c1_x_run(&p, go, &q, 2);
    const bool paired = __shfl(pair_run, lane & ~1) != 0;
    const bool odd = lane & 1;
    const bool col1 = 2 * q.ox + 1 < p.W, row1 = 2 * q.oy + 1 < p.H;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float v = acc[pg][reg], next = __shfl_down(v, 1);
      float* o = dx + at + reg * plane;
      if (paired) {
        if (!odd) *reinterpret_cast<F4U*>(o) = F4U{v, 0.f, next, 0.f};
        else if (row1) *reinterpret_cast<F4U*>(o + p.W - 2) = F4U{0.f, 0.f, 0.f, 0.f};   // the pair's columns, a row below
      } else if (exists) {
        o[0] = v;
        if (col1) o[1] = 0.f;
        if (row1) {
          o[p.W] = 0.f;
          if (col1) o[p.W + 1] = 0.f;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- weight gradient
struct StripRegs {
  float a[2][4], b[2][4];

  __device__ __forceinline__ void load(const float* __restrict__ x, const float* __restrict__ dy, const bbd_c1_plan& p,
                                       int strip, int lane, const int (&kb)[2], const int (&cb)[2]) {
    const int g = bbd_c1_strip_pixel(strip, lane), ch = lane & 15;
    bbd_c1_pixel qs[4];
    bool has[4];
    has[0] = g < p.pixels;
    qs[0] = bbd_c1_decode(&p, has[0] ? g : 0);
    const bool yrun = bbd_c1_y_run(&p, g, &qs[0]), xrun = bbd_c1_x_run(&p, g, &qs[0], 4);
    if (!(yrun && xrun)) {                           // (a strip at the end of a row, a sample or the batch)
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        has[j] = g + j < p.pixels;
        qs[j] = bbd_c1_decode(&p, has[j] ? g + j : 0);
      }
    }
    if (yrun) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const F4U t = *reinterpret_cast<const F4U*>(dy + bbd_c1_y_offset(&p, &qs[0], kb[i] * 16 + ch));
        a[i][0] = t.x; a[i][1] = t.y; a[i][2] = t.z; a[i][3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[i][j] = has[j] ? dy[bbd_c1_y_offset(&p, &qs[j], kb[i] * 16 + ch)] : 0.f;
    }
    if (xrun) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float* src = x + bbd_c1_x_offset(&p, &qs[0], cb[i] * 16 + ch);
        const F4U t = *reinterpret_cast<const F4U*>(src), u = *reinterpret_cast<const F4U*>(src + 4);
        b[i][0] = t.x; b[i][1] = t.z; b[i][2] = u.x; b[i][3] = u.z;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[i][j] = has[j] ? x[bbd_c1_x_offset(&p, &qs[j], cb[i] * 16 + ch)] : 0.f;
    }
  }
};

__global__ __launch_bounds__(THREADS) void conv1x1s2_wgrad_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ dy,
                                                                  double* __restrict__ scratch, bbd_c1_plan p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int kb[2], cb[2], kl[2], cl[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    kb[i] = bbd_c1_wave_block(&p, blockIdx.y, wave, 0, i);
    cb[i] = bbd_c1_wave_block(&p, blockIdx.y, wave, 1, i);
    kl[i] = kb[i] * 16 < p.K ? kb[i] : 0;            // a block past the last one loads block 0 and writes nothing
    cl[i] = cb[i] * 16 < p.C ? cb[i] : 0;
  }
  f32x4 acc[2][2];
  double total[2][2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2) {
      acc[i][i2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) total[i][i2][reg] = 0.0;
    }

  int first, last;
  bbd_c1_split_range(&p, blockIdx.x, &first, &last);
  StripRegs cur, nxt;
  if (first < last) cur.load(x, dy, p, first, lane, kl, cl);
  int in_run = 0;
#pragma unroll 1
  for (int st = first; st < last; ++st) {
    if (st + 1 < last) nxt.load(x, dy, p, st + 1, lane, kl, cl);      // in flight under this strip's MFMAs
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2)
          acc[i][i2] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[i][j], cur.b[i2][j], acc[i][i2], 0, 0, 0);
    if (++in_run == BBD_C1_RUN_STRIPS || st + 1 == last) {
      in_run = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) total[i][i2][reg] += (double)acc[i][i2][reg];
          acc[i][i2] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    cur = nxt;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2) {
      if (kb[i] * 16 >= p.K || cb[i2] * 16 >= p.C) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        scratch[bbd_c1_record_index(&p, blockIdx.x, kb[i], cb[i2], lane, reg)] = total[i][i2][reg];
    }
}

// Workgroup b: the BBD_C1_FINAL_E elements of dw from b * 16 on.  Thread (slice, e) adds the records slice, slice + 16,
// ... in that order, then thread e adds the 16 slices in order.
__global__ __launch_bounds__(BBD_C1_FINAL_E * BBD_C1_FINAL_G) void conv1x1s2_wgrad_final_kernel(
    const double* __restrict__ scratch, float* __restrict__ dw, bbd_c1_plan p) {
  __shared__ double part[BBD_C1_FINAL_G][BBD_C1_FINAL_E];
  const int e16 = threadIdx.x & (BBD_C1_FINAL_E - 1), slice = threadIdx.x / BBD_C1_FINAL_E;
  const long e = (long)blockIdx.x * BBD_C1_FINAL_E + e16, record = (long)p.K * p.C;
  double v = 0.0;
  for (int z = slice; z < p.splits; z += BBD_C1_FINAL_G) v += scratch[z * record + e];
  part[slice][e16] = v;
  __syncthreads();
  if (slice == 0) {
    double sum = 0.0;
    for (int s = 0; s < BBD_C1_FINAL_G; ++s) sum += part[s][e16];
    dw[e] = (float)sum;
  }
}

}  // namespace

extern "C" {

int bbd_conv1x1s2_supported(int N, int C, int K, int H, int W) {
  bbd_c1_plan p;
  return bbd_c1_make_plan(N, C, K, H, W, &p);
}

int bbd_conv1x1s2_wgrad_scratch_doubles(int N, int C, int K, int H, int W) {
  bbd_c1_plan p;
  return bbd_c1_make_plan(N, C, K, H, W, &p) ? bbd_c1_plan_scratch_doubles(&p) : 0;
}

int bbd_conv1x1s2_fwd(const float* x, const float* w, float* y, int N, int C, int K, int H, int W, void* stream) {
  bbd_c1_plan p;
  if (!x || !w || !y || !bbd_c1_make_plan(N, C, K, H, W, &p)) return BBD_E_BADARG;
  hipLaunchKernelGGL(conv1x1s2_fwd_kernel, dim3((unsigned)p.tiles, (unsigned)p.mblocks_fwd), dim3(THREADS), 0,
                     static_cast<hipStream_t>(stream), x, w, y, p);
  return status();
}

int bbd_conv1x1s2_bwd_data(const float* grad_y, const float* w, float* grad_x, int N, int C, int K, int H, int W,
                           int accumulate, void* stream) {
  bbd_c1_plan p;
  if (!grad_y || !w || !grad_x || !bbd_c1_make_plan(N, C, K, H, W, &p)) return BBD_E_BADARG;
  const dim3 grid((unsigned)p.tiles, (unsigned)p.mblocks_bwd), block(THREADS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (accumulate) hipLaunchKernelGGL(conv1x1s2_bwd_data_kernel<true>, grid, block, 0, st, grad_y, w, grad_x, p);
  else hipLaunchKernelGGL(conv1x1s2_bwd_data_kernel<false>, grid, block, 0, st, grad_y, w, grad_x, p);
  return status();
}

int bbd_conv1x1s2_wgrad(const float* x, const float* grad_y, float* grad_w, double* scratch, int scratch_doubles, int N,
                        int C, int K, int H, int W, void* stream) {
  bbd_c1_plan p;
  if (!x || !grad_y || !grad_w || !scratch || !bbd_c1_make_plan(N, C, K, H, W, &p) ||
      scratch_doubles < bbd_c1_plan_scratch_doubles(&p))
    return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(conv1x1s2_wgrad_kernel, dim3((unsigned)p.splits, (unsigned)(p.kblocks * p.cblocks)), dim3(THREADS),
                     0, st, x, grad_y, scratch, p);
  hipLaunchKernelGGL(conv1x1s2_wgrad_final_kernel, dim3((unsigned)((long)K * C / BBD_C1_FINAL_E)),
                     dim3(BBD_C1_FINAL_E * BBD_C1_FINAL_G), 0, st, scratch, grad_w, p);
  return status();
}

}  // extern "C"
