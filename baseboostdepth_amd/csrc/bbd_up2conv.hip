// bbd_up2conv.hip - the depth decoder's finest ConvBlock input without the up-sampled copy: nearest x2 up-sample +
// ReflectionPad2d(1) + 3x3 convolution of ELU(z + bias) as four 2x2 convolutions of the low-resolution map, one per
// output parity, and the adjoint of that (include/bbd_hip.h, bbd_up2conv3x3_*; the index arithmetic, the tile and the
// derivation of both forms: bbd_up2conv_math.h).  fp32 MFMA (v_mfma_f32_16x16x4_f32, an exact fp32 fma chain), no
// atomics: two launches give equal bits.
#include <hip/hip_runtime.h>

#include "../../include/bbd_hip.h"
#include "../../include/bbd_up2conv.h"
#include "bbd_up2conv_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CH = BBD_UP2CONV_CH;
constexpr int WG_THREADS = BBD_UP2CONV_WAVES * 64;
constexpr int TR = BBD_UP2CONV_TR, TC = BBD_UP2CONV_TC;
static_assert(TR == 2 * BBD_UP2CONV_WAVES, "a wave owns two rows of the forward tile");
static_assert(TC % BBD_UP2CONV_STRIP == 0, "a tile row is whole strips");
static_assert(BBD_UP2CONV_CSTRIDE >= (TR + 2) * BBD_UP2CONV_PITCH && BBD_UP2CONV_CSTRIDE % 64 == 16, "LDS channel stride");

struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };     // four floats at float alignment

int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// ELU as bbd_nn.hip's glue kernels write it (the weight gradient is taken from their copy of the same map).  ELU' is
// exp(v) from v itself: the glue's y + 1.0f carries the absolute error of y, 2^-25, which is 2^-25 * e^-v relative to
// ELU' - thousands of roundings where ELU is saturated - and the bound on grad_z has no room for that.
__device__ __forceinline__ float elu1(float v) { return v > 0.0f ? v : expm1f(v); }
__device__ __forceinline__ float elu1_grad(float g, float v) { return v > 0.0f ? g : g * expf(v); }

// sum over the kernel rows in `rows` and the kernel columns in `cols` (bit masks) of one 3x3 filter, in double
__device__ __forceinline__ float tap_sum(const float (&f)[9], int rows, int cols) {
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (((rows >> r) & 1) && ((cols >> c) & 1)) s += (double)f[r * 3 + c];
  return (float)s;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG_THREADS) void up2conv_fwd_kernel(const float* __restrict__ z, const float* __restrict__ bias,
                                                                const float* __restrict__ wt, float* __restrict__ out,
                                                                bbd_up2conv_plan p) {
  __shared__ float tile[BBD_UP2CONV_LDS_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bbd_up2conv_tile t = bbd_up2conv_decode(&p, blockIdx.x);

  // ELU(z + bias) of the tile and its clamped halo, once per element
  for (int e = threadIdx.x; e < CH * (TR + 2) * BBD_UP2CONV_PITCH; e += WG_THREADS) {
    int c, lr, lc;
    bbd_up2conv_fill_decode(e, &c, &lr, &lc);
    tile[bbd_up2conv_lds_index(c, lr, lc)] = elu1(z[bbd_up2conv_fill_src(&p, &t, c, lr, lc)] + bias[c]);
  }

  // A operands: wa[a][b][dy][dx][q] = the summed weights of output channel lane & 15, input channel 4q + (lane >> 4)
  float wa[2][2][2][2][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float f[9];
    const float* src = wt + ((lane & 15) * CH + 4 * q + (lane >> 4)) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = src[i];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx) wa[a][b][dy][dx][q] = tap_sum(f, bbd_up2conv_taps(a, dy), bbd_up2conv_taps(b, dx));
  }
  __syncthreads();

#pragma unroll 1
  for (int task = 0; task < 2 * (TC / BBD_UP2CONV_STRIP); ++task) {
    const int row = 2 * wave + task / (TC / BBD_UP2CONV_STRIP);          // row and first column inside the tile
    const int col0 = (task % (TC / BBD_UP2CONV_STRIP)) * BBD_UP2CONV_STRIP;
    const int i = t.i0 + row, j = t.j0 + col0 + (lane & 15);
    if (i >= p.h || t.j0 + col0 >= p.w) continue;                        // the same for the whole wave
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[3][3];                                                     // source rows i - 1 .. i + 1, columns j - 1 .. j + 1
#pragma unroll
      for (int dr = 0; dr < 3; ++dr)
#pragma unroll
        for (int dc = 0; dc < 3; ++dc) v[dr][dc] = tile[bbd_up2conv_b_index(q, lane, row + dr, col0 + dc)];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
              acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  wa[a][b][dy][dx][q], v[1 + bbd_up2conv_tap_offset(a, dy)][1 + bbd_up2conv_tap_offset(b, dx)], acc[a][b], 0, 0, 0);
    }
    if (j < p.w) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float2 o;
          o.x = acc[a][0][reg]; o.y = acc[a][1][reg];
          *reinterpret_cast<float2*>(out + bbd_up2conv_out_offset(&p, t.n, 4 * (lane >> 4) + reg, 2 * i + a, 2 * j)) = o;
        }
    }
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// the lane's data for output row Y: d[s][q] = the column sums of kernel column s, channel 4q + (lane >> 4)
__device__ __forceinline__ void load_row(const float* __restrict__ gout, const bbd_up2conv_plan& p, int n, int Y, int j, int lane,
                                         float (&d)[3][4]) {
  const bool inner = j > 0 && j < p.w - 1;                               // all four columns exist
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float* g = gout + bbd_up2conv_g_offset(&p, n, 4 * q + (lane >> 4), Y, j);
    float v[4];
    if (inner) {
      const F4U u = *reinterpret_cast<const F4U*>(g);
      v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) v[tt] = bbd_up2conv_g_live(&p, j, tt) ? g[tt] : 0.0f;
    }
    float s0 = v[2] + v[3], s2 = v[0] + v[1];
    if (j == 0) s0 += v[1];
    if (j == p.w - 1) s2 += v[2];
    d[0][q] = s0; d[1][q] = v[1] + v[2]; d[2][q] = s2;
  }
}

__global__ __launch_bounds__(WG_THREADS) void up2conv_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ z,
                                                                const float* __restrict__ bias, const float* __restrict__ wt,
                                                                float* __restrict__ gz, double* __restrict__ scratch,
                                                                bbd_up2conv_plan p) {
  __shared__ double part[BBD_UP2CONV_WAVES][CH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int n, i;
  const int group = bbd_up2conv_group(&p, blockIdx.x, &n, &i);

  // A operands: wb[u][s][q] = sum over the kernel rows of bbd_up2conv_bwd_taps(u) of w[k = 4q + (lane >> 4)][c = lane & 15][.][s]
  float wb[4][3][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float f[9];
    const float* src = wt + ((4 * q + (lane >> 4)) * CH + (lane & 15)) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) f[e] = src[e];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < 3; ++s) wb[u][s][q] = tap_sum(f, bbd_up2conv_bwd_taps(u), 1 << s);
  }
  float b4[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) b4[reg] = bias[4 * (lane >> 4) + reg];

  double bsum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int strip = wave; strip < p.strips; strip += BBD_UP2CONV_WAVES) {
    const int j = strip * BBD_UP2CONV_STRIP + (lane & 15);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!bbd_up2conv_row_live(&p, i, u)) continue;                     // the same for the whole workgroup
      float d[3][4];
      load_row(gout, p, n, 2 * i - 1 + u, j, lane, d);
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[u][s][q], d[s][q], acc, 0, 0, 0);
      // the clamp: output row 0 also reads source row 0 through kernel row 0 (wb[3]), output row 2h - 1 source row
      // h - 1 through kernel row 2 (wb[0])
      if (u == 1 && i == 0) {
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[3][s][q], d[s][q], acc, 0, 0, 0);
      }
      if (u == 2 && i == p.h - 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[0][s][q], d[s][q], acc, 0, 0, 0);
      }
    }
    if (j < p.w) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const long o = bbd_up2conv_src_offset(&p, n, 4 * (lane >> 4) + reg, i, j);
        const float r = elu1_grad(acc[reg], z[o] + b4[reg]);
        gz[o] = r;
        bsum[reg] += (double)r;
      }
    }
  }
  // grad_bias partial of the workgroup: 16 lanes of a channel, then the waves in order
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    double v = bsum[reg];
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((lane & 15) == 0) part[wave][4 * (lane >> 4) + reg] = v;
  }
  __syncthreads();
  if (threadIdx.x < CH) {
    double v = 0.0;
#pragma unroll
    for (int wv = 0; wv < BBD_UP2CONV_WAVES; ++wv) v += part[wv][threadIdx.x];
    scratch[bbd_up2conv_scratch_index(&p, threadIdx.x, group)] = v;
  }
}

// one wave per channel: lane l adds the groups l, l + 64, ... in that order, then the lanes are added pairwise
__global__ __launch_bounds__(BBD_UP2CONV_FINAL_THREADS) void up2conv_bias_final_kernel(const double* __restrict__ scratch,
                                                                                       float* __restrict__ gb,
                                                                                       bbd_up2conv_plan p) {
  const int c = blockIdx.x;
  double v = 0.0;
  for (int g = threadIdx.x; g < p.groups; g += BBD_UP2CONV_FINAL_THREADS) v += scratch[bbd_up2conv_scratch_index(&p, c, g)];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (threadIdx.x == 0) gb[c] = (float)v;
}

}  // namespace

extern "C" {

int bbd_up2conv3x3_supported(int N, int C, int K, int h, int w) {
  bbd_up2conv_plan p;
  return bbd_up2conv_make_plan(N, C, K, h, w, &p);
}

int bbd_up2conv3x3_scratch_doubles(int N, int C, int K, int h, int w) {
  bbd_up2conv_plan p;
  return bbd_up2conv_make_plan(N, C, K, h, w, &p) ? bbd_up2conv_plan_scratch_doubles(&p) : 0;
}

int bbd_up2conv3x3_fwd(const float* z, const float* bias, const float* w, float* out, int N, int C, int K, int h, int w_,
                       void* stream) {
  bbd_up2conv_plan p;
  if (!z || !bias || !w || !out || !bbd_up2conv_make_plan(N, C, K, h, w_, &p)) return BBD_E_BADARG;
  hipLaunchKernelGGL(up2conv_fwd_kernel, dim3((unsigned)p.blocks), dim3(WG_THREADS), 0, static_cast<hipStream_t>(stream), z,
                     bias, w, out, p);
  return status();
}

int bbd_up2conv3x3_bwd(const float* grad_out, const float* z, const float* bias, const float* w, float* grad_z,
                       float* grad_bias, double* scratch, int scratch_doubles, int N, int C, int K, int h, int w_,
                       void* stream) {
  bbd_up2conv_plan p;
  if (!grad_out || !z || !bias || !w || !grad_z || !grad_bias || !scratch || !bbd_up2conv_make_plan(N, C, K, h, w_, &p) ||
      scratch_doubles < bbd_up2conv_plan_scratch_doubles(&p))
    return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(up2conv_bwd_kernel, dim3((unsigned)p.groups), dim3(WG_THREADS), 0, st, grad_out, z, bias, w, grad_z,
                     scratch, p);
  hipLaunchKernelGGL(up2conv_bias_final_kernel, dim3(CH), dim3(BBD_UP2CONV_FINAL_THREADS), 0, st, scratch, grad_bias, p);
  return status();
}

}  // extern "C"
