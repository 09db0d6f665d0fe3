// bbd_wgrad.hip - weight gradient of a 3x3, stride-1 convolution of a pre-padded NCHW input, straight from the NCHW
// tensors: no transposed copies, no atomics, no zero-fill (include/bbd_hip.h, bbd_conv3x3_wgrad; the index arithmetic
// and the layout of a scratch record: bbd_wgrad_math.h).
//
//   dw[k][c][r][s] = sum over (n, y, x) of grad_z[n][k][y][x] * xp[n][c][y + r][x + s]
//
// is a GEMM that reduces over pixels, and in NCHW both operands are contiguous along pixels.  A wave takes strips of 16
// pixels of a row: lane l loads 4 pixels of grad_z for output channel l & 15 and, per kernel row and block of 16 input
// channels, the 6 floats of xp that the three taps of those pixels need (one 16-byte and one 8-byte access at 4-byte
// alignment); v_mfma_f32_16x16x4_f32 number j contracts component j of both.  The MFMA is an exact fp32 fma chain, so
// an accumulator that has taken BBD_WGRAD_RUN products is widened: the waves of a workgroup pass their tiles through
// LDS, one kernel row at a time, and the thread that owns an element adds the waves' values to its double in wave
// order.  The workgroup's doubles go to `scratch`; a second launch adds the workgroups in a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/bbd_hip.h"
#include "../../include/bbd_wgrad.h"
#include "bbd_wgrad_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WG_THREADS = BBD_WGRAD_WAVES * 64;
constexpr int WG_ROW = 3 * BBD_WGRAD_TILE;          // the three taps of one kernel row: what one LDS pass carries

int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// what one lane holds of one strip: its 4 pixels of grad_z and, per channel block and kernel row, 6 floats of xp
template <int NCB>
struct Frag {
  float g[4];
  float x[NCB][3][6];
};

struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };     // four / two floats at float alignment
struct __attribute__((packed, aligned(4))) F2U { float x, y; };

__device__ __forceinline__ void load4(const float* p, float* v) {
  const F4U t = *reinterpret_cast<const F4U*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void load2(const float* p, float* v) {
  const F2U t = *reinterpret_cast<const F2U*>(p);
  v[0] = t.x; v[1] = t.y;
}

// `pixels` = how many of the lane's 4 pixels lie inside the row.  A lane loads nothing beyond them (xp: + 2 columns of
// border), and takes zeros there.
template <int NCB>
__device__ __forceinline__ void load_strip(Frag<NCB>& f, const float* __restrict__ xp, const float* __restrict__ gz,
                                           const bbd_wgrad_plan& p, const bbd_wgrad_strip& s, int kb, int cb0, int lane,
                                           int g_lane, int x_lane) {
  // a pointer that is the wave's + an offset that is the lane's in every strip (bbd_wgrad_gz_offset / _xp_offset)
  const float* g = gz + bbd_wgrad_gz_base(&p, &s, kb) + g_lane;
  if (s.full) {
    load4(g, f.g);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float* x = xp + bbd_wgrad_xp_base(&p, &s, cb0 + cb, r) + x_lane;
        load4(x, f.x[cb][r]);
        load2(x + 4, f.x[cb][r] + 4);
      }
  } else {
    const int pixels = bbd_wgrad_lane_pixels(&p, &s, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) f.g[j] = j < pixels ? g[j] : 0.f;
    const int cols = pixels ? pixels + 2 : 0;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float* x = xp + bbd_wgrad_xp_base(&p, &s, cb0 + cb, r) + x_lane;
#pragma unroll
        for (int i = 0; i < 6; ++i) f.x[cb][r][i] = i < cols ? x[i] : 0.f;
      }
  }
}

// A pixel outside the row contributes 0 * 0: its grad_z is zero, and so is what stands for xp under each of its taps
// (in a strip that is not full, xp values of pixels that do exist may sit at the same position of another tap).
template <int NCB, bool FULL>
__device__ __forceinline__ void mfma_strip(f32x4 (&acc)[NCB][9], const Frag<NCB>& f, int pixels) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool live = FULL || j < pixels;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const float b = live ? f.x[cb][r][j + s] : 0.f;
          acc[cb][r * 3 + s] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.g[j], b, acc[cb][r * 3 + s], 0, 0, 0);
        }
  }
}

// End of an fp32 run: every wave's tiles, one kernel row of one channel block at a time, through `stage`; thread t < 192
// owns the 4 elements [t * 4, t * 4 + 4) of each such row and adds the waves' values to `total` in wave order.
template <int NCB>
__device__ __forceinline__ void widen(f32x4 (&acc)[NCB][9], f32x4 (*stage)[WG_ROW / 4], double* total, int wave, int lane) {
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      __syncthreads();                               // the pass before has been read
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        stage[wave][s * 64 + lane] = acc[cb][r * 3 + s];
        acc[cb][r * 3 + s] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      __syncthreads();
      const int t = threadIdx.x;
      if (t < WG_ROW / 4) {
        double* mine = total + ((cb * 3 + r) * (WG_ROW / 4) + t) * 4;
        double a0 = mine[0], a1 = mine[1], a2 = mine[2], a3 = mine[3];
#pragma unroll
        for (int w = 0; w < BBD_WGRAD_WAVES; ++w) {
          const f32x4 v = stage[w][t];
          a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
        }
        mine[0] = a0; mine[1] = a1; mine[2] = a2; mine[3] = a3;
      }
    }
}

template <int NCB>
__device__ __forceinline__ void conv3x3_wgrad_body(const float* __restrict__ xp, const float* __restrict__ gz,
                                                   double* __restrict__ scratch, const bbd_wgrad_plan& p) {
  __shared__ f32x4 stage[BBD_WGRAD_WAVES][WG_ROW / 4];          // 24 KB
  __shared__ double total[9 * NCB * BBD_WGRAD_TILE];            // 18 KB per channel block: the record
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // one value per wave: strips are scalar
  const int group = blockIdx.x, role = blockIdx.y;
  int kb, cb0;
  bbd_wgrad_role(&p, role, &kb, &cb0);
  for (int i = threadIdx.x; i < p.record; i += WG_THREADS) total[i] = 0.0;      // (widen() starts with a barrier)

  f32x4 acc[NCB][9];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[cb][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  int first, last;
  bbd_wgrad_wave_range(&p, group, wave, &first, &last);
  const int g_lane = bbd_wgrad_gz_lane(&p, lane), x_lane = bbd_wgrad_xp_lane(&p, lane);
  Frag<NCB> cur, nxt;
  bbd_wgrad_strip sc = bbd_wgrad_decode(&p, first < last ? first : 0), sn = sc;
  if (first < last) load_strip<NCB>(cur, xp, gz, p, sc, kb, cb0, lane, g_lane, x_lane);
  // every wave of the workgroup makes the same `per` steps, so that all of them meet at the barriers of widen()
  for (int i = 0; i < p.per; ++i) {
    const int strip = first + i;
    const bool have = strip < last, more = strip + 1 < last;
    if (more) {
      sn = bbd_wgrad_next(&p, sc);
      load_strip<NCB>(nxt, xp, gz, p, sn, kb, cb0, lane, g_lane, x_lane);
    }
    if (have) {
      if (sc.full) mfma_strip<NCB, true>(acc, cur, 4);
      else mfma_strip<NCB, false>(acc, cur, bbd_wgrad_lane_pixels(&p, &sc, lane));
    }
    if (more) { cur = nxt; sc = sn; }
    if (bbd_wgrad_run_ends(&p, i)) widen<NCB>(acc, stage, total, wave, lane);
  }
  __syncthreads();
  double* rec = scratch + bbd_wgrad_record_offset(&p, group, role);
  for (int i = threadIdx.x; i < p.record; i += WG_THREADS) rec[i] = total[i];
}

// One block of input channels per role: 36 accumulator registers, held to 128 registers in all so that two workgroups
// (4 waves per SIMD) share a CU.  Two blocks: 72 accumulator registers, one workgroup per CU.
__global__ __launch_bounds__(WG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void conv3x3_wgrad_kernel_1(
    const float* __restrict__ xp, const float* __restrict__ gz, double* __restrict__ scratch, bbd_wgrad_plan p) {
  conv3x3_wgrad_body<1>(xp, gz, scratch, p);
}
__global__ __launch_bounds__(WG_THREADS) void conv3x3_wgrad_kernel_2(
    const float* __restrict__ xp, const float* __restrict__ gz, double* __restrict__ scratch, bbd_wgrad_plan p) {
  conv3x3_wgrad_body<2>(xp, gz, scratch, p);
}

// Workgroup b: the BBD_WGRAD_FINAL_E record elements from b * 16 on.  Thread (slice, e) adds the groups slice, slice +
// 16, ... in that order (16 neighbouring doubles of a record per access), then thread e adds the 16 slices in order.
__global__ __launch_bounds__(BBD_WGRAD_FINAL_E * BBD_WGRAD_FINAL_G) void conv3x3_wgrad_final_kernel(
    const double* __restrict__ scratch, float* __restrict__ gw, bbd_wgrad_plan p) {
  __shared__ double part[BBD_WGRAD_FINAL_G][BBD_WGRAD_FINAL_E];
  const int e16 = threadIdx.x & (BBD_WGRAD_FINAL_E - 1), slice = threadIdx.x / BBD_WGRAD_FINAL_E;
  const int idx = blockIdx.x * BBD_WGRAD_FINAL_E + e16;         // element of the [roles][record] plane
  const int role = idx / p.record, e = idx - role * p.record;   // (record is a multiple of 16: one role per workgroup)
  double v = 0.0;
  for (int g = slice; g < p.groups; g += BBD_WGRAD_FINAL_G) v += scratch[bbd_wgrad_record_offset(&p, g, role) + e];
  part[slice][e16] = v;
  __syncthreads();
  if (slice == 0) {
    double sum = 0.0;
    for (int q = 0; q < BBD_WGRAD_FINAL_G; ++q) sum += part[q][e16];
    gw[bbd_wgrad_record_to_weight(&p, role, e)] = (float)sum;
  }
}

}  // namespace

extern "C" {

int bbd_conv3x3_wgrad_supported(int N, int C, int K, int H, int W) {
  bbd_wgrad_plan p;
  return bbd_wgrad_make_plan(N, C, K, H, W, BBD_WGRAD_RUN, &p);
}

int bbd_conv3x3_wgrad_scratch_doubles(int N, int C, int K, int H, int W) {
  bbd_wgrad_plan p;
  return bbd_wgrad_make_plan(N, C, K, H, W, BBD_WGRAD_RUN, &p) ? bbd_wgrad_plan_scratch_doubles(&p) : 0;
}

int bbd_conv3x3_wgrad(const float* xp, const float* grad_z, float* grad_w, double* scratch, int N, int C, int K, int H,
                      int W, void* stream) {
  bbd_wgrad_plan p;
  if (!xp || !grad_z || !grad_w || !scratch || !bbd_wgrad_make_plan(N, C, K, H, W, BBD_WGRAD_RUN, &p)) return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)p.groups, (unsigned)p.roles);
  if (p.ncb == 2)
    hipLaunchKernelGGL(conv3x3_wgrad_kernel_2, grid, dim3(WG_THREADS), 0, st, xp, grad_z, scratch, p);
  else
    hipLaunchKernelGGL(conv3x3_wgrad_kernel_1, grid, dim3(WG_THREADS), 0, st, xp, grad_z, scratch, p);
  const int elements = p.roles * p.record;                      // = 9 * C * K
  hipLaunchKernelGGL(conv3x3_wgrad_final_kernel, dim3((unsigned)(elements / BBD_WGRAD_FINAL_E)),
                     dim3(BBD_WGRAD_FINAL_E * BBD_WGRAD_FINAL_G), 0, st, scratch, grad_w, p);
  return status();
}

}  // extern "C"
