// bbd_sgm.hip - semi-global stereo matching on the device (ops.stereo_hints, --depth_hints; Hirschmueller,
// PAMI 2008; Watson et al., ICCV 2019): a proxy disparity per training frame from the rectified stereo pair the loader
// already delivers.  Every rule - grey, census, cost, the path recurrence and its overflow bound, winner takes all,
// uniqueness, the left-right check, the sub-pixel division, the fill - is bbd_sgm_math.h, shared with the host port.
// Integer arithmetic: device == port == numpy reference byte for byte, and the same bytes every run.
//
//   sgm_grey_kernel     a lane per pixel of both images: three float32 loads (mirrored column where side[b] != 0) ->
//                       one grey byte in matching coordinates
//   sgm_census_kernel   a lane per pixel of both images: 62 clamped grey loads (L1 / L2 hits) -> one 64-bit word
//   sgm_cost_kernel     a lane per pixel and four disparities: popcounts -> four cost bytes in one store
//   sgm_path_kernel     one launch per direction.  A WAVE walks one line of bbd_sgm_line_pixel (an image row for the
//                       horizontal directions; for the others a column that shifts by dx a row and wraps, so that four
//                       neighbouring waves of a workgroup read neighbouring pixels); its 64 lanes hold D / 64 neighbouring
//                       disparities each, the previous pixel's L_r stays in registers, d - 1 and d + 1 across lanes are
//                       two shuffles, the minimum a butterfly.  The cost and the old S of the NEXT pixel are loaded before
//                       the recurrence of this one, so the dependent chain is arithmetic and shuffles only.  The first
//                       direction stores S, the others add to it: launches of one stream, plain 16-bit adds, no atomics
//   sgm_select_kernel   a wave per pixel: the keys S * 256 + d of dL (its own D sums) and of dR (the diagonal S(x + d, d)),
//                       each a wave minimum, and the uniqueness test as a ballot -> one sel word
//   sgm_finish_kernel   a lane per pixel: validity from the sel words, the sub-pixel value, the store at the mirrored
//                       column where side[b] != 0; integer counts per workgroup, one integer atomic add per workgroup
//   sgm_fill_kernel     (fill only) a wave per row: 64 pixels a step, nearest valid pixel at a smaller x by ballot and
//                       shuffle, the carry across steps in a register
//
// Plain C++, vector stores, no inline assembly, no float atomics.  No allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "../../include/bbd_sgm.h"
#include "bbd_device_util.h"
#include "bbd_sgm_math.h"

namespace {

constexpr int ST = 256;  // threads of every kernel
constexpr int SW = ST / 64;

struct SgmCall {
  const float* left;   // [B,3,H,W]
  const float* right;  // [B,3,H,W]
  const int32_t* side; // [B]
  BbdSgmScratch s;
  int B, H, W, D, p1, p2, uniqueness;
};

__global__ __launch_bounds__(ST) void sgm_clear_kernel(int64_t* valid_count, int B) {
  for (int b = threadIdx.x; b < B; b += ST) valid_count[b] = 0;
}

__global__ __launch_bounds__(ST) void sgm_grey_kernel(SgmCall a) {
  const size_t plane = (size_t)a.H * a.W, n = (size_t)a.B * 2 * plane;
  for (size_t i = blockIdx.x * (size_t)ST + threadIdx.x; i < n; i += (size_t)gridDim.x * ST) {
    const size_t bi = i / plane, k = i - bi * plane;
    const int b = (int)(bi >> 1), y = (int)(k / a.W), x = (int)(k - (size_t)y * a.W);
    const float* img = ((bi & 1) ? a.right : a.left) + (size_t)b * 3 * plane + (size_t)y * a.W +
                       bbd_sgm_column(x, a.W, a.side[b] != 0);
    a.s.grey[i] = (uint8_t)bbd_sgm_luma(img[0], img[plane], img[2 * plane]);
  }
}

__global__ __launch_bounds__(ST) void sgm_census_kernel(SgmCall a) {
  const size_t plane = (size_t)a.H * a.W, n = (size_t)a.B * 2 * plane;
  for (size_t i = blockIdx.x * (size_t)ST + threadIdx.x; i < n; i += (size_t)gridDim.x * ST) {
    const size_t bi = i / plane, k = i - bi * plane;
    const int y = (int)(k / a.W), x = (int)(k - (size_t)y * a.W);
    a.s.census[i] = bbd_sgm_census(a.s.grey + bi * plane, a.H, a.W, x, y);
  }
}

__global__ __launch_bounds__(ST) void sgm_cost_kernel(SgmCall a) {
  const size_t quads = (size_t)(a.D / 4), n = (size_t)a.B * a.H * a.W * quads;
  for (size_t i = blockIdx.x * (size_t)ST + threadIdx.x; i < n; i += (size_t)gridDim.x * ST) {
    const size_t p = i / quads;                                      // pixel of the batch
    const int d0 = (int)(i - p * quads) * 4;
    const size_t row = p / a.W;                                      // b * H + y
    const int x = (int)(p - row * a.W), b = (int)(row / a.H);
    const uint64_t* cl = a.s.census + ((size_t)b * a.H + row) * a.W; // [b][0][y] = (2 b H + y) W, row = b H + y
    const uint64_t* cr = cl + (size_t)a.H * a.W;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= (uint32_t)bbd_sgm_cost(cl, cr, x, d0 + j) << (8 * j);
    reinterpret_cast<uint32_t*>(a.s.cost)[i] = word;                 // p * D + d0 is a multiple of 4
  }
}

// A lane's N cost bytes and N sums, aligned so that each is one load (N = 3: element by element).
template <int N>
struct alignas(N == 3 ? 1 : N) Bytes { uint8_t v[N]; };
template <int N>
struct alignas(N == 3 ? 2 : 2 * N) Halves { uint16_t v[N]; };

__device__ __forceinline__ int wave_min_all(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_min_all(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// N = D / 64 neighbouring disparities a lane: d = lane * N + j.
template <int N>
__global__ __launch_bounds__(ST) void sgm_path_kernel(SgmCall a, int dx, int dy, int first) {
  const int lane = threadIdx.x & 63;
  const int lines = bbd_sgm_lines(dy, a.H, a.W), steps = bbd_sgm_steps(dy, a.H, a.W);
  const long gw = (long)blockIdx.x * SW + (threadIdx.x >> 6);        // uniform over the wave; no barrier below
  if (gw >= (long)a.B * lines) return;
  const int b = (int)(gw / lines), line = (int)(gw - (long)b * lines);
  const size_t base = (size_t)b * a.H * a.W;
  const int D = a.D, d0 = lane * N, p1 = a.p1, p2 = a.p2;
  int prev[N], m = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) prev[j] = 0;
  int x, y;
  int start = bbd_sgm_line_pixel(dx, dy, a.H, a.W, line, 0, &x, &y);
  size_t at = (base + (size_t)y * a.W + x) * D + d0;                 // a multiple of N: both loads are aligned
  Bytes<N> c = *reinterpret_cast<const Bytes<N>*>(a.s.cost + at);
  Halves<N> old;
#pragma unroll
  for (int j = 0; j < N; ++j) old.v[j] = 0;
  if (!first) old = *reinterpret_cast<const Halves<N>*>(a.s.S + at);
  for (int t = 0; t < steps; ++t) {
    // the next pixel's loads do not depend on this pixel's recurrence: issue them first
    Bytes<N> c_next = c;
    Halves<N> old_next = old;
    size_t at_next = at;
    int start_next = 0;
    if (t + 1 < steps) {
      start_next = bbd_sgm_line_pixel(dx, dy, a.H, a.W, line, t + 1, &x, &y);
      at_next = (base + (size_t)y * a.W + x) * D + d0;
      c_next = *reinterpret_cast<const Bytes<N>*>(a.s.cost + at_next);
      if (!first) old_next = *reinterpret_cast<const Halves<N>*>(a.s.S + at_next);
    }
    int cur[N];
    if (start) {
#pragma unroll
      for (int j = 0; j < N; ++j) cur[j] = c.v[j];
    } else {
      const int from_below = __shfl_up(prev[N - 1], 1, 64);          // L_r(q, d0 - 1): lane - 1's last
      const int from_above = __shfl_down(prev[0], 1, 64);            // L_r(q, d0 + N): lane + 1's first
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int below = j ? prev[j - 1] : from_below, above = j + 1 < N ? prev[j + 1] : from_above;
        cur[j] = bbd_sgm_step(c.v[j], prev[j], below, above, d0 + j > 0, d0 + j + 1 < D, m, p1, p2);
      }
    }
    int mine = cur[0];
#pragma unroll
    for (int j = 1; j < N; ++j) mine = min(mine, cur[j]);
    m = wave_min_all(mine);
    Halves<N> out;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      out.v[j] = (uint16_t)(old.v[j] + cur[j]);                      // <= 8 (62 + P2) <= 65528
      prev[j] = cur[j];
    }
    *reinterpret_cast<Halves<N>*>(a.s.S + at) = out;
    c = c_next; old = old_next; at = at_next; start = start_next;
  }
}

template <int N>
__global__ __launch_bounds__(ST) void sgm_select_kernel(SgmCall a) {
  const int lane = threadIdx.x & 63;
  const size_t n = (size_t)a.B * a.H * a.W;
  const size_t p = (size_t)blockIdx.x * SW + (threadIdx.x >> 6);     // a wave per pixel; no barrier below
  if (p >= n) return;
  const int x = (int)(p % a.W), D = a.D, d0 = lane * N;
  const Halves<N> s = *reinterpret_cast<const Halves<N>*>(a.s.S + p * D + d0);
  uint32_t kl = 0xffffffffu, kr = 0xffffffffu;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    kl = min(kl, bbd_sgm_key(s.v[j], d0 + j));
    if (x + d0 + j < a.W) kr = min(kr, bbd_sgm_key(a.s.S[(p + d0 + j) * D + d0 + j], d0 + j));
  }
  kl = wave_min_all(kl);
  kr = wave_min_all(kr);                                             // d = 0 always takes part: never all ones
  const int best_s = (int)(kl >> 8), best_d = (int)(kl & 255u);
  int rival = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) rival |= bbd_sgm_rivals(s.v[j], d0 + j, best_s, best_d, a.uniqueness);
  const int not_unique = __ballot(rival) != 0;
  if (lane == 0) a.s.sel[p] = bbd_sgm_sel(best_d, (int)(kr & 255u), not_unique);
}

__global__ __launch_bounds__(ST) void sgm_finish_kernel(SgmCall a, int16_t* disp16, int64_t* valid_count) {
  __shared__ int part[SW];
  const int plane = a.H * a.W, b = blockIdx.y;                       // H W <= 2^26
  const int k = blockIdx.x * ST + threadIdx.x;
  int valid = 0;
  if (k < plane) {
    const int y = k / a.W, x = k - y * a.W;
    const size_t row = ((size_t)b * a.H + y) * a.W;
    valid = bbd_sgm_valid(a.s.sel + row, x);
    int v = BBD_SGM_INVALID;
    if (valid) v = bbd_sgm_disp16(a.s.S + (row + x) * a.D, (int)(a.s.sel[row + x] & 255u), a.D);
    disp16[row + bbd_sgm_column(x, a.W, a.side[b] != 0)] = (int16_t)v;
  }
  const int total = __popcll(__ballot(valid));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < SW; ++w) t += part[w];
    if (t) atomicAdd(reinterpret_cast<unsigned long long*>(valid_count + b), (unsigned long long)t);
  }
}

__global__ __launch_bounds__(ST) void sgm_fill_kernel(SgmCall a, int16_t* disp16) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)a.B * a.H, r = (long)blockIdx.x * SW + (threadIdx.x >> 6);
  if (r >= rows) return;                                             // uniform over the wave; no barrier below
  const int mirrored = a.side[r / a.H] != 0;
  int16_t* row = disp16 + (size_t)r * a.W;
  int carry = BBD_SGM_INVALID, first_x = a.W, first_v = BBD_SGM_INVALID;
  for (int x0 = 0; x0 < a.W; x0 += 64) {
    const int x = x0 + lane;
    int v = x < a.W ? row[bbd_sgm_column(x, a.W, mirrored)] : BBD_SGM_INVALID;
    const unsigned long long have = __ballot(v != BBD_SGM_INVALID);
    const unsigned long long upto = have & (lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull);
    const int src = upto ? 63 - __clzll((long long)upto) : 0;
    const int taken = __shfl(v, src, 64);
    const int filled = upto ? taken : carry;
    if (x < a.W && v == BBD_SGM_INVALID && filled != BBD_SGM_INVALID) row[bbd_sgm_column(x, a.W, mirrored)] = (int16_t)filled;
    if (have) {
      if (first_x == a.W) {
        const int f = __ffsll((long long)have) - 1;
        first_x = x0 + f;
        first_v = __shfl(v, f, 64);
      }
      carry = __shfl(v, 63 - __clzll((long long)have), 64);
    }
  }
  if (first_x < a.W)                                                 // what lies before the row's first valid pixel
    for (int x = lane; x < first_x; x += 64) row[bbd_sgm_column(x, a.W, mirrored)] = (int16_t)first_v;
}

unsigned blocks_for(size_t items, size_t per_block, size_t most) {
  const size_t n = (items + per_block - 1) / per_block;
  return (unsigned)(n < 1 ? 1 : n < most ? n : most);
}

template <int N>
void launch_paths(const SgmCall& a, int paths, hipStream_t st) {
  for (int r = 0; r < paths; ++r) {
    int dx, dy;
    bbd_sgm_direction(r, &dx, &dy);
    const size_t waves = (size_t)a.B * bbd_sgm_lines(dy, a.H, a.W);
    hipLaunchKernelGGL(sgm_path_kernel<N>, dim3(blocks_for(waves, SW, ~0u)), dim3(ST), 0, st, a, dx, dy, r == 0);
  }
  const size_t pixels = (size_t)a.B * a.H * a.W;                     // <= 2^26: the grid holds a wave per pixel
  hipLaunchKernelGGL(sgm_select_kernel<N>, dim3(blocks_for(pixels, SW, ~0u)), dim3(ST), 0, st, a);
}

}  // namespace

extern "C" long bbd_sgm_scratch_bytes(int B, int H, int W, int D, int paths) { return bbd_sgm_bytes(B, H, W, D, paths); }

extern "C" int bbd_sgm_hints(const float* left, const float* right, const int32_t* side, int16_t* disp16,
                             int64_t* valid_count, void* scratch, long scratch_bytes, int B, int H, int W, int D,
                             int paths, int p1, int p2, int uniqueness, int fill, void* stream) {
  const int rc = bbd_sgm_status(left, right, side, disp16, valid_count, scratch, scratch_bytes, B, H, W, D, paths, p1, p2,
                                uniqueness, fill);
  if (rc) return rc;
  SgmCall a;
  a.left = left; a.right = right; a.side = side;
  a.B = B; a.H = H; a.W = W; a.D = D; a.p1 = p1; a.p2 = p2; a.uniqueness = uniqueness;
  bbd_sgm_carve(scratch, B, H, W, D, &a.s);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t pixels = (size_t)B * H * W, most = 1 << 20;           // work beyond `most` workgroups is reached by striding
  hipLaunchKernelGGL(sgm_clear_kernel, dim3(1), dim3(ST), 0, st, valid_count, B);
  hipLaunchKernelGGL(sgm_grey_kernel, dim3(blocks_for(2 * pixels, ST, most)), dim3(ST), 0, st, a);
  hipLaunchKernelGGL(sgm_census_kernel, dim3(blocks_for(2 * pixels, ST, most)), dim3(ST), 0, st, a);
  hipLaunchKernelGGL(sgm_cost_kernel, dim3(blocks_for(pixels * (D / 4), ST, most)), dim3(ST), 0, st, a);
  switch (D / 64) {
    case 1: launch_paths<1>(a, paths, st); break;
    case 2: launch_paths<2>(a, paths, st); break;
    case 3: launch_paths<3>(a, paths, st); break;
    default: launch_paths<4>(a, paths, st); break;
  }
  hipLaunchKernelGGL(sgm_finish_kernel, dim3(blocks_for((size_t)H * W, ST, ~0u), B), dim3(ST), 0, st, a, disp16,
                     valid_count);
  if (fill) hipLaunchKernelGGL(sgm_fill_kernel, dim3(blocks_for((size_t)B * H, SW, ~0u)), dim3(ST), 0, st, a, disp16);
  return launch_status();
}
