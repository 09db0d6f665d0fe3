// bbd_nn.hip - fused training-mode BatchNorm2d (+ residual add) (+ ReLU), forward and backward.
//
// The encoders are torchvision-layout ResNets (networks/resnet_encoder.py:12-91): every convolution is
// followed by BatchNorm2d, then either ReLU or "+ identity, ReLU".  In eager PyTorch-ROCm that is one
// MIOpen batch-norm launch plus separate add / clamp / threshold kernels, each a full round trip over
// the activation (profiles/r01/bench_md2_one_steady_step_v6.csv: 2.6 ms BN + ~1.3 ms add/ReLU per step).
// Here the tail of a block is two launches each way over NCHW fp32:
//
//   forward : stats   per channel sums of x - pivot and its square (centred fp32 runs, fp64 partials, fixed-order combine)
//             apply   y = relu(gamma * (x - mean) * invstd + beta + residual); running stats updated
//   backward: reduce  g = dy * (y > 0);  per channel sum(g), sum(g * xhat)
//             apply   dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat));  dresidual = g;
//                     dgamma = sum(g * xhat), dbeta = sum(g)
//
// Same definition as torch.nn.functional.batch_norm(training=True): biased variance for the
// normalisation, unbiased for running_var, momentum update of the running statistics.  HBM-bound
// elementwise / reduction work: coalesced float4 accesses of each (n, c) plane, one workgroup per
// (channel, slice of the plane), deterministic (no floating-point atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_bn_groups.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_SPLIT = 64;
#ifndef BN_SMALL_ELEMS
#define BN_SMALL_ELEMS 8192     // per (channel, call group): at or below this the two passes of a direction share one launch
#endif
static_assert(BBD_STEM_MIN_ELEMS == BN_SMALL_ELEMS, "the stem takes exactly the activations of the two-launch form");

struct BnArgs {
  const float* x;        // [N,C,HW] conv output
  const float* res;      // residual or NULL
  const float* gamma;    // [C]
  const float* beta;     // [C]
  float* y;              // [N,C,HW]
  double* part;          // [C, split, 2] scratch
  float* mean;           // [C] saved for backward
  float* invstd;         // [C]
  float* run_mean;       // [C] or NULL
  float* run_var;        // [C] or NULL
  long long* batches;    // num_batches_tracked (int64 scalar) or NULL
  // backward
  const float* dy;
  float* dx;
  float* dres;           // or NULL
  float* dgamma;
  float* dbeta;
  int N, C, HW, split, relu;
  float eps, momentum;
  // encoder stem (bbd_stem_*): MaxPool2d(3, 2, 1) of y fused into both directions.  W = row length of the HW plane;
  // forward: y may be NULL, pooled / code [N,C,OH,OW] are written; backward: dy may be NULL, gpool / code are read
  int W;
  float* pooled;
  uint8_t* code;
  const float* gpool;
  // call groups: samples [rows[g], rows[g+1]) are normalised with their own statistics, as if each group had been
  // a separate call of the layer (one batched pass of a network that the reference calls G times); blockIdx.z = g
  int G;
  int untracked;         // the last `untracked` groups are normalised like the others but leave the running statistics alone
  // device-resident group table (bbd_bn_act_grouped_dev_*): rows[0..G] then, at [BBD_BN_MAX_GROUPS + 1], the number of
  // tracked groups - a launch whose arguments do not depend on the batch signature, so that ONE captured step graph
  // serves every ordering with the same padded row count.  Groups may be empty there.  NULL: the by-value table below
  const int32_t* rows_dev;
  int rows[BBD_BN_MAX_GROUPS + 1];
};

__device__ __forceinline__ int group_row(const BnArgs& a, int g) { return a.rows_dev ? a.rows_dev[g] : a.rows[g]; }
__device__ __forceinline__ int tracked_groups(const BnArgs& a) {
  return a.rows_dev ? a.rows_dev[BBD_BN_MAX_GROUPS + 1] : a.G - a.untracked;
}

__device__ __forceinline__ double block_sum(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// number of plane slices for a batch of N images (host: grid size for the largest group; device: each group's own, so
// that a group is reduced exactly as a separate call on that sub-batch would reduce it)
__host__ __device__ inline int pick_split(int N, int HW) {
  long long per = (long long)N * HW;
  int s = (int)((per + 4095) / 4096);
  if (s < 1) s = 1;
  if (s > MAX_SPLIT) s = MAX_SPLIT;
  const int max_by_plane = (HW + 3) / 4;     // at least one float4 of the plane per slice
  return s < max_by_plane ? s : max_by_plane;
}

// slice k of `split` of the HW plane: [lo, hi), multiples of 4 when HW % 4 == 0
__device__ __forceinline__ void plane_slice(int HW, int split, int k, int* lo, int* hi) {
  int len = (HW + split - 1) / split;
  len = (len + 3) & ~3;
  *lo = k * len;
  *hi = min(HW, *lo + len);
}

// The four passes below are written per (channel c, call group grp, plane slice k).  Large activations launch one
// workgroup per slice and pass the per-slice sums through `part` (two launches per direction); small ones (a whole
// (channel, group) fits one workgroup comfortably) run both passes in ONE launch, the workgroup looping over the same
// slices and adding their block totals in the same order - identical numbers, half the launches, no partial round trip.
// Thread layout: 64 lanes sweep the slice, the 4 waves take every 4th image - a slice is only ~100 float4 long, so 256
// lanes along it left most of them idle with one dependent load per image in flight.

// The pivot of one (channel, group): its first element.  The totals that leave stats_slice are sums of (x - pivot) and
// (x - pivot)^2, so that the subtraction in group_moments cancels digits of a deviation (about one standard deviation
// for typical data, exactly 0 for a constant channel) and not of the mean.  A far-off pivot (an outlier in that very
// place) costs digits of the double totals only - the fp32 part below never sees it.
__device__ __forceinline__ double group_pivot(const BnArgs& a, int c, int grp) {
  const int first = group_row(a, grp);
  if (first >= group_row(a, grp + 1)) return 0.0;              // an empty group of a device-resident table
  return (double)a.x[((size_t)first * a.C + c) * a.HW];
}

// forward statistics of slice k: block totals of (x - pivot) and (x - pivot)^2.
// Squares of x itself, added up in fp32, lose (mean / std)^2 of the variance's digits however the runs are combined
// afterwards.  So each lane keeps (count, mean, M2 = sum of squared deviations from that mean) of its run through one
// image: a float4 is centred in registers (its own mean, the squared deviations of its four values) and merged by
// Chan's update.  Its weights depend on the iteration count alone, 1 / j and 4 (j - 1) / j at the j-th float4, and the
// reciprocal is the hardware's one-instruction approximation: both updates use the same w, so an ulp of it moves
// mean and M2 by an ulp of a deviation.  At the end of the image the run becomes n * (mean - pivot) and M2 + n * (mean - pivot)^2 in
// double.  M2 and the merged differences are deviations; the lane's mean is an fp32 number of the data's size, so the
// hand-over carries its rounding, 2^-24 |mean| per run, into both totals (the cross term 2 (mean - pivot) * sum(x - mean)
// is taken as 0).  That is the error fp32 x - mean has in the apply pass anyway, it has no preferred sign and averages
// over the runs; it is what limits the variance once mean / std reaches the thousands.
__device__ __forceinline__ void stats_slice(const BnArgs& a, int c, int grp, int split, int k, double* sh, double* ts,
                                            double* tss) {
  int lo, hi;
  plane_slice(a.HW, split, k, &lo, &hi);
  const double pivot = group_pivot(a, c, grp);
  double ds = 0.0, dss = 0.0;
  const bool vec = (a.HW & 3) == 0;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  for (int n = group_row(a, grp) + sub; n < group_row(a, grp + 1); n += NT / 64) {
    const float* p = a.x + ((size_t)n * a.C + c) * a.HW;
    float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
    if (vec) {
      for (int i = lo + 4 * lane; i < hi; i += 4 * 64) {
        const float4 v = *reinterpret_cast<const float4*>(p + i);
        const float m4 = ((v.x + v.y) + (v.z + v.w)) * 0.25f;
        const float dx = v.x - m4, dy = v.y - m4, dz = v.z - m4, dw = v.w - m4;
        const float q4 = (dx * dx + dy * dy) + (dz * dz + dw * dw);
        const float delta = m4 - mean;
        const float w = __builtin_amdgcn_rcpf(cnt * 0.25f + 1.0f);       // 1 / j: exact at j = 1, 2, 4, ...
        mean += delta * w;
        m2 += q4 + (delta * delta) * (cnt * w);
        cnt += 4.0f;
      }
    } else {
      for (int i = lo + lane; i < hi; i += 64) {
        const float v = p[i];
        const float delta = v - mean;
        cnt += 1.0f;
        mean += delta * __builtin_amdgcn_rcpf(cnt);
        m2 += delta * (v - mean);
      }
    }
    const double d = (double)mean - pivot;       // fp64 across images; cnt = 0 adds exact zeros
    ds += (double)cnt * d;
    dss += (double)m2 + (double)cnt * d * d;
  }
  *ts = block_sum(ds, sh);
  *tss = block_sum(dss, sh);
}

// mean / variance of one (channel, group) from its totals about the pivot
__device__ __forceinline__ void group_moments(const BnArgs& a, int c, int grp, double ts, double tss, double* mean,
                                              double* var) {
  const double cnt = (double)(group_row(a, grp + 1) - group_row(a, grp)) * (double)a.HW;
  if (!(cnt > 0.0)) { *mean = 0.0; *var = 0.0; return; }      // an empty group of a device-resident table
  const double off = ts / cnt;
  *mean = group_pivot(a, c, grp) + off;
  double v = tss / cnt - off * off;
  *var = v > 0.0 ? v : 0.0;
}
// running statistics: one momentum update per group, in group order = the order of the calls replaced.
// totals(q, &s, &ss) yields group q's sums.
template <typename Totals>
__device__ __forceinline__ void update_running(const BnArgs& a, int c, Totals totals) {
  if (a.run_mean) {
    float rm = a.run_mean[c], rv = a.run_var[c];
    const int tracked = tracked_groups(a);
    for (int q = 0; q < tracked; ++q) {
      double qs, qss, qmean, qvar;
      totals(q, &qs, &qss);
      group_moments(a, c, q, qs, qss, &qmean, &qvar);
      const double qcnt = (double)(group_row(a, q + 1) - group_row(a, q)) * (double)a.HW;
      const double unbiased = qcnt > 1.0 ? qvar * qcnt / (qcnt - 1.0) : qvar;
      rm = (1.0f - a.momentum) * rm + a.momentum * (float)qmean;
      rv = (1.0f - a.momentum) * rv + a.momentum * (float)unbiased;
    }
    a.run_mean[c] = rm;
    a.run_var[c] = rv;
  }
  if (a.batches && c == 0) *a.batches += tracked_groups(a);
}

// forward apply of slice k
__device__ __forceinline__ void apply_slice(const BnArgs& a, int c, int grp, int split, int k, float mean, float scale,
                                            float shift) {
  int lo, hi;
  plane_slice(a.HW, split, k, &lo, &hi);
  const bool vec = (a.HW & 3) == 0;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  for (int n = group_row(a, grp) + sub; n < group_row(a, grp + 1); n += NT / 64) {
    const size_t base = ((size_t)n * a.C + c) * a.HW;
    if (vec) {
      for (int i = lo + 4 * lane; i < hi; i += 4 * 64) {
        const float4 v = *reinterpret_cast<const float4*>(a.x + base + i);
        float4 o;
        o.x = (v.x - mean) * scale + shift; o.y = (v.y - mean) * scale + shift;
        o.z = (v.z - mean) * scale + shift; o.w = (v.w - mean) * scale + shift;
        if (a.res) {
          const float4 r = *reinterpret_cast<const float4*>(a.res + base + i);
          o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        if (a.relu) {
          o.x = o.x > 0.0f ? o.x : 0.0f; o.y = o.y > 0.0f ? o.y : 0.0f;
          o.z = o.z > 0.0f ? o.z : 0.0f; o.w = o.w > 0.0f ? o.w : 0.0f;
        }
        *reinterpret_cast<float4*>(a.y + base + i) = o;
      }
    } else {
      for (int i = lo + lane; i < hi; i += 64) {
        float o = (a.x[base + i] - mean) * scale + shift;
        if (a.res) o += a.res[base + i];
        if (a.relu) o = o > 0.0f ? o : 0.0f;
        a.y[base + i] = o;
      }
    }
  }
}

// ---- where the backward takes g from.  POOL = false: a load of dy.  POOL = true (the encoder stem, bbd_stem_bwd):
// g = [dy, if given] + the gradient that MaxPool2d(3, 2, 1) of y hands back to the pixel, gathered from the pooled
// gradients whose code points at it - the full-size gradient of the pool and its sum with dy are never written.
// pool_grad4: the four pixels (h, w0 .. w0 + 3) of plane `pl`, w0 % 4 == 0 and W % 4 == 0, with the very expressions
// (and association) of maxpool3s2_bwd_kernel's a, b (even rows) and c, d (odd rows), so the sums have its bits.
__device__ __forceinline__ float4 pool_grad4(const BnArgs& a, size_t pl, int h, int w0) {
  const int H = a.HW / a.W, OH = (H - 1) / 2 + 1, OW = a.W >> 1;
  const int oy = h >> 1, ox = w0 >> 1;                        // ox is even, OW is even: ox + 1 < OW
  const size_t r0 = (pl * OH + oy) * OW + ox;
  const bool right = ox + 2 < OW;
  const float2 g0 = *reinterpret_cast<const float2*>(a.gpool + r0);
  const uchar2 k0 = *reinterpret_cast<const uchar2*>(a.code + r0);
  const float g00 = g0.x, g01 = g0.y, g02 = right ? a.gpool[r0 + 2] : 0.0f;
  const int c00 = k0.x, c01 = k0.y, c02 = right ? (int)a.code[r0 + 2] : -1;
  float4 o;
  if (!(h & 1)) {                                             // row 2 oy: window positions 4, 5 of (oy, .), 3 of (oy, . + 1)
    o.x = c00 == 4 ? g00 : 0.0f;
    o.y = (c00 == 5 ? g00 : 0.0f) + (c01 == 3 ? g01 : 0.0f);
    o.z = c01 == 4 ? g01 : 0.0f;
    o.w = (c01 == 5 ? g01 : 0.0f) + (c02 == 3 ? g02 : 0.0f);
    return o;
  }
  const bool down = oy + 1 < OH;                              // row 2 oy + 1: positions 7, 8 of (oy, .), 1, 2 of (oy + 1, .)
  float g10 = 0.0f, g11 = 0.0f, g12 = 0.0f;
  int c10 = -1, c11 = -1, c12 = -1;
  if (down) {
    const float2 g1 = *reinterpret_cast<const float2*>(a.gpool + r0 + OW);
    const uchar2 k1 = *reinterpret_cast<const uchar2*>(a.code + r0 + OW);
    g10 = g1.x; g11 = g1.y; c10 = k1.x; c11 = k1.y;
    if (right) { g12 = a.gpool[r0 + OW + 2]; c12 = a.code[r0 + OW + 2]; }
  }
  o.x = (c00 == 7 ? g00 : 0.0f) + (c10 == 1 ? g10 : 0.0f);
  o.y = ((c00 == 8 ? g00 : 0.0f) + (c01 == 6 ? g01 : 0.0f)) + ((c10 == 2 ? g10 : 0.0f) + (c11 == 0 ? g11 : 0.0f));
  o.z = (c01 == 7 ? g01 : 0.0f) + (c11 == 1 ? g11 : 0.0f);
  o.w = ((c01 == 8 ? g01 : 0.0f) + (c02 == 6 ? g02 : 0.0f)) + ((c11 == 2 ? g11 : 0.0f) + (c12 == 0 ? g12 : 0.0f));
  return o;
}

// g of the float4 at offset i (a multiple of 4) of plane (n, c); base = that plane's offset in x
template <bool POOL>
__device__ __forceinline__ float4 grad4(const BnArgs& a, int n, int c, size_t base, int i) {
  if (!POOL) return *reinterpret_cast<const float4*>(a.dy + base + i);
  const int h = i / a.W;
  float4 g = pool_grad4(a, (size_t)n * a.C + c, h, i - h * a.W);
  if (a.dy) {
    const float4 t = *reinterpret_cast<const float4*>(a.dy + base + i);
    g.x = t.x + g.x; g.y = t.y + g.y; g.z = t.z + g.z; g.w = t.w + g.w;
  }
  return g;
}
// one element (planes that are no multiple of 4 long: never the stem, whose rows are)
template <bool POOL>
__device__ __forceinline__ float grad1(const BnArgs& a, int n, int c, size_t base, int i) {
  if (!POOL) return a.dy[base + i];
  const float4 g = grad4<true>(a, n, c, base, i & ~3);
  return (i & 3) == 0 ? g.x : (i & 3) == 1 ? g.y : (i & 3) == 2 ? g.z : g.w;
}

// backward reduction of slice k: block totals of g = dy * (y > 0) and g * xhat
template <bool POOL>
__device__ __forceinline__ void bwd_reduce_slice(const BnArgs& a, int c, int grp, int split, int k, double* sh, double* tg,
                                                 double* tgx) {
  int lo, hi;
  plane_slice(a.HW, split, k, &lo, &hi);
  const float mean = a.mean[(size_t)grp * a.C + c], invstd = a.invstd[(size_t)grp * a.C + c];
  // ReLU mask without the saved output (no residual in the forward): apply_slice's own expression on x
  const bool remask = a.relu && a.y == nullptr;
  const float scale = remask ? a.gamma[c] * invstd : 0.0f, shift = remask ? a.beta[c] : 0.0f;
  double dg = 0.0, dgx = 0.0;
  const bool vec = (a.HW & 3) == 0;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  for (int n = group_row(a, grp) + sub; n < group_row(a, grp + 1); n += NT / 64) {
    const size_t base = ((size_t)n * a.C + c) * a.HW;
    float sg = 0.0f, sgx = 0.0f;
    if (vec) {
      for (int i = lo + 4 * lane; i < hi; i += 4 * 64) {
        float4 g = grad4<POOL>(a, n, c, base, i);
        const float4 x = *reinterpret_cast<const float4*>(a.x + base + i);
        if (a.relu) {
          float4 y;
          if (remask) {
            y.x = (x.x - mean) * scale + shift; y.y = (x.y - mean) * scale + shift;
            y.z = (x.z - mean) * scale + shift; y.w = (x.w - mean) * scale + shift;
          } else {
            y = *reinterpret_cast<const float4*>(a.y + base + i);
          }
          g.x = y.x > 0.0f ? g.x : 0.0f; g.y = y.y > 0.0f ? g.y : 0.0f;
          g.z = y.z > 0.0f ? g.z : 0.0f; g.w = y.w > 0.0f ? g.w : 0.0f;
        }
        sg += (g.x + g.y) + (g.z + g.w);
        sgx += (g.x * ((x.x - mean) * invstd) + g.y * ((x.y - mean) * invstd)) +
               (g.z * ((x.z - mean) * invstd) + g.w * ((x.w - mean) * invstd));
      }
    } else {
      for (int i = lo + lane; i < hi; i += 64) {
        float g = grad1<POOL>(a, n, c, base, i);
        if (a.relu && !((remask ? (a.x[base + i] - mean) * scale + shift : a.y[base + i]) > 0.0f)) g = 0.0f;
        sg += g;
        sgx += g * ((a.x[base + i] - mean) * invstd);
      }
    }
    dg += (double)sg;
    dgx += (double)sgx;
  }
  *tg = block_sum(dg, sh);
  *tgx = block_sum(dgx, sh);
}

// backward apply of slice k
template <bool POOL>
__device__ __forceinline__ void bwd_apply_slice(const BnArgs& a, int c, int grp, int split, int k, float mg, float mgx,
                                                float kk) {
  const float mean = a.mean[(size_t)grp * a.C + c], invstd = a.invstd[(size_t)grp * a.C + c];
  const bool remask = a.relu && a.y == nullptr;
  const float scale = remask ? a.gamma[c] * invstd : 0.0f, shift = remask ? a.beta[c] : 0.0f;
  int lo, hi;
  plane_slice(a.HW, split, k, &lo, &hi);
  const bool vec = (a.HW & 3) == 0;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  for (int n = group_row(a, grp) + sub; n < group_row(a, grp + 1); n += NT / 64) {
    const size_t base = ((size_t)n * a.C + c) * a.HW;
    if (vec) {
      for (int i = lo + 4 * lane; i < hi; i += 4 * 64) {
        float4 g = grad4<POOL>(a, n, c, base, i);
        const float4 x = *reinterpret_cast<const float4*>(a.x + base + i);
        if (a.relu) {
          float4 y;
          if (remask) {
            y.x = (x.x - mean) * scale + shift; y.y = (x.y - mean) * scale + shift;
            y.z = (x.z - mean) * scale + shift; y.w = (x.w - mean) * scale + shift;
          } else {
            y = *reinterpret_cast<const float4*>(a.y + base + i);
          }
          g.x = y.x > 0.0f ? g.x : 0.0f; g.y = y.y > 0.0f ? g.y : 0.0f;
          g.z = y.z > 0.0f ? g.z : 0.0f; g.w = y.w > 0.0f ? g.w : 0.0f;
        }
        if (a.dres) *reinterpret_cast<float4*>(a.dres + base + i) = g;
        float4 o;
        o.x = kk * (g.x - mg - ((x.x - mean) * invstd) * mgx);
        o.y = kk * (g.y - mg - ((x.y - mean) * invstd) * mgx);
        o.z = kk * (g.z - mg - ((x.z - mean) * invstd) * mgx);
        o.w = kk * (g.w - mg - ((x.w - mean) * invstd) * mgx);
        *reinterpret_cast<float4*>(a.dx + base + i) = o;
      }
    } else {
      for (int i = lo + lane; i < hi; i += 64) {
        float g = grad1<POOL>(a, n, c, base, i);
        if (a.relu && !((remask ? (a.x[base + i] - mean) * scale + shift : a.y[base + i]) > 0.0f)) g = 0.0f;
        if (a.dres) a.dres[base + i] = g;
        a.dx[base + i] = kk * (g - mg - ((a.x[base + i] - mean) * invstd) * mgx);
      }
    }
  }
}

// per-(channel, group) sums of the two partial columns written by the two-launch reduction kernels
__device__ __forceinline__ void group_totals(const BnArgs& a, int c, int grp, double* t0, double* t1) {
  double s0 = 0.0, s1 = 0.0;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  for (int k = 0; k < split; ++k) {
    s0 += a.part[(((size_t)c * a.G + grp) * a.split + k) * 2];
    s1 += a.part[(((size_t)c * a.G + grp) * a.split + k) * 2 + 1];
  }
  *t0 = s0; *t1 = s1;
}

// ---- two launches per direction: grid (slices of the largest group, C, G)
__global__ __launch_bounds__(NT) void bn_stats_kernel(BnArgs a) {
  __shared__ double sh[4];
  const int c = blockIdx.y, grp = blockIdx.z;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  if ((int)blockIdx.x >= split) return;      // the grid is sized for the largest group
  double ts, tss;
  stats_slice(a, c, grp, split, blockIdx.x, sh, &ts, &tss);
  if (threadIdx.x == 0) {
    a.part[(((size_t)c * a.G + grp) * a.split + blockIdx.x) * 2] = ts;
    a.part[(((size_t)c * a.G + grp) * a.split + blockIdx.x) * 2 + 1] = tss;
  }
}

__global__ __launch_bounds__(NT) void bn_apply_kernel(BnArgs a) {
  __shared__ float s_mean, s_scale, s_shift;
  const int c = blockIdx.y, grp = blockIdx.z;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  if ((int)blockIdx.x >= split) return;
  if (threadIdx.x == 0) {
    double ts, tss, mean, var;
    group_totals(a, c, grp, &ts, &tss);
    group_moments(a, c, grp, ts, tss, &mean, &var);
    const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
    s_mean = (float)mean;
    s_scale = a.gamma[c] * invstd;
    s_shift = a.beta[c];
    if (blockIdx.x == 0) {
      a.mean[(size_t)grp * a.C + c] = (float)mean;
      a.invstd[(size_t)grp * a.C + c] = invstd;
      if (grp == 0) update_running(a, c, [&](int q, double* s0, double* s1) { group_totals(a, c, q, s0, s1); });
    }
  }
  __syncthreads();
  apply_slice(a, c, grp, split, blockIdx.x, s_mean, s_scale, s_shift);
}

// ---- encoder stem, forward: bn_stats_kernel as above, then apply + ReLU + MaxPool2d(3, 2, 1) in one pass.
// W % 4 == 0, so OW = W / 2 and a float4 of a row holds the windows of two pooled columns but for the pixel to its left.
// A task is a strip of 4 columns through STEM_TP pooled rows of one image: it loads input rows 2 p0 - 1 .. 2 p0 + 2 TP - 1
// (all in flight together), owns the last 2 TP of them (the first is the halo, the previous tile's row, fetched a second
// time through the cache) and walks down them.  Tasks are numbered image-major, then tile, then strip, so a wave's lanes
// read and write runs of a row: float4 of x and y, float2 of pooled values, two code bytes.  The left neighbour's last
// value comes from the lane below; a wave's first lane loads it.  Grid (task groups of the largest group, C, G).
constexpr int STEM_TP = 4;

__device__ __forceinline__ float stem_y(float v, float mean, float scale, float shift) {
  const float o = (v - mean) * scale + shift;        // apply_slice's expression
  return o > 0.0f ? o : 0.0f;
}
// maxpool3s2_fwd_kernel's rule: the first maximum in row-major window order, a NaN replaces the running maximum
__device__ __forceinline__ void stem_take(float v, int pos, float* best, int* bc) {
  if (*bc < 0 || v > *best || v != v) { *best = v; *bc = pos; }
}

__global__ __launch_bounds__(NT) void stem_apply_pool_kernel(BnArgs a) {
  __shared__ float s_mean, s_scale, s_shift;
  const int c = blockIdx.y, grp = blockIdx.z;
  const int first = group_row(a, grp), rows = group_row(a, grp + 1) - first;
  const int W = a.W, H = a.HW / W, OH = (H - 1) / 2 + 1, OW = W >> 1, CW = W >> 2;
  const int tiles = (OH + STEM_TP - 1) / STEM_TP;
  const long long tasks = (long long)rows * tiles * CW;
  if (blockIdx.x > 0 && (long long)blockIdx.x * NT >= tasks) return;      // the grid is sized for the largest group
  if (threadIdx.x == 0) {
    double ts, tss, mean, var;
    group_totals(a, c, grp, &ts, &tss);
    group_moments(a, c, grp, ts, tss, &mean, &var);
    const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
    s_mean = (float)mean;
    s_scale = a.gamma[c] * invstd;
    s_shift = a.beta[c];
    if (blockIdx.x == 0) {
      a.mean[(size_t)grp * a.C + c] = (float)mean;
      a.invstd[(size_t)grp * a.C + c] = invstd;
      if (grp == 0) update_running(a, c, [&](int q, double* s0, double* s1) { group_totals(a, c, q, s0, s1); });
    }
  }
  __syncthreads();
  const float mean = s_mean, scale = s_scale, shift = s_shift;
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  const bool live = t < tasks;
  // a dead lane keeps in step with the wave (the exchange below) on the coordinates of task 0; it loads and stores nothing
  const long long tt = live ? t : 0;
  const int img = (int)(tt / ((long long)tiles * CW));
  const int rem = (int)(tt - (long long)img * tiles * CW);
  const int tile = rem / CW, strip = rem - tile * CW;
  const int p0 = tile * STEM_TP, w0 = strip << 2;
  const size_t pl = (size_t)(first + img) * a.C + c;
  const float* xp = a.x + pl * a.HW;
  constexpr int NR = 2 * STEM_TP + 1;
  float4 v[NR];
  float lf[NR];
  const bool own_left = strip > 0 && (threadIdx.x & 63) == 0;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int h = 2 * p0 - 1 + r;
    const bool in = live && h >= 0 && h < H;
    v[r] = in ? *reinterpret_cast<const float4*>(xp + (size_t)h * W + w0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    lf[r] = (in && own_left) ? xp[(size_t)h * W + w0 - 1] : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    v[r].x = stem_y(v[r].x, mean, scale, shift); v[r].y = stem_y(v[r].y, mean, scale, shift);
    v[r].z = stem_y(v[r].z, mean, scale, shift); v[r].w = stem_y(v[r].w, mean, scale, shift);
    const float below = __shfl_up(v[r].w, 1, 64);              // the strip to the left, when it is in this wave
    lf[r] = own_left ? stem_y(lf[r], mean, scale, shift) : below;
  }
  if (!live) return;
  if (a.y) {
    float* yp = a.y + pl * a.HW;
#pragma unroll
    for (int r = 1; r < NR; ++r) {
      const int h = 2 * p0 - 1 + r;
      if (h < H) *reinterpret_cast<float4*>(yp + (size_t)h * W + w0) = v[r];
    }
  }
#pragma unroll
  for (int j = 0; j < STEM_TP; ++j) {
    const int oy = p0 + j;
    if (oy >= OH) break;
    float b0 = -INFINITY, b1 = -INFINITY;
    int k0 = -1, k1 = -1;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int h = 2 * oy - 1 + dy;
      if (h < 0 || h >= H) continue;
      const float4 q = v[2 * j + dy];
      if (strip > 0) stem_take(lf[2 * j + dy], dy * 3, &b0, &k0);
      stem_take(q.x, dy * 3 + 1, &b0, &k0);
      stem_take(q.y, dy * 3 + 2, &b0, &k0);
      stem_take(q.y, dy * 3, &b1, &k1);
      stem_take(q.z, dy * 3 + 1, &b1, &k1);
      stem_take(q.w, dy * 3 + 2, &b1, &k1);
    }
    const size_t o = (pl * OH + oy) * OW + 2 * strip;
    *reinterpret_cast<float2*>(a.pooled + o) = make_float2(b0, b1);
    *reinterpret_cast<uchar2*>(a.code + o) = make_uchar2((unsigned char)k0, (unsigned char)k1);
  }
}

template <bool POOL>
__global__ __launch_bounds__(NT) void bn_bwd_reduce_kernel(BnArgs a) {
  __shared__ double sh[4];
  const int c = blockIdx.y, grp = blockIdx.z;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  if ((int)blockIdx.x >= split) return;
  double tg, tgx;
  bwd_reduce_slice<POOL>(a, c, grp, split, blockIdx.x, sh, &tg, &tgx);
  if (threadIdx.x == 0) {
    a.part[(((size_t)c * a.G + grp) * a.split + blockIdx.x) * 2] = tg;
    a.part[(((size_t)c * a.G + grp) * a.split + blockIdx.x) * 2 + 1] = tgx;
  }
}

template <bool POOL>
__global__ __launch_bounds__(NT) void bn_bwd_apply_kernel(BnArgs a) {
  __shared__ float s_k[3];
  const int c = blockIdx.y, grp = blockIdx.z;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  if ((int)blockIdx.x >= split) return;
  if (threadIdx.x == 0) {
    double tg, tgx;
    group_totals(a, c, grp, &tg, &tgx);
    const double cnt = (double)(group_row(a, grp + 1) - group_row(a, grp)) * (double)a.HW;
    s_k[0] = (float)(tg / cnt);
    s_k[1] = (float)(tgx / cnt);
    s_k[2] = a.gamma[c] * a.invstd[(size_t)grp * a.C + c];
    if (blockIdx.x == 0 && grp == 0) {      // parameter gradients: sums over every group, in group order
      double sg = tg, sgx = tgx;
      for (int q = 1; q < a.G; ++q) {
        double qg, qgx;
        group_totals(a, c, q, &qg, &qgx);
        sg += qg; sgx += qgx;
      }
      a.dgamma[c] = (float)sgx;
      a.dbeta[c] = (float)sg;
    }
  }
  __syncthreads();
  bwd_apply_slice<POOL>(a, c, grp, split, blockIdx.x, s_k[0], s_k[1], s_k[2]);
}

// ---- one launch per direction for small activations: grid (1, C, G), the workgroup owns its whole (channel, group).
// `part` then holds one (total, total) pair per (channel, group): [C][G][2].  With more than one group the
// cross-group results (running statistics; parameter gradients) come from a C-thread follow-up launch.
__global__ __launch_bounds__(NT) void bn_fwd_small_kernel(BnArgs a) {
  __shared__ double sh[4];
  __shared__ float s_mean, s_scale, s_shift;
  const int c = blockIdx.y, grp = blockIdx.z;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  double ts = 0.0, tss = 0.0;
  for (int k = 0; k < split; ++k) {          // the same slices, added in the same order, as the two-launch form
    double ks, kss;
    stats_slice(a, c, grp, split, k, sh, &ks, &kss);
    ts += ks; tss += kss;
  }
  if (threadIdx.x == 0) {
    double mean, var;
    group_moments(a, c, grp, ts, tss, &mean, &var);
    const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
    s_mean = (float)mean;
    s_scale = a.gamma[c] * invstd;
    s_shift = a.beta[c];
    a.mean[(size_t)grp * a.C + c] = (float)mean;
    a.invstd[(size_t)grp * a.C + c] = invstd;
    if (a.G == 1) {
      update_running(a, c, [&](int, double* s0, double* s1) { *s0 = ts; *s1 = tss; });
    } else {
      a.part[((size_t)c * a.G + grp) * 2] = ts;
      a.part[((size_t)c * a.G + grp) * 2 + 1] = tss;
    }
  }
  __syncthreads();
  for (int k = 0; k < split; ++k) apply_slice(a, c, grp, split, k, s_mean, s_scale, s_shift);
}
__global__ __launch_bounds__(64) void bn_running_small_kernel(BnArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.C) return;
  update_running(a, c, [&](int q, double* s0, double* s1) {
    *s0 = a.part[((size_t)c * a.G + q) * 2];
    *s1 = a.part[((size_t)c * a.G + q) * 2 + 1];
  });
}

__global__ __launch_bounds__(NT) void bn_bwd_small_kernel(BnArgs a) {
  __shared__ double sh[4];
  __shared__ float s_k[3];
  const int c = blockIdx.y, grp = blockIdx.z;
  const int split = pick_split(group_row(a, grp + 1) - group_row(a, grp), a.HW);
  double tg = 0.0, tgx = 0.0;
  for (int k = 0; k < split; ++k) {
    double kg, kgx;
    bwd_reduce_slice<false>(a, c, grp, split, k, sh, &kg, &kgx);
    tg += kg; tgx += kgx;
  }
  if (threadIdx.x == 0) {
    const double cnt = (double)(group_row(a, grp + 1) - group_row(a, grp)) * (double)a.HW;
    s_k[0] = (float)(tg / cnt);
    s_k[1] = (float)(tgx / cnt);
    s_k[2] = a.gamma[c] * a.invstd[(size_t)grp * a.C + c];
    if (a.G == 1) {
      a.dgamma[c] = (float)tgx;
      a.dbeta[c] = (float)tg;
    } else {
      a.part[((size_t)c * a.G + grp) * 2] = tg;
      a.part[((size_t)c * a.G + grp) * 2 + 1] = tgx;
    }
  }
  __syncthreads();
  for (int k = 0; k < split; ++k) bwd_apply_slice<false>(a, c, grp, split, k, s_k[0], s_k[1], s_k[2]);
}
__global__ __launch_bounds__(64) void bn_param_grad_small_kernel(BnArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.C) return;
  double sg = 0.0, sgx = 0.0;
  for (int q = 0; q < a.G; ++q) {            // group order, like bn_bwd_apply_kernel
    sg += a.part[((size_t)c * a.G + q) * 2];
    sgx += a.part[((size_t)c * a.G + q) * 2 + 1];
  }
  a.dgamma[c] = (float)sgx;
  a.dbeta[c] = (float)sg;
}

// ---------------------------------------------------------------------------------------------
// ReflectionPad2d(1) (layers.py:118-133, every decoder convolution) and MaxPool2d(3, 2, 1)
// (networks/resnet_encoder.py: the torchvision stem), forward and gather-form backward: no atomics,
// deterministic, one coalesced pass.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect1(int i, int n) {   // index into the un-padded axis for padded index i
  i -= 1;
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

// Row-tiled launches: a workgroup of 64 x 4 threads owns 4 rows of one plane (blockIdx.y = plane), the
// 64 lanes of a wave sweep the row, so every access is a coalesced run with no index division.
constexpr int RW = 64, RR = 4;

__global__ __launch_bounds__(RW * RR) void reflect_pad1_fwd_kernel(const float* __restrict__ in,
                                                                   float* __restrict__ out, int H, int W) {
  const int PH = H + 2, PW = W + 2;
  const int py = blockIdx.x * RR + threadIdx.y;
  if (py >= PH) return;
  const size_t pl = blockIdx.y;
  const float* src = in + (pl * H + reflect1(py, H)) * W;
  float* dst = out + (pl * PH + py) * PW;
  for (int px = threadIdx.x; px < PW; px += RW) dst[px] = src[reflect1(px, W)];
}

// grad_in[y][x] = sum of grad_out over every padded position that reads (y, x)
__global__ __launch_bounds__(RW * RR) void reflect_pad1_bwd_kernel(const float* __restrict__ gout,
                                                                   float* __restrict__ gin, int H, int W) {
  const int PH = H + 2, PW = W + 2;
  const int y = blockIdx.x * RR + threadIdx.y;
  if (y >= H) return;
  const size_t pl = blockIdx.y;
  const float* g = gout + pl * PH * PW;
  float* dst = gin + (pl * H + y) * W;
  int ys[3], ny = 0;                       // padded rows that map onto y (wave-uniform)
  ys[ny++] = y + 1;
  if (y == 1) ys[ny++] = 0;
  if (y == H - 2) ys[ny++] = PH - 1;
  for (int x = threadIdx.x; x < W; x += RW) {
    float acc = 0.0f;
    for (int a = 0; a < ny; ++a) {
      const float* row = g + (size_t)ys[a] * PW;
      acc += row[x + 1];
      if (x == 1) acc += row[0];
      if (x == W - 2) acc += row[PW - 1];
    }
    dst[x] = acc;
  }
}

// ---- decoder glue: nearest x2 up-sampling + skip concatenation + ReflectionPad2d(1) as ONE pass -------------
// (reference networks/depth_decoder.py:44-50: `upsample(x)`, `torch.cat([x, skip], 1)`, then the next ConvBlock's
// ReflectionPad2d(1), layers.py:118-133 - three full-tensor round trips in eager mode).  out[n, c, py, px] for the
// padded (H+2)x(W+2) image of the concatenation; H = 2h, W = 2w.
__global__ __launch_bounds__(RW * RR) void upcat_pad_fwd_kernel(const float* __restrict__ x, const float* __restrict__ skip,
                                                                float* __restrict__ out, int C1, int C2, int h, int w) {
  const int H = 2 * h, W = 2 * w, PH = H + 2, PW = W + 2;
  const int py = blockIdx.x * RR + threadIdx.y;
  if (py >= PH) return;
  const int pl = blockIdx.y, n = pl / (C1 + C2), c = pl - n * (C1 + C2);
  const int yy = reflect1(py, H);
  float* dst = out + ((size_t)pl * PH + py) * PW;
  if (c < C1) {
    const float* src = x + (((size_t)n * C1 + c) * h + (yy >> 1)) * w;
    for (int px = threadIdx.x; px < PW; px += RW) dst[px] = src[reflect1(px, W) >> 1];
  } else {
    const float* src = skip + (((size_t)n * C2 + (c - C1)) * H + yy) * W;
    for (int px = threadIdx.x; px < PW; px += RW) dst[px] = src[reflect1(px, W)];
  }
}

// sum of grad_out over every padded position that reads image position (y, x)  (1, 2, 3, 4, 6 or 9 terms)
__device__ __forceinline__ float pad1_adjoint(const float* __restrict__ g, int y, int x, int H, int W) {
  const int PW = W + 2;
  int rows[3], nr = 0;
  rows[nr++] = y + 1;
  if (y == 1) rows[nr++] = 0;
  if (y == H - 2) rows[nr++] = H + 1;
  float acc = 0.0f;
  for (int a = 0; a < nr; ++a) {
    const float* row = g + (size_t)rows[a] * PW;
    acc += row[x + 1];
    if (x == 1) acc += row[0];
    if (x == W - 2) acc += row[PW - 1];
  }
  return acc;
}

__global__ __launch_bounds__(RW * RR) void upcat_pad_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gx,
                                                                float* __restrict__ gskip, int C1, int C2, int h, int w) {
  const int H = 2 * h, W = 2 * w, PH = H + 2, PW = W + 2;
  const int pl = blockIdx.y, n = pl / (C1 + C2), c = pl - n * (C1 + C2);
  const float* g = gout + (size_t)pl * PH * PW;
  if (c < C1) {                                  // low-resolution rows: each output sums its 2x2 up-sampled block
    const int i = blockIdx.x * RR + threadIdx.y;
    if (i >= h) return;
    float* dst = gx + (((size_t)n * C1 + c) * h + i) * w;
    for (int j = threadIdx.x; j < w; j += RW)
      dst[j] = (pad1_adjoint(g, 2 * i, 2 * j, H, W) + pad1_adjoint(g, 2 * i, 2 * j + 1, H, W)) +
               (pad1_adjoint(g, 2 * i + 1, 2 * j, H, W) + pad1_adjoint(g, 2 * i + 1, 2 * j + 1, H, W));
  } else {
    for (int y = blockIdx.x * RR + threadIdx.y; y < H; y += gridDim.x * RR) {
      float* dst = gskip + (((size_t)n * C2 + (c - C1)) * H + y) * W;
      for (int xx = threadIdx.x; xx < W; xx += RW) dst[xx] = pad1_adjoint(g, y, xx, H, W);
    }
  }
}

// ---- decoder glue: bias + ELU in place on the convolution's output, and its backward with the bias gradient ------
// (layers.ConvBlock = Conv3x3 + ELU, layers.py:103-115; eager PyTorch-ROCm launches conv, a bias add and ELU forward,
// and ELU-backward plus a bias reduction backward).  ELU(alpha = 1): y = v > 0 ? v : expm1(v); dy/dv = y > 0 ? 1 : y + 1.
__global__ __launch_bounds__(NT) void bias_elu_fwd_kernel(float* __restrict__ y, const float* __restrict__ bias, int C, int HW,
                                                          size_t total) {
  for (size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) * 4; i < total; i += (size_t)gridDim.x * NT * 4) {
    const int c = (int)((i / HW) % C);            // HW % 4 == 0: the four elements share a channel
    const float b = bias[c];
    float4 v = *reinterpret_cast<float4*>(y + i);
    v.x += b; v.y += b; v.z += b; v.w += b;
    v.x = v.x > 0.0f ? v.x : expm1f(v.x); v.y = v.y > 0.0f ? v.y : expm1f(v.y);
    v.z = v.z > 0.0f ? v.z : expm1f(v.z); v.w = v.w > 0.0f ? v.w : expm1f(v.w);
    *reinterpret_cast<float4*>(y + i) = v;
  }
}

__global__ __launch_bounds__(NT) void bias_elu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gy,
                                                          float* __restrict__ gx, double* __restrict__ part, int N, int C,
                                                          int HW, int split) {
  __shared__ double sh[4];
  const int c = blockIdx.y;
  int len = (HW + split - 1) / split;
  len = (len + 3) & ~3;
  const int lo = blockIdx.x * len, hi = min(HW, lo + len);
  double acc = 0.0;
  for (int n = 0; n < N; ++n) {
    const size_t base = ((size_t)n * C + c) * HW;
    float s = 0.0f;
    for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += 4 * NT) {
      const float4 o = *reinterpret_cast<const float4*>(y + base + i);
      float4 g = *reinterpret_cast<const float4*>(gy + base + i);
      g.x = o.x > 0.0f ? g.x : g.x * (o.x + 1.0f); g.y = o.y > 0.0f ? g.y : g.y * (o.y + 1.0f);
      g.z = o.z > 0.0f ? g.z : g.z * (o.z + 1.0f); g.w = o.w > 0.0f ? g.w : g.w * (o.w + 1.0f);
      *reinterpret_cast<float4*>(gx + base + i) = g;
      s += (g.x + g.y) + (g.z + g.w);
    }
    acc += (double)s;
  }
  const double t = block_sum(acc, sh);
  if (threadIdx.x == 0) part[(size_t)c * split + blockIdx.x] = t;
}

__global__ __launch_bounds__(64) void bias_grad_final_kernel(const double* __restrict__ part, float* __restrict__ gbias, int C,
                                                             int split) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int k = 0; k < split; ++k) s += part[(size_t)c * split + k];
  gbias[c] = (float)s;
}

// ---- decoder glue with the ConvBlock's bias + ELU inside (bbd_upcat_pad_act_*, bbd_bias_elu_pad_*) -------------------
// A decoder level is conv -> bias + ELU -> up-sample + concat + pad -> conv -> bias + ELU -> pad (the next level's).  The
// separate passes above move every convolution output through HBM once more for the activation and again for the copy
// into the next padded input; here the activation rides on the copy.  Numbers are those of the composition: the same
// ELU expression, pad1_adjoint's row / centre / left / right order, the (a + b) + (c + d) block sum, g * (y + 1.0f).
//
// All four kernels are driven by the UN-padded rows: a wave owns one source row (several short ones: glue_row below), reads it with 16-byte accesses and
// writes (forward) or gathers (backward) the one to three padded rows that mirror it.  A padded row starts 8-byte
// aligned (its pitch W + 2 is even) and its interior one float later, so the padded side moves 16 bytes per lane at
// 4-byte alignment - global accesses wider than a dword need dword alignment only - and the two border columns are
// single stores / loads of the lanes that hold columns 1 and W - 2.  Rows that are no multiple of four floats long (or
// whose tensors are not 16-byte aligned) take one element per lane.
struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };     // four floats at float alignment

__device__ __forceinline__ float elu1(float v) { return v > 0.0f ? v : expm1f(v); }                  // bias_elu_fwd_kernel's
__device__ __forceinline__ float elu1_grad(float g, float y) { return y > 0.0f ? g : g * (y + 1.0f); }   // bias_elu_bwd_kernel's

// image columns x0 .. x0 + 3 of one unpadded row into a padded row: the interior, and the border column that mirrors
// column 1 / W - 2 where the run holds it.  x0 % 4 == 0, W % 4 == 0.
__device__ __forceinline__ void pad_row_store4(float* __restrict__ prow, int x0, int W, const float4& v) {
  F4U o; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
  *reinterpret_cast<F4U*>(prow + x0 + 1) = o;
  if (x0 == 0) prow[0] = v.y;
  if (x0 + 4 == W) prow[W + 1] = v.z;
}
__device__ __forceinline__ void pad_row_store1(float* __restrict__ prow, int x, int W, float v) {
  prow[x + 1] = v;
  if (x == 1) prow[0] = v;
  if (x == W - 2) prow[W + 1] = v;
}

// pad1_adjoint for K = 4 or 8 neighbouring columns x0 .. x0 + K - 1 of image row y (x0 % K == 0, W % K == 0): per
// column the additions of pad1_adjoint in its order, the centre terms fetched as 16-byte runs.
template <int K>
__device__ __forceinline__ void pad1_adjoint_row(const float* __restrict__ row, int x0, int W, float (&acc)[K]) {
  float m[K];
#pragma unroll
  for (int v = 0; v < K / 4; ++v) {
    const F4U t = *reinterpret_cast<const F4U*>(row + x0 + 1 + 4 * v);
    m[4 * v] = t.x; m[4 * v + 1] = t.y; m[4 * v + 2] = t.z; m[4 * v + 3] = t.w;
  }
#pragma unroll
  for (int e = 0; e < K; ++e) {
    acc[e] += m[e];
    if (x0 + e == 1) acc[e] += row[0];
    if (x0 + e == W - 2) acc[e] += row[W + 1];
  }
}
template <int K>
__device__ __forceinline__ void pad1_adjoint_run(const float* __restrict__ g, int y, int x0, int H, int W, float (&acc)[K]) {
  const int PW = W + 2;
#pragma unroll
  for (int e = 0; e < K; ++e) acc[e] = 0.0f;
  pad1_adjoint_row<K>(g + (size_t)(y + 1) * PW, x0, W, acc);
  if (y == 1) pad1_adjoint_row<K>(g, x0, W, acc);
  if (y == H - 2) pad1_adjoint_row<K>(g + (size_t)(H + 1) * PW, x0, W, acc);
}

// block total of a 64 x RR workgroup (threadIdx.y = wave); every thread of the block calls it
__device__ __forceinline__ double block_sum_rows(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if (threadIdx.x == 0) sh[threadIdx.y] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
static_assert(RR == 4 && RR == BBD_GLUE_ROWS, "block_sum_rows adds four waves; the partial count is the header's");

// Short rows: the decoder's coarse levels have rows of 20 or 40 floats - five or ten lanes' worth of float4s.  A wave
// then takes 64 >> lg rows at once with 1 << lg lanes along each (lg chosen by the host from the row length, 6 = the
// whole wave along one row); shifts and masks only.  A workgroup covers RR << (6 - lg) consecutive rows.
__device__ __forceinline__ int glue_row(int lg) { return ((blockIdx.x * RR + threadIdx.y) << (6 - lg)) + (threadIdx.x >> lg); }
__device__ __forceinline__ int glue_lane(int lg) { return threadIdx.x & ((1 << lg) - 1); }

// out = ReflectionPad2d(1)(cat(nearest_x2(ELU(z + bias)), skip)).  Source row i of z is image rows 2i, 2i + 1 = padded
// rows 2i + 1, 2i + 2, and also padded row 0 (i = 0) and 2h + 1 (i = h - 1); the activation is computed once per element.
__global__ __launch_bounds__(RW * RR) void upcat_pad_act_fwd_kernel(const float* __restrict__ z, const float* __restrict__ bias,
                                                                    const float* __restrict__ skip, float* __restrict__ out,
                                                                    int C1, int C2, int h, int w, int vec_z, int vec_skip, int lg_z,
                                                                    int lg_skip) {
  const int H = 2 * h, W = 2 * w, PH = H + 2, PW = W + 2;
  const int pl = blockIdx.y, n = pl / (C1 + C2), c = pl - n * (C1 + C2);
  float* dst = out + (size_t)pl * PH * PW;
  if (c < C1) {
    const int i = glue_row(lg_z);
    if (i >= h) return;
    const float b = bias[c];
    const float* src = z + (((size_t)n * C1 + c) * h + i) * w;
    int rows[4], nr = 0;                     // the padded rows that show source row i (offsets: a plane is below 2^31)
    rows[nr++] = (2 * i + 1) * PW;
    rows[nr++] = (2 * i + 2) * PW;
    if (i == 0) rows[nr++] = 0;
    if (i == h - 1) rows[nr++] = (H + 1) * PW;
    if (vec_z) {
      for (int j0 = 4 * glue_lane(lg_z); j0 < w; j0 += 4 << lg_z) {
        float4 a = *reinterpret_cast<const float4*>(src + j0);
        a.x = elu1(a.x + b); a.y = elu1(a.y + b); a.z = elu1(a.z + b); a.w = elu1(a.w + b);
        F4U lo, hi;
        lo.x = a.x; lo.y = a.x; lo.z = a.y; lo.w = a.y;
        hi.x = a.z; hi.y = a.z; hi.z = a.w; hi.w = a.w;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r < nr) {
            float* p = dst + rows[r];
            *reinterpret_cast<F4U*>(p + 2 * j0 + 1) = lo;
            *reinterpret_cast<F4U*>(p + 2 * j0 + 5) = hi;
            if (j0 == 0) p[0] = a.x;
            if (j0 + 4 == w) p[PW - 1] = a.w;
          }
        }
      }
    } else {
      for (int j = glue_lane(lg_z); j < w; j += 1 << lg_z) {
        const float a = elu1(src[j] + b);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r < nr) {
            float* p = dst + rows[r];
            p[2 * j + 1] = a;
            p[2 * j + 2] = a;
            if (j == 0) p[0] = a;
            if (j == w - 1) p[PW - 1] = a;
          }
        }
      }
    }
  } else {
    for (int y = glue_row(lg_skip); y < H; y += (gridDim.x * RR) << (6 - lg_skip)) {
      const float* src = skip + (((size_t)n * C2 + (c - C1)) * H + y) * W;
      float* mid = dst + (size_t)(y + 1) * PW;
      float* top = y == 1 ? dst : nullptr;
      float* bot = y == H - 2 ? dst + (size_t)(H + 1) * PW : nullptr;
      if (vec_skip) {
        for (int x0 = 4 * glue_lane(lg_skip); x0 < W; x0 += 4 << lg_skip) {
          const float4 v = *reinterpret_cast<const float4*>(src + x0);
          pad_row_store4(mid, x0, W, v);
          if (top) pad_row_store4(top, x0, W, v);
          if (bot) pad_row_store4(bot, x0, W, v);
        }
      } else {
        for (int x = glue_lane(lg_skip); x < W; x += 1 << lg_skip) {
          const float v = src[x];
          pad_row_store1(mid, x, W, v);
          if (top) pad_row_store1(top, x, W, v);
          if (bot) pad_row_store1(bot, x, W, v);
        }
      }
    }
  }
}

// grad_z = g * ELU'(y), y = ELU(z + bias) recomputed, g = upcat_pad_bwd_kernel's 2x2 sum; grad_skip as there.  A lane of
// the 16-byte form owns four low-resolution columns: the eight padded columns 2 j0 + 1 .. 2 j0 + 8 of a padded row are
// two 16-byte loads (one lane fetches the pair 2j + 1, 2j + 2 together).  part[c][n * gridDim.x + blockIdx.x] = the
// block's sum of grad_z in double.
__global__ __launch_bounds__(RW * RR) void upcat_pad_act_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ z,
                                                                    const float* __restrict__ bias, float* __restrict__ gz,
                                                                    float* __restrict__ gskip, double* __restrict__ part,
                                                                    int N, int C1, int C2, int h, int w, int vec_z,
                                                                    int vec_skip, int lg_z, int lg_skip) {
  __shared__ double sh[RR];
  const int H = 2 * h, W = 2 * w, PH = H + 2, PW = W + 2;
  const int pl = blockIdx.y, n = pl / (C1 + C2), c = pl - n * (C1 + C2);
  const float* g = gout + (size_t)pl * PH * PW;
  if (c < C1) {
    const int i = glue_row(lg_z);
    double acc = 0.0;
    if (i < h) {
      const float b = bias[c];
      const size_t base = (((size_t)n * C1 + c) * h + i) * w;
      if (vec_z) {
        for (int j0 = 4 * glue_lane(lg_z); j0 < w; j0 += 4 << lg_z) {
          float a0[8], a1[8];
          pad1_adjoint_run<8>(g, 2 * i, 2 * j0, H, W, a0);
          pad1_adjoint_run<8>(g, 2 * i + 1, 2 * j0, H, W, a1);
          float4 y = *reinterpret_cast<const float4*>(z + base + j0);
          y.x = elu1(y.x + b); y.y = elu1(y.y + b); y.z = elu1(y.z + b); y.w = elu1(y.w + b);
          float4 r;
          r.x = elu1_grad((a0[0] + a0[1]) + (a1[0] + a1[1]), y.x);
          r.y = elu1_grad((a0[2] + a0[3]) + (a1[2] + a1[3]), y.y);
          r.z = elu1_grad((a0[4] + a0[5]) + (a1[4] + a1[5]), y.z);
          r.w = elu1_grad((a0[6] + a0[7]) + (a1[6] + a1[7]), y.w);
          *reinterpret_cast<float4*>(gz + base + j0) = r;
          acc += (double)((r.x + r.y) + (r.z + r.w));
        }
      } else {
        for (int j = glue_lane(lg_z); j < w; j += 1 << lg_z) {
          const float gg = (pad1_adjoint(g, 2 * i, 2 * j, H, W) + pad1_adjoint(g, 2 * i, 2 * j + 1, H, W)) +
                           (pad1_adjoint(g, 2 * i + 1, 2 * j, H, W) + pad1_adjoint(g, 2 * i + 1, 2 * j + 1, H, W));
          const float r = elu1_grad(gg, elu1(z[base + j] + b));
          gz[base + j] = r;
          acc += (double)r;
        }
      }
    }
    const double t = block_sum_rows(acc, sh);
    if (threadIdx.x == 0 && threadIdx.y == 0) part[((size_t)c * N + n) * gridDim.x + blockIdx.x] = t;
  } else {
    for (int y = glue_row(lg_skip); y < H; y += (gridDim.x * RR) << (6 - lg_skip)) {
      float* dst = gskip + (((size_t)n * C2 + (c - C1)) * H + y) * W;
      if (vec_skip) {
        for (int x0 = 4 * glue_lane(lg_skip); x0 < W; x0 += 4 << lg_skip) {
          float a[4];
          pad1_adjoint_run<4>(g, y, x0, H, W, a);
          *reinterpret_cast<float4*>(dst + x0) = make_float4(a[0], a[1], a[2], a[3]);
        }
      } else {
        for (int xx = glue_lane(lg_skip); xx < W; xx += 1 << lg_skip) dst[xx] = pad1_adjoint(g, y, xx, H, W);
      }
    }
  }
}

// y <- ELU(y + bias) in place and yp = ReflectionPad2d(1)(y): image row r is padded row r + 1, and also padded row 0
// (r = 1) and H + 1 (r = H - 2).
__global__ __launch_bounds__(RW * RR) void bias_elu_pad_fwd_kernel(float* __restrict__ y, const float* __restrict__ bias,
                                                                   float* __restrict__ yp, int C, int H, int W, int vec, int lg) {
  const int PH = H + 2, PW = W + 2;
  const int r = glue_row(lg);
  if (r >= H) return;
  const size_t pl = blockIdx.y;
  const float b = bias[(int)(pl % C)];
  float* row = y + (pl * H + r) * W;
  float* dst = yp + pl * PH * PW;
  float* mid = dst + (size_t)(r + 1) * PW;
  float* top = r == 1 ? dst : nullptr;
  float* bot = r == H - 2 ? dst + (size_t)(H + 1) * PW : nullptr;
  if (vec) {
    for (int x0 = 4 * glue_lane(lg); x0 < W; x0 += 4 << lg) {
      float4 v = *reinterpret_cast<float4*>(row + x0);
      v.x = elu1(v.x + b); v.y = elu1(v.y + b); v.z = elu1(v.z + b); v.w = elu1(v.w + b);
      *reinterpret_cast<float4*>(row + x0) = v;
      pad_row_store4(mid, x0, W, v);
      if (top) pad_row_store4(top, x0, W, v);
      if (bot) pad_row_store4(bot, x0, W, v);
    }
  } else {
    for (int x = glue_lane(lg); x < W; x += 1 << lg) {
      const float v = elu1(row[x] + b);
      row[x] = v;
      pad_row_store1(mid, x, W, v);
      if (top) pad_row_store1(top, x, W, v);
      if (bot) pad_row_store1(bot, x, W, v);
    }
  }
}

// grad_z = (pad1_adjoint(grad_yp) + grad_y) * ELU'(y); either gradient may be NULL.  part as in upcat_pad_act_bwd_kernel.
__global__ __launch_bounds__(RW * RR) void bias_elu_pad_bwd_kernel(const float* __restrict__ gyp, const float* __restrict__ gy,
                                                                   const float* __restrict__ y, float* __restrict__ gz,
                                                                   double* __restrict__ part, int N, int C, int H, int W,
                                                                   int vec, int lg) {
  __shared__ double sh[RR];
  const int PH = H + 2, PW = W + 2;
  const int r = glue_row(lg);
  const int pl = blockIdx.y, n = pl / C, c = pl - n * C;
  const float* g = gyp ? gyp + (size_t)pl * PH * PW : nullptr;
  double acc = 0.0;
  if (r < H) {
    const size_t base = ((size_t)pl * H + r) * W;
    if (vec) {
      for (int x0 = 4 * glue_lane(lg); x0 < W; x0 += 4 << lg) {
        float a[4];
        if (g) {
          pad1_adjoint_run<4>(g, r, x0, H, W, a);
          if (gy) {
            const float4 u = *reinterpret_cast<const float4*>(gy + base + x0);
            a[0] += u.x; a[1] += u.y; a[2] += u.z; a[3] += u.w;
          }
        } else {
          const float4 u = *reinterpret_cast<const float4*>(gy + base + x0);
          a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w;
        }
        const float4 o = *reinterpret_cast<const float4*>(y + base + x0);
        float4 q;
        q.x = elu1_grad(a[0], o.x); q.y = elu1_grad(a[1], o.y); q.z = elu1_grad(a[2], o.z); q.w = elu1_grad(a[3], o.w);
        *reinterpret_cast<float4*>(gz + base + x0) = q;
        acc += (double)((q.x + q.y) + (q.z + q.w));
      }
    } else {
      for (int x = glue_lane(lg); x < W; x += 1 << lg) {
        float a;
        if (g) {
          a = pad1_adjoint(g, r, x, H, W);
          if (gy) a += gy[base + x];
        } else {
          a = gy[base + x];
        }
        const float q = elu1_grad(a, y[base + x]);
        gz[base + x] = q;
        acc += (double)q;
      }
    }
  }
  const double t = block_sum_rows(acc, sh);
  if (threadIdx.x == 0 && threadIdx.y == 0) part[((size_t)c * N + n) * gridDim.x + blockIdx.x] = t;
}

// grad_bias[c] = sum of the channel's `count` block partials: one wave per channel, lane l adds partials l, l + 64, ...
// in order, then the lanes are folded - a fixed order for a given shape.
__global__ __launch_bounds__(64) void bias_grad_final_wave_kernel(const double* __restrict__ part, float* __restrict__ gbias,
                                                                  int count) {
  const double* p = part + (size_t)blockIdx.x * count;
  double s = 0.0;
  for (int k = threadIdx.x; k < count; k += 64) s += p[k];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (threadIdx.x == 0) gbias[blockIdx.x] = (float)s;
}

// MaxPool2d(kernel 3, stride 2, padding 1): ATen's scan order and tie / NaN rule (first maximum in
// row-major window order; a NaN replaces the running maximum).  `code` = window position 0..8.
__global__ __launch_bounds__(RW * RR) void maxpool3s2_fwd_kernel(const float* __restrict__ in,
                                                                 float* __restrict__ out, uint8_t* __restrict__ code,
                                                                 int H, int W, int OH, int OW) {
  const int oy = blockIdx.x * RR + threadIdx.y;
  if (oy >= OH) return;
  const size_t pl = blockIdx.y;
  const float* p = in + pl * H * W;
  for (int ox = threadIdx.x; ox < OW; ox += RW) {
    float best = -INFINITY;
    int bc = -1;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int y = 2 * oy - 1 + dy;
      if (y < 0 || y >= H) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int x = 2 * ox - 1 + dx;
        if (x < 0 || x >= W) continue;
        const float v = p[(size_t)y * W + x];
        if (bc < 0 || v > best || v != v) { best = v; bc = dy * 3 + dx; }
      }
    }
    out[(pl * OH + oy) * OW + ox] = best;
    code[(pl * OH + oy) * OW + ox] = (uint8_t)bc;
  }
}

// Backward, one thread per output window (oy, ox): it owns the 2x2 input block whose top-left pixel is
// the window centre (2oy, 2ox) and gathers from the <= 4 windows that overlap the block, so every code /
// gradient value is read once per neighbour and the stores are two coalesced float2 rows.
__global__ __launch_bounds__(RW * RR) void maxpool3s2_bwd_kernel(const float* __restrict__ gout,
                                                                 const uint8_t* __restrict__ code,
                                                                 float* __restrict__ gin, int H, int W, int OH,
                                                                 int OW) {
  const int oy = blockIdx.x * RR + threadIdx.y;
  if (oy >= OH) return;
  const size_t pl = blockIdx.y;
  const float* g = gout + pl * OH * OW;
  const uint8_t* cd = code + pl * OH * OW;
  float* dst = gin + pl * H * W;
  const bool down = oy + 1 < OH;
  const int y0 = 2 * oy, y1 = 2 * oy + 1;
  for (int ox = threadIdx.x; ox < OW; ox += RW) {
    const bool right = ox + 1 < OW;
    const size_t i00 = (size_t)oy * OW + ox;
    const int c00 = cd[i00];
    const float g00 = g[i00];
    const int c01 = right ? cd[i00 + 1] : -1;
    const float g01 = right ? g[i00 + 1] : 0.0f;
    const int c10 = down ? cd[i00 + OW] : -1;
    const float g10 = down ? g[i00 + OW] : 0.0f;
    const int c11 = (down && right) ? cd[i00 + OW + 1] : -1;
    const float g11 = (down && right) ? g[i00 + OW + 1] : 0.0f;
    // window (oy,ox) covers rows 2oy-1..2oy+1: the block's pixels sit at window positions 4,5 / 7,8
    const float a = c00 == 4 ? g00 : 0.0f;                                            // (y0, x0)
    const float b = (c00 == 5 ? g00 : 0.0f) + (c01 == 3 ? g01 : 0.0f);                // (y0, x0+1)
    const float c = (c00 == 7 ? g00 : 0.0f) + (c10 == 1 ? g10 : 0.0f);                // (y0+1, x0)
    const float d = ((c00 == 8 ? g00 : 0.0f) + (c01 == 6 ? g01 : 0.0f)) +
                    ((c10 == 2 ? g10 : 0.0f) + (c11 == 0 ? g11 : 0.0f));              // (y0+1, x0+1)
    const int x0 = 2 * ox;
    dst[(size_t)y0 * W + x0] = a;
    if (x0 + 1 < W) dst[(size_t)y0 * W + x0 + 1] = b;
    if (y1 < H) {
      dst[(size_t)y1 * W + x0] = c;
      if (x0 + 1 < W) dst[(size_t)y1 * W + x0 + 1] = d;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Disparity head of the depth decoder: Conv3x3(C -> 1) = ReflectionPad2d(1) + Conv2d(C, 1, 3) + bias
// (layers.py:118-133, networks/depth_decoder.py:38-39, C = 16/32/64/128 at 192x640 .. 24x80).  With one
// output channel the layer is a pure streaming reduction over C input planes; MIOpen runs it at
// ~2.4 TFLOP/s (0.54 ms for C=16 at full resolution, forward+backward).  Here: one pass over x each way,
// reflection handled by index (no padded copy), weights in LDS, deterministic weight-gradient partials.
// ---------------------------------------------------------------------------------------------
constexpr int DC_MAXC = 256;
constexpr int DC_CHUNKS = 256;    // most partial rows of the weight gradient (four per lane of the final reduction)
constexpr int DC_UC = 4;          // channels whose windows a thread of the weight gradient has in flight at once
constexpr int DC_WAVES = NT / 64;

// Forward and weight gradient share one layout.  W % 4 == 0 (every size the decoder has): a task is a 4-pixel strip of
// TWO adjacent rows, so a channel costs 4 rows x (float4 + 2 halo scalars) for 8 outputs - a row is fetched twice, not
// three times.  Other widths: a task is one pixel.  The four scales differ by 64 in pixels and by 8 in channels
// (192 x 640 x 16 .. 24 x 80 x 128), so the CHANNELS are divided as well wherever the pixels alone would leave the
// machine idle: between `parts` threads of a workgroup in the forward (partial sums meet in LDS, added in part order),
// between gridDim.z workgroups in the data gradient (each writes its own planes), between gridDim.y in the weight gradient.
struct StripTask {
  int py0, px0;            // first row, first column
  int rr[4];               // offsets of rows py0 - 1 .. py0 + 2 inside a plane, reflected
  int cl, cr;              // columns left and right of the strip, reflected
  bool has1;               // the second row py0 + 1 exists
};

__device__ __forceinline__ StripTask strip_task(int t, int H, int W) {
  const int SW = W >> 2;
  StripTask k;
  const int rp = t / SW;
  k.py0 = 2 * rp;
  k.px0 = (t - rp * SW) << 2;
  k.has1 = k.py0 + 1 < H;
  k.rr[0] = reflect1(k.py0, H) * W;
  k.rr[1] = k.py0 * W;
  k.rr[2] = reflect1(k.py0 + 2, H) * W;
  k.rr[3] = k.has1 ? reflect1(k.py0 + 3, H) * W : k.rr[2];
  k.cl = reflect1(k.px0, W);
  k.cr = reflect1(k.px0 + 5, W);
  return k;
}
__device__ __forceinline__ int strip_tasks(int H, int W) { return ((H + 1) >> 1) * (W >> 2); }

// 4 rows x 6 columns (px0 - 1 .. px0 + 4) of U consecutive planes
template <int U>
__device__ __forceinline__ void load_strip_windows(const float* __restrict__ plane, int hw, const StripTask& k,
                                                   float win[U][4][6]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = plane + (size_t)u * hw + k.rr[r];
      const float4 m = *reinterpret_cast<const float4*>(row + k.px0);
      win[u][r][0] = row[k.cl];
      win[u][r][1] = m.x; win[u][r][2] = m.y; win[u][r][3] = m.z; win[u][r][4] = m.w;
      win[u][r][5] = row[k.cr];
    }
}

// the gradient that reaches the convolution's output through y = sigmoid(v): ATen's sigmoid_backward, grad * (1 - y) * y
__device__ __forceinline__ float through_sigmoid(float g, float y) { return (g * (1.0f - y)) * y; }

// y = conv(x) + bias, or its sigmoid.  Grid (groups of NT / parts tasks, N); thread (task s, part p) walks channels
// p, p + parts, ...  The sums are kept in double (one DFMA per tap, the rate of an fp32 multiply and add kept apart),
// and so is the sigmoid: where it is saturated, y ~ exp(v), every absolute error of v is a RELATIVE error of y and of the
// gradient through it, and an fp32 sum of taps of size 100 is off by 1e-5.
__global__ __launch_bounds__(NT) void dispconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y,
                                                          int C, int H, int W, int parts, int sigmoid) {
  __shared__ double sw[DC_MAXC * 9];
  __shared__ double red[8][NT];
  for (int i = threadIdx.x; i < C * 9; i += NT) sw[i] = (double)w[i];
  __syncthreads();
  const int hw = H * W, per = NT / parts;
  const int part = threadIdx.x / per, s = threadIdx.x - part * per;
  const size_t n = blockIdx.y;
  const float* xn = x + n * C * hw;
  const bool vec = (W & 3) == 0;
  const int tasks = vec ? strip_tasks(H, W) : hw;
  const int t = blockIdx.x * per + s;
  const bool live = t < tasks;
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0;
  StripTask k = {};
  if (vec) {
    k = strip_task(live ? t : tasks - 1, H, W);
#pragma unroll 2
    for (int c = part; c < C; c += parts) {
      float win[1][4][6];
      load_strip_windows<1>(xn + (size_t)c * hw, hw, k, win);
      const double* q = sw + c * 9;
      double d[4][6];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 6; ++i) d[r][i] = (double)win[0][r][i];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) acc[r * 4 + j] = fma(q[dy * 3 + dx], d[r + dy][j + dx], acc[r * 4 + j]);
    }
  } else {
    const int p = live ? t : tasks - 1;
    const int py = p / W, px = p - py * W;
    const int rows[3] = {reflect1(py, H) * W, py * W, reflect1(py + 2, H) * W};
    const int cols[3] = {reflect1(px, W), px, reflect1(px + 2, W)};
    for (int c = part; c < C; c += parts) {
      const float* xc = xn + (size_t)c * hw;
      const double* q = sw + c * 9;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) acc[0] = fma(q[dy * 3 + dx], (double)xc[rows[dy] + cols[dx]], acc[0]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[i][threadIdx.x] = acc[i];
  __syncthreads();
  if (!live) return;
  // the parts of a task share out its outputs: each adds the partial sums of one in part order and finishes it
  const double b = bias ? (double)bias[0] : 0.0;
  float* yn = y + n * hw;
  const int outs = vec ? (k.has1 ? 8 : 4) : 1;
  for (int i = part; i < outs; i += parts) {
    double v = 0.0;
    for (int p = 0; p < parts; ++p) v += red[i][p * per + s];
    v += b;
    if (sigmoid) v = 1.0 / (1.0 + exp(-v));
    yn[vec ? k.rr[1] + (i >> 2) * W + k.px0 + (i & 3) : t] = (float)v;
  }
}

// grad wrt x:  gx[n,c,q] = sum_d w[c][d] * G_d(q),  G_d(q) = sum over the padded positions (u,v) that
// read q of g[n, u - dy, v - dx] (zero outside the image) - G_d is shared by all channels.  g = gy, or gy taken
// through the sigmoid (y given).  Every q is read by (qy + 1, qx + 1): that term is the 3 x 3 window of the
// zero-extended g around q.  Row 1 is also read by padded row 0, which only window row dy = 0 of output row 0 touches,
// and row 0 is the window's own top row; likewise row H - 2 / padded row H + 1 / output row H - 1, and the columns.
// So the border terms are sums of window entries already in registers.  Grid (NT-strip groups, N, channel parts): a
// thread builds G of its 4-pixel strip once (one-channel reads) and writes channels z, z + gridDim.z, ... as float4.
__global__ __launch_bounds__(NT) void dispconv_bwd_data_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                               const float* __restrict__ w, float* __restrict__ gx,
                                                               int C, int H, int W) {
  const int hw = H * W;
  const size_t n = blockIdx.y;
  const float* g = gy + n * hw;
  const float* yn = y ? y + n * hw : nullptr;
  auto at = [&](int i) { return yn ? through_sigmoid(g[i], yn[i]) : g[i]; };
  const int t = blockIdx.x * NT + threadIdx.x;
  if ((W & 3) == 0) {
    if (t >= (hw >> 2)) return;
    const int q = t << 2;
    const int qy = q / W, qx0 = q - qy * W;
    float win[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int row = qy - 1 + r;
#pragma unroll
      for (int i = 0; i < 6; ++i) win[r][i] = 0.0f;
      if (row < 0 || row >= H) continue;
      const int o = row * W + qx0;
      float4 m = *reinterpret_cast<const float4*>(g + o);
      if (yn) {
        const float4 s = *reinterpret_cast<const float4*>(yn + o);
        m.x = through_sigmoid(m.x, s.x); m.y = through_sigmoid(m.y, s.y);
        m.z = through_sigmoid(m.z, s.z); m.w = through_sigmoid(m.w, s.w);
      }
      win[r][1] = m.x; win[r][2] = m.y; win[r][3] = m.z; win[r][4] = m.w;
      if (qx0 > 0) win[r][0] = at(o - 1);
      if (qx0 + 4 < W) win[r][5] = at(o + 4);
    }
    float G[4][9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) G[j][dy * 3 + dx] = win[2 - dy][j + 2 - dx];
    const bool top = qy == 1, bottom = qy == H - 2;           // both at H == 3
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        if (top) G[j][dx] += win[0][j + 2 - dx];
        if (bottom) G[j][6 + dx] += win[2][j + 2 - dx];
      }
    if (qx0 == 0) {                                           // qx = 1 is also read by padded column 0
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) G[1][dy * 3] += win[2 - dy][1];
      if (top) G[1][0] += win[0][1];
      if (bottom) G[1][6] += win[2][1];
    }
    if (qx0 + 4 == W) {                                       // qx = W - 2 by padded column W + 1
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) G[2][dy * 3 + 2] += win[2 - dy][4];
      if (top) G[2][2] += win[0][4];
      if (bottom) G[2][8] += win[2][4];
    }
    for (int c = blockIdx.z; c < C; c += gridDim.z) {
      const float* k = w + c * 9;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = ((k[0] * G[j][0] + k[1] * G[j][1] + k[2] * G[j][2]) + (k[3] * G[j][3] + k[4] * G[j][4] + k[5] * G[j][5])) +
               (k[6] * G[j][6] + k[7] * G[j][7] + k[8] * G[j][8]);
      *reinterpret_cast<float4*>(gx + (n * C + c) * hw + q) = make_float4(v[0], v[1], v[2], v[3]);
    }
    return;
  }
  if (t >= hw) return;
  const int qy = t / W, qx = t - qy * W;
  int us[3], vs[3], nu = 0, nv = 0;            // padded coordinates (0..H+1, 0..W+1) mapping onto (qy, qx)
  us[nu++] = qy + 1;
  if (qy == 1) us[nu++] = 0;
  if (qy == H - 2) us[nu++] = H + 1;
  vs[nv++] = qx + 1;
  if (qx == 1) vs[nv++] = 0;
  if (qx == W - 2) vs[nv++] = W + 1;
  float G[9];
#pragma unroll
  for (int d = 0; d < 9; ++d) G[d] = 0.0f;
  for (int a = 0; a < nu; ++a)
    for (int b = 0; b < nv; ++b) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int py = us[a] - dy;             // output row whose window row dy sits on padded row us[a]
        if (py < 0 || py >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int px = vs[b] - dx;
          if (px < 0 || px >= W) continue;
          G[dy * 3 + dx] += at(py * W + px);
        }
      }
    }
  for (int c = blockIdx.z; c < C; c += gridDim.z) {
    const float* k = w + c * 9;
    gx[(n * C + c) * hw + t] = ((k[0] * G[0] + k[1] * G[1] + k[2] * G[2]) + (k[3] * G[3] + k[4] * G[4] + k[5] * G[5])) +
                               (k[6] * G[6] + k[7] * G[7] + k[8] * G[8]);
  }
}

// grad wrt w (and bias): block (chunk, group of DC_UC channels) accumulates its share of the N * tasks tasks in fp32
// per thread, fp64 from there on; g is read once for the group's channels and their DC_UC windows (48 loads) are in
// flight together.  gridDim.x = as many chunks as there are workgroups' worth of tasks, DC_CHUNKS at the most.  A last,
// ragged group loads channel C - 1 in its spare slots and drops what they add up.  Every group forms the bias column;
// the final kernel reads channel 0's.
__global__ __launch_bounds__(NT) void dispconv_bwd_weight_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ gy,
                                                                 const float* __restrict__ y,
                                                                 double* __restrict__ part, int N, int C, int H,
                                                                 int W) {
  constexpr int TOTALS = DC_UC * 9 + 1;
  __shared__ double sh[DC_WAVES][TOTALS];
  const int hw = H * W, c0 = blockIdx.y * DC_UC;
  float acc[TOTALS];
#pragma unroll
  for (int i = 0; i < TOTALS; ++i) acc[i] = 0.0f;
  if ((W & 3) == 0) {
    const int tasks = strip_tasks(H, W);
    const long long total = (long long)N * tasks;
    for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < total; t += (long long)gridDim.x * NT) {
      const int n = (int)(t / tasks);
      const StripTask k = strip_task((int)(t - (long long)n * tasks), H, W);
      float g[2][4];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r == 1 && !k.has1) {
          g[1][0] = g[1][1] = g[1][2] = g[1][3] = 0.0f;
          continue;
        }
        const size_t o = (size_t)n * hw + k.rr[1] + r * W + k.px0;
        float4 m = *reinterpret_cast<const float4*>(gy + o);
        if (y) {
          const float4 s = *reinterpret_cast<const float4*>(y + o);
          m.x = through_sigmoid(m.x, s.x); m.y = through_sigmoid(m.y, s.y);
          m.z = through_sigmoid(m.z, s.z); m.w = through_sigmoid(m.w, s.w);
        }
        g[r][0] = m.x; g[r][1] = m.y; g[r][2] = m.z; g[r][3] = m.w;
      }
      float win[DC_UC][4][6];
#pragma unroll
      for (int u = 0; u < DC_UC; ++u) {
        float one[1][4][6];
        load_strip_windows<1>(x + ((size_t)n * C + min(c0 + u, C - 1)) * hw, hw, k, one);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int i = 0; i < 6; ++i) win[u][r][i] = one[0][r][i];
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r == 1 && !k.has1) continue;                      // no 0 * inf from the row below the image
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int u = 0; u < DC_UC; ++u)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx)
                acc[u * 9 + dy * 3 + dx] = fmaf(g[r][j], win[u][r + dy][j + dx], acc[u * 9 + dy * 3 + dx]);
          acc[TOTALS - 1] += g[r][j];
        }
      }
    }
  } else {
    const long long total = (long long)N * hw;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
      const int n = (int)(i / hw), p = (int)(i - (long long)n * hw);
      const int py = p / W, px = p - py * W;
      const float gi = y ? through_sigmoid(gy[i], y[i]) : gy[i];
      const int rows[3] = {reflect1(py, H) * W, py * W, reflect1(py + 2, H) * W};
      const int cols[3] = {reflect1(px, W), px, reflect1(px + 2, W)};
#pragma unroll
      for (int u = 0; u < DC_UC; ++u) {
        const float* xc = x + ((size_t)n * C + min(c0 + u, C - 1)) * hw;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc[u * 9 + dy * 3 + dx] += gi * xc[rows[dy] + cols[dx]];
      }
      acc[TOTALS - 1] += gi;
    }
  }
  // wave sums of all totals side by side - no barrier between them - then ONE exchange through LDS, waves in index order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < TOTALS; ++i) {
    double v = (double)acc[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave][i] = v;
  }
  __syncthreads();
  static_assert(DC_WAVES == 4, "the sum below names the four waves");
  if (threadIdx.x >= TOTALS) return;
  const int i = threadIdx.x;
  const double total = (sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]);
  double* row = part + (size_t)blockIdx.x * C * 10;
  if (i < TOTALS - 1) {
    const int u = i / 9;
    if (c0 + u < C) row[(c0 + u) * 10 + (i - u * 9)] = total;
  } else {
    for (int u = 0; u < DC_UC && c0 + u < C; ++u) row[(c0 + u) * 10 + 9] = total;
  }
}

// one wave per output: lane l adds chunks l, l + 64, ... in that order, then a fixed-order butterfly
__global__ __launch_bounds__(64) void dispconv_bwd_weight_final_kernel(const double* __restrict__ part,
                                                                      float* __restrict__ gw, float* __restrict__ gb,
                                                                      int C, int chunks) {
  const int i = blockIdx.x;                    // 0 .. C*9 (the last one is the bias)
  const int c = i < C * 9 ? i / 9 : 0, d = i < C * 9 ? i - c * 9 : 9;
  double v = 0.0;
  for (int k = threadIdx.x; k < chunks; k += 64) v += part[((size_t)k * C + c) * 10 + d];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if (threadIdx.x == 0) {
    if (i < C * 9) gw[i] = (float)v;
    else if (gb) gb[0] = (float)v;
  }
}

int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int bbd_bn_scratch_doubles(int N, int C, int HW) { return C * pick_split(N, HW) * 2; }
int bbd_bn_grouped_scratch_doubles(int max_group_rows, int G, int C, int HW) {
  return G * C * pick_split(max_group_rows, HW) * 2;
}

namespace {
int launch_bn_fwd(BnArgs& a, int biggest, bool running, hipStream_t st) {
  a.split = pick_split(biggest, a.HW);
  if ((long long)biggest * a.HW <= BN_SMALL_ELEMS) {       // one launch (+ a C-thread one for the cross-group results)
    hipLaunchKernelGGL(bn_fwd_small_kernel, dim3(1, (unsigned)a.C, (unsigned)a.G), dim3(NT), 0, st, a);
    if (a.G > 1 && running)
      hipLaunchKernelGGL(bn_running_small_kernel, dim3((unsigned)((a.C + 63) / 64)), dim3(64), 0, st, a);
    return status();
  }
  const dim3 grid((unsigned)a.split, (unsigned)a.C, (unsigned)a.G);
  hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(NT), 0, st, a);
  hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(NT), 0, st, a);
  return status();
}
int launch_bn_bwd(BnArgs& a, int biggest, hipStream_t st) {
  a.split = pick_split(biggest, a.HW);
  if ((long long)biggest * a.HW <= BN_SMALL_ELEMS) {
    hipLaunchKernelGGL(bn_bwd_small_kernel, dim3(1, (unsigned)a.C, (unsigned)a.G), dim3(NT), 0, st, a);
    if (a.G > 1) hipLaunchKernelGGL(bn_param_grad_small_kernel, dim3((unsigned)((a.C + 63) / 64)), dim3(64), 0, st, a);
    return status();
  }
  const dim3 grid((unsigned)a.split, (unsigned)a.C, (unsigned)a.G);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, grid, dim3(NT), 0, st, a);
  hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(NT), 0, st, a);
  return status();
}
void fill_fwd(BnArgs& a, const float* x, const float* residual, const float* gamma, const float* beta, float* y,
              float* save_mean, float* save_invstd, float* running_mean, float* running_var, long long* num_batches_tracked,
              double* scratch, int N, int C, int HW, double eps, double momentum, int relu) {
  a.x = x; a.res = residual; a.gamma = gamma; a.beta = beta; a.y = y; a.part = scratch; a.mean = save_mean;
  a.invstd = save_invstd; a.run_mean = running_mean; a.run_var = running_var; a.batches = num_batches_tracked; a.N = N; a.C = C; a.HW = HW;
  a.relu = relu; a.eps = (float)eps; a.momentum = (float)momentum;
}
void fill_bwd(BnArgs& a, const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
              const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual, float* grad_gamma,
              float* grad_beta, double* scratch, int N, int C, int HW, int relu) {
  a.x = x; a.y = const_cast<float*>(y); a.dy = grad_y; a.gamma = gamma; a.beta = beta; a.mean = const_cast<float*>(save_mean);
  a.invstd = const_cast<float*>(save_invstd); a.dx = grad_x; a.dres = grad_residual; a.dgamma = grad_gamma;
  a.dbeta = grad_beta; a.part = scratch; a.N = N; a.C = C; a.HW = HW; a.relu = relu;
}

// The one body per direction behind every bbd_bn_act_* entry point: they differ in the description of the call groups only
int bn_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y, float* save_mean,
           float* save_invstd, float* running_mean, float* running_var, long long* num_batches_tracked, double* scratch,
           const BbdBnGroups& groups, int N, int C, int HW, double eps, double momentum, int relu, void* stream) {
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !scratch || N <= 0 || C <= 0 || HW <= 0)
    return BBD_E_BADARG;
  if ((running_mean == nullptr) != (running_var == nullptr)) return BBD_E_BADARG;
  BnArgs a = {};
  const int biggest = bbd_bn_resolve_groups(groups, N, &a);
  if (!biggest) return BBD_E_BADARG;
  fill_fwd(a, x, residual, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch,
           N, C, HW, eps, momentum, relu);
  return launch_bn_fwd(a, biggest, running_mean || num_batches_tracked, static_cast<hipStream_t>(stream));
}

int bn_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
           const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual, float* grad_gamma,
           float* grad_beta, double* scratch, const BbdBnGroups& groups, int N, int C, int HW, int relu, void* stream) {
  if (!x || !grad_y || !gamma || !save_mean || !save_invstd || !grad_x || !grad_gamma || !grad_beta || !scratch ||
      N <= 0 || C <= 0 || HW <= 0 || (relu && !y && !beta))
    return BBD_E_BADARG;
  BnArgs a = {};
  const int biggest = bbd_bn_resolve_groups(groups, N, &a);
  if (!biggest) return BBD_E_BADARG;
  fill_bwd(a, x, y, grad_y, gamma, beta, save_mean, save_invstd, grad_x, grad_residual, grad_gamma, grad_beta, scratch, N, C,
           HW, relu);
  return launch_bn_bwd(a, biggest, static_cast<hipStream_t>(stream));
}
}  // namespace

int bbd_bn_act_grouped_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                           float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                           long long* num_batches_tracked, double* scratch, const int32_t* group_rows, int G,
                           int untracked_groups, int N, int C, int HW, double eps, double momentum, int relu, void* stream) {
  return bn_fwd(x, residual, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch,
                {group_rows, nullptr, G, untracked_groups, 0}, N, C, HW, eps, momentum, relu, stream);
}

int bbd_bn_act_grouped_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual,
                           float* grad_gamma, float* grad_beta, double* scratch, const int32_t* group_rows, int G, int N,
                           int C, int HW, int relu, void* stream) {
  return bn_bwd(x, y, grad_y, gamma, beta, save_mean, save_invstd, grad_x, grad_residual, grad_gamma, grad_beta, scratch,
                {group_rows, nullptr, G, 0, 0}, N, C, HW, relu, stream);
}

// Device-resident group table (ABI 7): the same launches with NOTHING of the batch signature in their arguments.
int bbd_bn_act_grouped_dev_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                               float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                               long long* num_batches_tracked, double* scratch, const int32_t* group_table, int G,
                               int max_group_rows, int N, int C, int HW, double eps, double momentum, int relu,
                               void* stream) {
  return bn_fwd(x, residual, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch,
                {nullptr, group_table, G, 0, max_group_rows}, N, C, HW, eps, momentum, relu, stream);
}

int bbd_bn_act_grouped_dev_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual,
                               float* grad_gamma, float* grad_beta, double* scratch, const int32_t* group_table, int G,
                               int max_group_rows, int N, int C, int HW, int relu, void* stream) {
  return bn_bwd(x, y, grad_y, gamma, beta, save_mean, save_invstd, grad_x, grad_residual, grad_gamma, grad_beta, scratch,
                {nullptr, group_table, G, 0, max_group_rows}, N, C, HW, relu, stream);
}

// ---- encoder stem: conv1 -> bn1 + ReLU -> MaxPool2d(3, 2, 1).  Only the two-launch form exists (BBD_STEM_MIN_ELEMS)
namespace {
bool stem_shape_ok(int biggest, int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || C > 65535 || H < 1 || W < 4 || (W & 3) || biggest < 1 || biggest > N) return false;
  if ((long long)H * W > 0x7fffffffLL) return false;
  return (long long)biggest * H * W > BN_SMALL_ELEMS;
}
bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

int launch_stem_fwd(BnArgs& a, int biggest, int H, int W, hipStream_t st) {
  a.split = pick_split(biggest, a.HW);
  a.W = W;
  hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)a.split, (unsigned)a.C, (unsigned)a.G), dim3(NT), 0, st, a);
  const int OH = (H - 1) / 2 + 1;
  const long long tasks = (long long)biggest * ((OH + STEM_TP - 1) / STEM_TP) * (W >> 2);
  const long long groups = (tasks + NT - 1) / NT;
  if (groups > 0x7fffffffLL) return BBD_E_BADARG;
  hipLaunchKernelGGL(stem_apply_pool_kernel, dim3((unsigned)groups, (unsigned)a.C, (unsigned)a.G), dim3(NT), 0, st, a);
  return status();
}
int launch_stem_bwd(BnArgs& a, int biggest, int W, hipStream_t st) {
  a.split = pick_split(biggest, a.HW);
  a.W = W;
  const dim3 grid((unsigned)a.split, (unsigned)a.C, (unsigned)a.G);
  if (a.gpool) {
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, grid, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, dim3(NT), 0, st, a);
  } else {                                   // the pool's output was not used: the plain backward on grad_y
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, grid, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(NT), 0, st, a);
  }
  return status();
}
bool stem_fwd_ptrs_ok(const float* x, const float* gamma, const float* beta, const float* y, const float* pooled,
                      const uint8_t* code, const float* save_mean, const float* save_invstd, const float* running_mean,
                      const float* running_var, const double* scratch) {
  if (!x || !gamma || !beta || !pooled || !code || !save_mean || !save_invstd || !scratch) return false;
  if ((running_mean == nullptr) != (running_var == nullptr)) return false;
  return aligned(x, 16) && aligned(y, 16) && aligned(pooled, 8) && aligned(code, 2);
}
bool stem_bwd_ptrs_ok(const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code, const float* gamma,
                      const float* beta, const float* save_mean, const float* save_invstd, const float* grad_x,
                      const float* grad_gamma, const float* grad_beta, const double* scratch) {
  if (!x || !gamma || !beta || !save_mean || !save_invstd || !grad_x || !grad_gamma || !grad_beta || !scratch) return false;
  if (!grad_y && !grad_pooled) return false;
  if (grad_pooled && !code) return false;
  return aligned(x, 16) && aligned(grad_y, 16) && aligned(grad_x, 16) && aligned(grad_pooled, 8) && aligned(code, 2);
}
void fill_stem_bwd(BnArgs& a, const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code,
                   const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, float* grad_x,
                   float* grad_gamma, float* grad_beta, double* scratch, int N, int C, int H, int W) {
  // y = NULL: the ReLU mask is re-derived from x, as in the backward of a forward without a residual
  fill_bwd(a, x, nullptr, grad_y, gamma, beta, save_mean, save_invstd, grad_x, nullptr, grad_gamma, grad_beta, scratch, N, C,
           H * W, 1);
  a.gpool = grad_pooled;
  a.code = const_cast<uint8_t*>(code);
}

int stem_fwd(const float* x, const float* gamma, const float* beta, float* y, float* pooled, uint8_t* code, float* save_mean,
             float* save_invstd, float* running_mean, float* running_var, long long* num_batches_tracked, double* scratch,
             const BbdBnGroups& groups, int N, int C, int H, int W, double eps, double momentum, void* stream) {
  if (!stem_fwd_ptrs_ok(x, gamma, beta, y, pooled, code, save_mean, save_invstd, running_mean, running_var, scratch))
    return BBD_E_BADARG;
  BnArgs a = {};
  const int biggest = bbd_bn_resolve_groups(groups, N, &a);
  if (!biggest || !stem_shape_ok(biggest, N, C, H, W)) return BBD_E_BADARG;
  fill_fwd(a, x, nullptr, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch, N, C,
           H * W, eps, momentum, 1);
  a.pooled = pooled; a.code = code;
  return launch_stem_fwd(a, biggest, H, W, static_cast<hipStream_t>(stream));
}

int stem_bwd(const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code, const float* gamma,
             const float* beta, const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma,
             float* grad_beta, double* scratch, const BbdBnGroups& groups, int N, int C, int H, int W, void* stream) {
  if (!stem_bwd_ptrs_ok(x, grad_y, grad_pooled, code, gamma, beta, save_mean, save_invstd, grad_x, grad_gamma, grad_beta,
                        scratch))
    return BBD_E_BADARG;
  BnArgs a = {};
  const int biggest = bbd_bn_resolve_groups(groups, N, &a);
  if (!biggest || !stem_shape_ok(biggest, N, C, H, W)) return BBD_E_BADARG;
  fill_stem_bwd(a, x, grad_y, grad_pooled, code, gamma, beta, save_mean, save_invstd, grad_x, grad_gamma, grad_beta, scratch,
                N, C, H, W);
  return launch_stem_bwd(a, biggest, W, static_cast<hipStream_t>(stream));
}
}  // namespace

int bbd_stem_fwd(const float* x, const float* gamma, const float* beta, float* y, float* pooled, uint8_t* code,
                 float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                 long long* num_batches_tracked, double* scratch, const int32_t* group_rows, int G, int untracked_groups,
                 int N, int C, int H, int W, double eps, double momentum, void* stream) {
  return stem_fwd(x, gamma, beta, y, pooled, code, save_mean, save_invstd, running_mean, running_var, num_batches_tracked,
                  scratch, {group_rows, nullptr, G, untracked_groups, 0}, N, C, H, W, eps, momentum, stream);
}

int bbd_stem_bwd(const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code, const float* gamma,
                 const float* beta, const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma,
                 float* grad_beta, double* scratch, const int32_t* group_rows, int G, int N, int C, int H, int W,
                 void* stream) {
  return stem_bwd(x, grad_y, grad_pooled, code, gamma, beta, save_mean, save_invstd, grad_x, grad_gamma, grad_beta, scratch,
                  {group_rows, nullptr, G, 0, 0}, N, C, H, W, stream);
}

int bbd_stem_dev_fwd(const float* x, const float* gamma, const float* beta, float* y, float* pooled, uint8_t* code,
                     float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                     long long* num_batches_tracked, double* scratch, const int32_t* group_table, int G,
                     int max_group_rows, int N, int C, int H, int W, double eps, double momentum, void* stream) {
  return stem_fwd(x, gamma, beta, y, pooled, code, save_mean, save_invstd, running_mean, running_var, num_batches_tracked,
                  scratch, {nullptr, group_table, G, 0, max_group_rows}, N, C, H, W, eps, momentum, stream);
}

int bbd_stem_dev_bwd(const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code, const float* gamma,
                     const float* beta, const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma,
                     float* grad_beta, double* scratch, const int32_t* group_table, int G, int max_group_rows, int N, int C,
                     int H, int W, void* stream) {
  return stem_bwd(x, grad_y, grad_pooled, code, gamma, beta, save_mean, save_invstd, grad_x, grad_gamma, grad_beta, scratch,
                  {nullptr, group_table, G, 0, max_group_rows}, N, C, H, W, stream);
}

int bbd_bn_act_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                   float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                   long long* num_batches_tracked, double* scratch, int N, int C, int HW, double eps, double momentum,
                   int relu, void* stream) {
  const int32_t rows[2] = {0, N};
  return bn_fwd(x, residual, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch,
                {rows, nullptr, 1, 0, 0}, N, C, HW, eps, momentum, relu, stream);
}

int bbd_bn_act_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
                   const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual, float* grad_gamma, float* grad_beta,
                   double* scratch, int N, int C, int HW, int relu, void* stream) {
  const int32_t rows[2] = {0, N};
  return bn_bwd(x, y, grad_y, gamma, beta, save_mean, save_invstd, grad_x, grad_residual, grad_gamma, grad_beta, scratch,
                {rows, nullptr, 1, 0, 0}, N, C, HW, relu, stream);
}

int bbd_reflect_pad1_fwd(const float* in, float* out, int planes, int H, int W, void* stream) {
  if (!in || !out || planes <= 0 || planes > 65535 || H < 2 || W < 2) return BBD_E_BADARG;
  hipLaunchKernelGGL(reflect_pad1_fwd_kernel, dim3((unsigned)((H + 2 + RR - 1) / RR), (unsigned)planes), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), in, out, H, W);
  return status();
}

int bbd_reflect_pad1_bwd(const float* grad_out, float* grad_in, int planes, int H, int W, void* stream) {
  if (!grad_out || !grad_in || planes <= 0 || planes > 65535 || H < 2 || W < 2) return BBD_E_BADARG;
  hipLaunchKernelGGL(reflect_pad1_bwd_kernel, dim3((unsigned)((H + RR - 1) / RR), (unsigned)planes), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), grad_out, grad_in, H, W);
  return status();
}

int bbd_upcat_pad1_fwd(const float* x, const float* skip, float* out, int N, int C1, int C2, int h, int w, void* stream) {
  if (!x || !out || N <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !skip) || h < 1 || w < 1) return BBD_E_BADARG;
  if ((long)N * (C1 + C2) > 65535) return BBD_E_BADARG;
  hipLaunchKernelGGL(upcat_pad_fwd_kernel, dim3((unsigned)((2 * h + 2 + RR - 1) / RR), (unsigned)(N * (C1 + C2))), dim3(RW, RR),
                     0, static_cast<hipStream_t>(stream), x, skip, out, C1, C2, h, w);
  return status();
}

int bbd_upcat_pad1_bwd(const float* grad_out, float* grad_x, float* grad_skip, int N, int C1, int C2, int h, int w,
                       void* stream) {
  if (!grad_out || !grad_x || N <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !grad_skip) || h < 1 || w < 1) return BBD_E_BADARG;
  if ((long)N * (C1 + C2) > 65535) return BBD_E_BADARG;
  hipLaunchKernelGGL(upcat_pad_bwd_kernel, dim3((unsigned)((2 * h + RR - 1) / RR), (unsigned)(N * (C1 + C2))), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), grad_out, grad_x, grad_skip, C1, C2, h, w);
  return status();
}

int bbd_bias_elu_scratch_doubles(int N, int C, int HW) { return C * pick_split(N, HW); }

int bbd_bias_elu_fwd(float* y, const float* bias, int N, int C, int HW, void* stream) {
  if (!y || !bias || N <= 0 || C <= 0 || HW <= 0 || (HW & 3)) return BBD_E_BADARG;
  const size_t total = (size_t)N * C * HW;
  const size_t blocks = (total / 4 + NT - 1) / NT;
  hipLaunchKernelGGL(bias_elu_fwd_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), y, bias, C, HW, total);
  return status();
}

int bbd_bias_elu_bwd(const float* y, const float* grad_y, float* grad_x, float* grad_bias, double* scratch, int N, int C,
                     int HW, void* stream) {
  if (!y || !grad_y || !grad_x || !grad_bias || !scratch || N <= 0 || C <= 0 || HW <= 0 || (HW & 3)) return BBD_E_BADARG;
  const int split = pick_split(N, HW);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bias_elu_bwd_kernel, dim3((unsigned)split, (unsigned)C), dim3(NT), 0, st, y, grad_y, grad_x, scratch, N, C,
                     HW, split);
  hipLaunchKernelGGL(bias_grad_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, scratch, grad_bias, C, split);
  return status();
}

namespace {
// may this tensor be read or written in float4 steps?  (NULL: it is not touched)
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// glue_row / glue_lane: log2 of the lanes along a row whose lanes have `items` things to do in all, and the workgroups
// that then cover `rows` rows
int glue_lanes_log2(int items) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < items) ++lg;
  return lg;
}
int glue_blocks(int rows, int lg) {
  const int per = RR << (6 - lg);
  return (rows + per - 1) / per;
}
}  // namespace

int bbd_upcat_pad_act_fwd(const float* z, const float* bias, const float* skip, float* out, int N, int C1, int C2, int h, int w,
                          void* stream) {
  if (!z || !bias || !out || N <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !skip) || h < 1 || w < 1) return BBD_E_BADARG;
  if ((long)N * (C1 + C2) > 65535 || (2L * h + 2) * (2L * w + 2) > 2147483647L) return BBD_E_BADARG;
  const int vec_z = (w % 4 == 0) && aligned16(z), vec_skip = (w % 2 == 0) && aligned16(skip);
  const int lg_z = glue_lanes_log2(vec_z ? w / 4 : w), lg_skip = glue_lanes_log2(vec_skip ? w / 2 : 2 * w);
  hipLaunchKernelGGL(upcat_pad_act_fwd_kernel, dim3((unsigned)glue_blocks(h, lg_z), (unsigned)(N * (C1 + C2))), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), z, bias, skip, out, C1, C2, h, w, vec_z, vec_skip, lg_z, lg_skip);
  return status();
}

int bbd_upcat_pad_act_bwd(const float* grad_out, const float* z, const float* bias, float* grad_z, float* grad_skip,
                          float* grad_bias, double* scratch, int scratch_doubles, int N, int C1, int C2, int h, int w,
                          void* stream) {
  if (!grad_out || !z || !bias || !grad_z || !grad_bias || !scratch || N <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && !grad_skip) ||
      h < 1 || w < 1)
    return BBD_E_BADARG;
  if ((long)N * (C1 + C2) > 65535 || (2L * h + 2) * (2L * w + 2) > 2147483647L) return BBD_E_BADARG;
  if ((long)C1 * N * ((h + RR - 1) / RR) > scratch_doubles) return BBD_E_BADARG;
  const int vec_z = (w % 4 == 0) && aligned16(z) && aligned16(grad_z), vec_skip = (w % 2 == 0) && aligned16(grad_skip);
  const int lg_z = glue_lanes_log2(vec_z ? w / 4 : w), lg_skip = glue_lanes_log2(vec_skip ? w / 2 : 2 * w);
  const int gx = glue_blocks(h, lg_z);          // <= ceil(h / BBD_GLUE_ROWS), the partials the caller made room for
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(upcat_pad_act_bwd_kernel, dim3((unsigned)gx, (unsigned)(N * (C1 + C2))), dim3(RW, RR), 0, st, grad_out, z,
                     bias, grad_z, grad_skip, scratch, N, C1, C2, h, w, vec_z, vec_skip, lg_z, lg_skip);
  hipLaunchKernelGGL(bias_grad_final_wave_kernel, dim3((unsigned)C1), dim3(64), 0, st, scratch, grad_bias, N * gx);
  return status();
}

int bbd_bias_elu_pad_fwd(float* y, const float* bias, float* yp, int N, int C, int H, int W, void* stream) {
  if (!y || !bias || !yp || N <= 0 || C <= 0 || (long)N * C > 65535 || H < 2 || W < 2) return BBD_E_BADARG;
  const int vec = (W % 4 == 0) && aligned16(y), lg = glue_lanes_log2(vec ? W / 4 : W);
  hipLaunchKernelGGL(bias_elu_pad_fwd_kernel, dim3((unsigned)glue_blocks(H, lg), (unsigned)(N * C)), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), y, bias, yp, C, H, W, vec, lg);
  return status();
}

int bbd_bias_elu_pad_bwd(const float* grad_yp, const float* grad_y, const float* y, float* grad_z, float* grad_bias,
                         double* scratch, int scratch_doubles, int N, int C, int H, int W, void* stream) {
  if ((!grad_yp && !grad_y) || !y || !grad_z || !grad_bias || !scratch || N <= 0 || C <= 0 || (long)N * C > 65535 || H < 2 ||
      W < 2)
    return BBD_E_BADARG;
  if ((long)C * N * ((H + RR - 1) / RR) > scratch_doubles) return BBD_E_BADARG;
  const int vec = (W % 4 == 0) && aligned16(y) && aligned16(grad_z) && aligned16(grad_y);
  const int lg = glue_lanes_log2(vec ? W / 4 : W), gx = glue_blocks(H, lg);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bias_elu_pad_bwd_kernel, dim3((unsigned)gx, (unsigned)(N * C)), dim3(RW, RR), 0, st, grad_yp, grad_y, y,
                     grad_z, scratch, N, C, H, W, vec, lg);
  hipLaunchKernelGGL(bias_grad_final_wave_kernel, dim3((unsigned)C), dim3(64), 0, st, scratch, grad_bias, N * gx);
  return status();
}

int bbd_maxpool3s2_fwd(const float* in, float* out, uint8_t* code, int planes, int H, int W, void* stream) {
  if (!in || !out || !code || planes <= 0 || planes > 65535 || H < 1 || W < 1) return BBD_E_BADARG;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;          // floor((H + 2 - 3) / 2) + 1
  hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3((unsigned)((OH + RR - 1) / RR), (unsigned)planes), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), in, out, code, H, W, OH, OW);
  return status();
}

int bbd_maxpool3s2_bwd(const float* grad_out, const uint8_t* code, float* grad_in, int planes, int H, int W,
                       void* stream) {
  if (!grad_out || !code || !grad_in || planes <= 0 || planes > 65535 || H < 1 || W < 1) return BBD_E_BADARG;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3((unsigned)((OH + RR - 1) / RR), (unsigned)planes), dim3(RW, RR), 0,
                     static_cast<hipStream_t>(stream), grad_out, code, grad_in, H, W, OH, OW);
  return status();
}

int bbd_dispconv_scratch_doubles(int C) { return DC_CHUNKS * C * 10; }

namespace {
constexpr long DC_FILL = 65536;      // threads' worth of tasks from which on the pixels alone fill the machine
constexpr long DC_RESIDENT = 1024;  // workgroups of the weight gradient that the machine holds at once

int launch_dispconv_fwd(const float* x, const float* weight, const float* bias, float* y, int N, int C, int H, int W,
                        int sigmoid, void* stream) {
  if (!x || !weight || !y || N <= 0 || N > 65535 || C <= 0 || C > DC_MAXC || H < 2 || W < 2) return BBD_E_BADARG;
  const int tasks = (W & 3) == 0 ? ((H + 1) / 2) * (W / 4) : H * W;
  const int parts = (long)N * tasks * 4 >= DC_FILL ? 4 : 16;
  const int per = NT / parts;
  hipLaunchKernelGGL(dispconv_fwd_kernel, dim3((unsigned)((tasks + per - 1) / per), (unsigned)N), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), x, weight, bias, y, C, H, W, parts, sigmoid);
  return status();
}
int launch_dispconv_bwd(const float* x, const float* weight, const float* y, const float* grad_y, float* grad_x,
                        float* grad_weight, float* grad_bias, double* scratch, int N, int C, int H, int W, void* stream) {
  if (!x || !weight || !grad_y || !scratch || N <= 0 || N > 65535 || C <= 0 || C > DC_MAXC || H < 2 || W < 2)
    return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (W & 3) == 0;
  if (grad_x) {
    const int work = vec ? H * W / 4 : H * W;
    long z = (DC_FILL + (long)N * work - 1) / ((long)N * work);
    z = z < 1 ? 1 : z > C ? C : z;
    hipLaunchKernelGGL(dispconv_bwd_data_kernel, dim3((unsigned)((work + NT - 1) / NT), (unsigned)N, (unsigned)z), dim3(NT), 0,
                       st, grad_y, y, weight, grad_x, C, H, W);
  }
  if (grad_weight) {
    // one workgroup's worth of tasks per chunk, but no more workgroups than are resident at once (4 per CU at this
    // kernel's 127 registers, 256 CUs): beyond that a workgroup only waits for a slot and adds an epilogue
    const long total = (long)N * (vec ? ((H + 1) / 2) * (W / 4) : H * W);
    const int groups = (C + DC_UC - 1) / DC_UC;
    long chunks = (total + NT - 1) / NT;
    const long resident = DC_RESIDENT / groups > 1 ? DC_RESIDENT / groups : 1;
    chunks = chunks > resident ? resident : chunks;
    chunks = chunks > DC_CHUNKS ? DC_CHUNKS : chunks;
    hipLaunchKernelGGL(dispconv_bwd_weight_kernel, dim3((unsigned)chunks, (unsigned)groups), dim3(NT), 0,
                       st, x, grad_y, y, scratch, N, C, H, W);
    hipLaunchKernelGGL(dispconv_bwd_weight_final_kernel, dim3((unsigned)(C * 9 + 1)), dim3(64), 0, st, scratch,
                       grad_weight, grad_bias, C, (int)chunks);
  }
  return status();
}
}  // namespace

int bbd_dispconv_fwd(const float* x, const float* weight, const float* bias, float* y, int N, int C, int H, int W,
                     void* stream) {
  return launch_dispconv_fwd(x, weight, bias, y, N, C, H, W, 0, stream);
}

int bbd_dispconv_bwd(const float* x, const float* weight, const float* grad_y, float* grad_x, float* grad_weight,
                     float* grad_bias, double* scratch, int N, int C, int H, int W, void* stream) {
  return launch_dispconv_bwd(x, weight, nullptr, grad_y, grad_x, grad_weight, grad_bias, scratch, N, C, H, W, stream);
}

int bbd_disp_head_fwd(const float* x, const float* weight, const float* bias, float* disp, int N, int C, int H, int W,
                      void* stream) {
  return launch_dispconv_fwd(x, weight, bias, disp, N, C, H, W, 1, stream);
}

int bbd_disp_head_bwd(const float* x, const float* weight, const float* disp, const float* grad_disp, float* grad_x,
                      float* grad_weight, float* grad_bias, double* scratch, int N, int C, int H, int W, void* stream) {
  if (!disp) return BBD_E_BADARG;
  return launch_dispconv_bwd(x, weight, disp, grad_disp, grad_x, grad_weight, grad_bias, scratch, N, C, H, W, stream);
}

}  // extern "C"
