// bbd_syns.hip - the SYNS-Patches half of evaluate_depth.py on the device (evaluate_depth.py:26-102, :244-297;
// trainer.py:576-594): predicted depth edges, exact Euclidean distance transforms, edge accuracy / completeness,
// `err`, and the point-cloud F-score / IoU of `--chamfer`, for a ragged batch of images per call.
//
// The reference does this per image on the host with cv2 (GaussianBlur, two Sobel), scipy (two
// distance_transform_edt) and a third-party CUDA extension (brute-force chamfer distance).  Here:
//
//   edges     log_kernel    L = to_log(prediction resampled at every ground-truth pixel)         (grid, image)
//             blur_kernel   B = 3x3 Gaussian of L, float32, placed products                      (grid, image)
//             sobel_kernel  mag = |5x5 Sobel of B| in float64                                    (grid, image)
//             thresh_kernel mean(mag) as an fp64 sum in a fixed order, edge = mag > mean, count  one workgroup / image
//   distance  edt_col_kernel  vertical distance to the nearest set pixel, one lane per column
//             edt_row_kernel  one workgroup per row holds the row's squared column distances in LDS; every pixel takes
//                             min over x' of (x - x')^2 + g^2[x'] - exact, integer, order-free
//   metrics   edge_reduce_kernel  one workgroup per image, fp64 sums in a fixed order
//   clouds    cloud_kernel  masked back-projection with a deterministic compaction (block scan), one workgroup / image
//             nn_kernel     all-pairs nearest neighbour: NQ queries per lane in registers, targets tiled through LDS
//                           (every lane reads the same target: a broadcast), minima combined across target splits
//                           with integer atomicMin on the float bits (distances are >= 0: the bits order as the values)
//             cloud_reduce_kernel  counts, precision / recall, F-score and IoU in float32
//
// Every sum is either integer or an fp64 sum whose order is fixed by the kernel (lane-strided accumulators, a wave
// tree, waves in order); every minimum is over integers or over float32 values whose minimum does not depend on order.
// Nothing depends on launch geometry, on scheduling or on the order atomics land in.  No allocation, no host
// synchronisation; scratch is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_eval_math.h"
#include "bbd_syns_math.h"

namespace {

constexpr int PT = 256;            // threads of the per-pixel kernels
constexpr int RT = 1024;           // threads of the one-workgroup-per-image kernels
constexpr int RW = RT / 64;
constexpr int NN_T = 256;          // nearest neighbour: threads per workgroup
constexpr int NN_Q = 8;            //                    queries per lane
constexpr int NN_TILE = 1024;      //                    targets per LDS tile (16 KB)
constexpr int NN_SPLIT = 8;        //                    target ranges (grid.y)
constexpr int EDT_MAX_W = 8192;    // row pass: one row of int32 in LDS

struct Img {
  size_t off;        // element offset of the image in the ground-truth buffers
  int GH, GW, npx;
  bool ok;
};

__device__ __forceinline__ Img load_img(const int32_t* desc, int i, int px_stride) {
  const BbdEvalRow row = bbd_eval_row(desc, i);
  Img m;
  m.off = row.off;
  m.GH = row.GH;
  m.GW = row.GW;
  m.ok = m.GH >= 1 && m.GW >= 1 && (long)m.GH * (long)m.GW <= (long)px_stride;   // a row that does not fit is skipped
  m.npx = m.ok ? m.GH * m.GW : 0;
  return m;
}

struct PredArgs {
  const float* pred;       // [n,h,w]
  const int32_t* desc;
  int h, w, px_stride;
  float clamp_lo, clamp_hi, scale_factor;
  int flags;
};

__device__ __forceinline__ float pred_at(const PredArgs& a, int img, int y, int x, int GH, int GW) {
  return bbd_eval_resample(a.pred + (size_t)img * a.h * a.w, a.h, a.w, a.scale_factor, a.clamp_lo, a.clamp_hi,
                           a.flags & BBD_EVAL_PRED_IS_DISP, y, x, GH, GW);
}

// ------------------------------------------------------------------------------------------------ edges
__global__ __launch_bounds__(PT) void syns_log_kernel(PredArgs a, float* L) {
  const Img m = load_img(a.desc, blockIdx.y, a.px_stride);
  float* out = L + (size_t)blockIdx.y * a.px_stride;
  for (int p = blockIdx.x * PT + threadIdx.x; p < m.npx; p += gridDim.x * PT) {
    const int y = p / m.GW, x = p - y * m.GW;
    out[p] = bbd_syns_log(pred_at(a, blockIdx.y, y, x, m.GH, m.GW));
  }
}

__global__ __launch_bounds__(PT) void syns_blur_kernel(const int32_t* desc, int px_stride, const float* L, float* B) {
  const Img m = load_img(desc, blockIdx.y, px_stride);
  const float* in = L + (size_t)blockIdx.y * px_stride;
  float* out = B + (size_t)blockIdx.y * px_stride;
  for (int p = blockIdx.x * PT + threadIdx.x; p < m.npx; p += gridDim.x * PT) {
    const int y = p / m.GW, x = p - y * m.GW;
    out[p] = bbd_syns_blur(in, y, x, m.GH, m.GW);
  }
}

__global__ __launch_bounds__(PT) void syns_sobel_kernel(const int32_t* desc, int px_stride, const float* B, double* mag) {
  const Img m = load_img(desc, blockIdx.y, px_stride);
  const float* in = B + (size_t)blockIdx.y * px_stride;
  double* out = mag + (size_t)blockIdx.y * px_stride;
  for (int p = blockIdx.x * PT + threadIdx.x; p < m.npx; p += gridDim.x * PT) {
    const int y = p / m.GW, x = p - y * m.GW;
    out[p] = bbd_syns_sobel_mag(in, y, x, m.GH, m.GW);
  }
}

__global__ __launch_bounds__(RT) void syns_thresh_kernel(const int32_t* desc, int px_stride, const double* mag,
                                                         uint8_t* edge, double* stats) {
  __shared__ double red[RW + 1];
  __shared__ unsigned int s_count;
  const int img = blockIdx.x, tid = threadIdx.x;
  const Img m = load_img(desc, img, px_stride);
  const double* in = mag + (size_t)img * px_stride;
  uint8_t* out = edge + (size_t)img * px_stride;
  if (tid == 0) s_count = 0u;
  double s = 0;
  for (int p = tid; p < m.npx; p += RT) s += in[p];
  const double mean = block_sum<RT>(s, red) / (double)m.npx;    // an empty image: 0 / 0, as np.mean of nothing
  unsigned int c = 0;
  for (int p = tid; p < m.npx; p += RT) {
    const uint8_t e = in[p] > mean ? 1 : 0;
    out[p] = e;
    c += e;
  }
  atomicAdd(&s_count, c);
  __syncthreads();
  if (tid == 0) {
    stats[2 * img] = mean;
    stats[2 * img + 1] = (double)s_count;
  }
}

// ------------------------------------------------------------------------------------------------ distance transform
struct EdtArgs {
  const uint8_t* map;      // image i at map + i * px_stride, or NULL: the target mask valid & gt_edge
  const float* gt;         // (target mask) ragged ground-truth depth
  const uint8_t* gt_edge;  // (target mask) ragged ground-truth edges, same offsets
  const int32_t* desc;
  int32_t* out;            // image i at out + i * px_stride
  uint8_t* mask_out;       // (target mask, may be NULL) the mask itself, image i at mask_out + i * px_stride
  int px_stride;
  float lo, hi;
};

__global__ __launch_bounds__(PT) void syns_edt_col_kernel(EdtArgs a) {
  const Img m = load_img(a.desc, blockIdx.y, a.px_stride);
  const int x = blockIdx.x * PT + threadIdx.x;
  if (!m.ok || m.GW > EDT_MAX_W || x >= m.GW) return;
  int32_t* out = a.out + (size_t)blockIdx.y * a.px_stride;
  const uint8_t* map = a.map ? a.map + (size_t)blockIdx.y * a.px_stride : nullptr;
  int d = BBD_SYNS_EDT_FAR;
  for (int y = 0; y < m.GH; ++y) {                  // downwards: distance to the nearest set pixel above
    const size_t p = (size_t)y * m.GW + x;
    bool set;
    if (map) {
      set = map[p] != 0;
    } else {
      const float g = a.gt[m.off + p];
      set = g > a.lo && g < a.hi && a.gt_edge[m.off + p] != 0;
      if (a.mask_out) a.mask_out[(size_t)blockIdx.y * a.px_stride + p] = set ? 1 : 0;
    }
    d = set ? 0 : (d < BBD_SYNS_EDT_FAR ? d + 1 : BBD_SYNS_EDT_FAR);
    out[p] = d;
  }
  d = BBD_SYNS_EDT_FAR;
  for (int y = m.GH - 1; y >= 0; --y) {             // upwards: the nearer of above and below
    const size_t p = (size_t)y * m.GW + x;
    const int up = out[p];
    d = up == 0 ? 0 : (d < BBD_SYNS_EDT_FAR ? d + 1 : BBD_SYNS_EDT_FAR);
    out[p] = d < up ? d : up;
  }
}

__global__ __launch_bounds__(PT) void syns_edt_row_kernel(EdtArgs a) {
  __shared__ int32_t g2[EDT_MAX_W];
  const Img m = load_img(a.desc, blockIdx.y, a.px_stride);
  const int y = blockIdx.x;
  if (!m.ok || m.GW > EDT_MAX_W || y >= m.GH) return;       // (a row wider than the LDS row is skipped)
  int32_t* row = a.out + (size_t)blockIdx.y * a.px_stride + (size_t)y * m.GW;
  for (int x = threadIdx.x; x < m.GW; x += PT) {
    const int g = row[x];
    g2[x] = g >= BBD_SYNS_EDT_FAR ? BBD_SYNS_EDT_NONE : g * g;
  }
  __syncthreads();
  for (int x0 = 0; x0 < m.GW; x0 += 4 * PT) {       // four pixels per lane share every LDS read
    const int xa = x0 + threadIdx.x, xb = xa + PT, xc = xb + PT, xd = xc + PT;
    int ba = BBD_SYNS_EDT_NONE + EDT_MAX_W * EDT_MAX_W, bb = ba, bc = ba, bd = ba;
    for (int xp = 0; xp < m.GW; ++xp) {
      const int g = g2[xp];
      const int da = xa - xp, db = xb - xp, dc = xc - xp, dd = xd - xp;
      ba = min(ba, da * da + g);
      bb = min(bb, db * db + g);
      bc = min(bc, dc * dc + g);
      bd = min(bd, dd * dd + g);
    }
    if (xa < m.GW) row[xa] = ba;
    if (xb < m.GW) row[xb] = bb;
    if (xc < m.GW) row[xc] = bc;
    if (xd < m.GW) row[xd] = bd;
  }
}

// ------------------------------------------------------------------------------------------------ edge metrics
struct ReduceArgs {
  PredArgs p;
  const float* gt;
  const float* rows;        // [n, BBD_EVAL_OUT] of bbd_depth_metrics: column 7 is the median-scaling ratio
  const uint8_t* pred_edge; // image i at + i * px_stride
  const uint8_t* tgt;
  const int32_t* d_t;
  const int32_t* d_p;
  double* out;              // [n, BBD_SYNS_OUT]
  float lo, hi;
  double th;
};

__global__ __launch_bounds__(RT) void syns_edge_reduce_kernel(ReduceArgs a) {
  __shared__ double red[RW + 1];
  __shared__ unsigned int cnt[4];
  const int img = blockIdx.x, tid = threadIdx.x;
  const Img m = load_img(a.p.desc, img, a.p.px_stride);
  const size_t base = (size_t)img * a.p.px_stride;
  const float* gt = a.gt + m.off;
  const float ratio = a.rows[(size_t)img * BBD_EVAL_OUT + 7];
  if (tid < 4) cnt[tid] = 0u;
  double s_acc = 0, s_comp = 0, s_err = 0;
  unsigned int n_near = 0, n_tgt = 0, n_valid = 0, n_edge = 0;
  for (int p = tid; p < m.npx; p += RT) {
    const bool pe = a.pred_edge[base + p] != 0, tg = a.tgt[base + p] != 0;
    n_edge += pe;
    if (pe) {
      const double dt = sqrt((double)a.d_t[base + p]);
      if (dt < a.th) { s_acc += dt; n_near += 1u; }
    }
    if (tg) { s_comp += sqrt((double)a.d_p[base + p]); n_tgt += 1u; }
    const float g = gt[p];
    if (g > a.lo && g < a.hi) {
      const int y = p / m.GW, x = p - y * m.GW;
      float v = pred_at(a.p, img, y, x, m.GH, m.GW);
      if (!(a.p.flags & BBD_EVAL_NO_MEDIAN_SCALING)) v *= ratio;
      v = v < a.lo ? a.lo : v;
      v = v > a.hi ? a.hi : v;
      s_err += (double)fabsf(v - g);
      n_valid += 1u;
    }
  }
  s_acc = block_sum<RT>(s_acc, red);
  s_comp = block_sum<RT>(s_comp, red);
  s_err = block_sum<RT>(s_err, red);
  atomicAdd(&cnt[0], n_near);
  atomicAdd(&cnt[1], n_tgt);
  atomicAdd(&cnt[2], n_valid);
  atomicAdd(&cnt[3], n_edge);
  __syncthreads();
  if (tid == 0) {
    double* o = a.out + (size_t)img * BBD_SYNS_OUT;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // evaluate_depth.py:94-95: both fall back to th when no predicted edge lies within th of a target edge; with no
    // target pixel at all scipy's transform has no background to measure from and its answer is an artefact: NaN.
    o[0] = cnt[1] == 0u ? nan : (cnt[0] ? s_acc / (double)cnt[0] : a.th);
    o[1] = cnt[1] == 0u ? nan : (cnt[0] ? s_comp / (double)cnt[1] : a.th);
    o[2] = s_err / (double)cnt[2];
    o[3] = (double)cnt[0];
    o[4] = (double)cnt[1];
    o[5] = (double)cnt[2];
    o[6] = (double)cnt[3];
    o[7] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ point clouds
struct CloudArgs {
  PredArgs p;
  const float* gt;
  const float* rows;
  const float* inv_K;       // [3,3] row-major
  float4* pts_p;            // image i at + i * px_stride
  float4* pts_t;
  int32_t* counts;          // [n]
  float lo, hi;
  int pixel_rays;
};

__global__ __launch_bounds__(RT) void syns_cloud_kernel(CloudArgs a) {
  __shared__ int scan[RW];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Img m = load_img(a.p.desc, img, a.p.px_stride);
  const float* gt = a.gt + m.off;
  const float ratio = a.rows[(size_t)img * BBD_EVAL_OUT + 7];
  float iK[9];
  for (int j = 0; j < 9; ++j) iK[j] = a.inv_K[j];
  const int chunk = (m.npx + RT - 1) / RT, p0 = tid * chunk, p1 = min(p0 + chunk, m.npx);
  int c = 0;
  for (int p = p0; p < p1; ++p) {
    const float g = gt[p];
    c += (g > a.lo && g < a.hi) ? 1 : 0;
  }
  int incl = c;                                       // inclusive scan: within the wave, then over the waves
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) scan[wave] = incl;
  __syncthreads();
  int before = 0;
  for (int wv = 0; wv < wave; ++wv) before += scan[wv];
  int k = before + incl - c;                          // slot of this lane's first valid pixel
  if (tid == RT - 1) a.counts[img] = before + incl;
  float4* pp = a.pts_p + (size_t)img * a.p.px_stride;
  float4* pt = a.pts_t + (size_t)img * a.p.px_stride;
  for (int p = p0; p < p1; ++p) {
    const float g = gt[p];
    if (!(g > a.lo && g < a.hi)) continue;
    const int y = p / m.GW, x = p - y * m.GW;
    float v = pred_at(a.p, img, y, x, m.GH, m.GW);     // evaluate_depth.py:254, :286, :291-292
    if (!(a.p.flags & BBD_EVAL_NO_MEDIAN_SCALING)) v *= ratio;
    v = v < a.lo ? a.lo : v;
    v = v > a.hi ? a.hi : v;
    float q[3];
    bbd_syns_backproject(iK, p, m.GH, m.GW, a.pixel_rays, v, q);
    pp[k] = make_float4(q[0], q[1], q[2], 0.0f);
    bbd_syns_backproject(iK, p, m.GH, m.GW, a.pixel_rays, g, q);
    pt[k] = make_float4(q[0], q[1], q[2], 0.0f);
    ++k;
  }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct NNArgs {
  const float* q;            // queries, problem z at q + z * q_stride floats, point i at + i * pt_floats
  const float* t;            // targets, likewise
  const int32_t* counts;     // per-problem point count of BOTH sets (device), or NULL: nq / nt below
  uint32_t* out;             // float bits of min squared distance, problem z at out + z * out_stride; +inf on entry
  long q_stride, t_stride, out_stride;
  int nq, nt, pt_floats;     // pt_floats: 3 (packed xyz) or 4 (xyz + pad)
};

__global__ __launch_bounds__(NN_T) void syns_nn_kernel(NNArgs a) {
  __shared__ float4 tile[NN_TILE];
  const int z = blockIdx.z, tid = threadIdx.x;
  const int nq = a.counts ? a.counts[z] : a.nq, nt = a.counts ? a.counts[z] : a.nt;
  const int q0 = blockIdx.x * (NN_T * NN_Q);
  if (q0 >= nq) return;
  // this workgroup's range of targets: whole tiles, NN_SPLIT ranges
  const int tiles = (nt + NN_TILE - 1) / NN_TILE, per = (tiles + NN_SPLIT - 1) / NN_SPLIT;
  const int t0 = blockIdx.y * per * NN_TILE, t1 = min(nt, t0 + per * NN_TILE);
  if (t0 >= t1) return;
  const float* qs = a.q + (size_t)z * a.q_stride;
  const float* ts = a.t + (size_t)z * a.t_stride;
  // two queries per packed register: the subtractions, products and sums below are v_pk_add_f32 / v_pk_mul_f32, one
  // IEEE operation per component, the same values as bbd_syns_dist2 on each query
  f32x2 qx[NN_Q / 2], qy[NN_Q / 2], qz[NN_Q / 2];
  float best[NN_Q];
#pragma unroll
  for (int k = 0; k < NN_Q; ++k) {
    const int i = q0 + k * NN_T + tid;
    const float* s = qs + (size_t)(i < nq ? i : 0) * a.pt_floats;
    qx[k >> 1][k & 1] = s[0]; qy[k >> 1][k & 1] = s[1]; qz[k >> 1][k & 1] = s[2];
    best[k] = __uint_as_float(0x7f800000u);
  }
  for (int tb = t0; tb < t1; tb += NN_TILE) {
    const int cnt = min(NN_TILE, t1 - tb);
    __syncthreads();
    for (int j = tid; j < NN_TILE; j += NN_T) {
      // the tail of the last tile repeats its first target: a duplicate never changes a minimum
      const float* s = ts + (size_t)(tb + (j < cnt ? j : 0)) * a.pt_floats;
      tile[j] = make_float4(s[0], s[1], s[2], 0.0f);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < NN_TILE; ++j) {
      const float4 t = tile[j];
      const f32x2 tx = {t.x, t.x}, ty = {t.y, t.y}, tz = {t.z, t.z};
#pragma unroll
      for (int k = 0; k < NN_Q / 2; ++k) {
        const f32x2 dx = qx[k] - tx, dy = qy[k] - ty, dz = qz[k] - tz;
        const f32x2 d = (dx * dx + dy * dy) + dz * dz;
        best[2 * k] = fminf(best[2 * k], d[0]);
        best[2 * k + 1] = fminf(best[2 * k + 1], d[1]);
      }
    }
  }
  uint32_t* out = a.out + (size_t)z * a.out_stride;
#pragma unroll
  for (int k = 0; k < NN_Q; ++k) {
    const int i = q0 + k * NN_T + tid;
    if (i < nq) atomicMin(out + i, __float_as_uint(best[k]));
  }
}

struct CloudReduceArgs {
  const float* nn_p;         // image i at + i * px_stride
  const float* nn_t;
  const int32_t* counts;
  float* out;                // [n, BBD_SYNS_CLOUD_OUT]
  int px_stride;
  float th;
};

__global__ __launch_bounds__(RT) void syns_cloud_reduce_kernel(CloudReduceArgs a) {
  __shared__ unsigned int cnt[2];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int N = a.counts[img];
  const float* np_ = a.nn_p + (size_t)img * a.px_stride;
  const float* nt_ = a.nn_t + (size_t)img * a.px_stride;
  if (tid < 2) cnt[tid] = 0u;
  __syncthreads();
  unsigned int cp = 0, ct = 0;
  for (int i = tid; i < N; i += RT) {
    cp += sqrtf(np_[i]) < a.th ? 1u : 0u;
    ct += sqrtf(nt_[i]) < a.th ? 1u : 0u;
  }
  atomicAdd(&cnt[0], cp);
  atomicAdd(&cnt[1], ct);
  __syncthreads();
  if (tid == 0) {
    // (x < th).float().mean(): a float32 sum of zeros and ones is exact below 2^24, then one division
    const float P = (float)cnt[0] / (float)N, R = (float)cnt[1] / (float)N;
    float f, iou;
    bbd_syns_f_iou(P, R, &f, &iou);
    float* o = a.out + (size_t)img * BBD_SYNS_CLOUD_OUT;
    o[0] = f; o[1] = iou; o[2] = P; o[3] = R; o[4] = (float)cnt[0]; o[5] = (float)cnt[1]; o[6] = (float)N; o[7] = 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline int tiles_for(long px) { const long t = (px + PT - 1) / PT; return (int)(t < 1 ? 1 : (t > 4096 ? 4096 : t)); }

bool sizes_ok(int n, int px_stride, int max_h, int max_w) {
  return n > 0 && n <= 65535 && px_stride >= 4 && (px_stride & 3) == 0 && max_h >= 1 && max_w >= 1 &&
         (long)max_h * (long)max_w <= (long)px_stride;
}

int edt_size_status(int max_h, int max_w) {
  if (max_w > EDT_MAX_W || max_h >= BBD_SYNS_EDT_FAR) return BBD_E_TOOMANY;
  if ((long)max_h * max_h + (long)max_w * max_w >= (long)BBD_SYNS_EDT_NONE) return BBD_E_TOOMANY;
  return 0;
}

void launch_edt(const EdtArgs& a, int n, int max_h, int max_w, hipStream_t st) {
  hipLaunchKernelGGL(syns_edt_col_kernel, dim3((unsigned)((max_w + PT - 1) / PT), (unsigned)n), dim3(PT), 0, st, a);
  hipLaunchKernelGGL(syns_edt_row_kernel, dim3((unsigned)max_h, (unsigned)n), dim3(PT), 0, st, a);
}

PredArgs pred_args(const float* pred, const int32_t* desc, int h, int w, int px_stride, double clamp_lo,
                   double clamp_hi, double scale_factor, int flags) {
  PredArgs p;
  p.pred = pred; p.desc = desc; p.h = h; p.w = w; p.px_stride = px_stride;
  p.clamp_lo = (float)clamp_lo; p.clamp_hi = (float)clamp_hi; p.scale_factor = (float)scale_factor; p.flags = flags;
  return p;
}

}  // namespace

extern "C" int bbd_syns_scratch_ints(int n, int px_stride) {
  if (n <= 0 || px_stride < 4 || (px_stride & 3)) return BBD_E_BADARG;
  const long ints = (long)n * (10L * px_stride + 16L);
  return ints > 0x7fffffffL ? BBD_E_TOOMANY : (int)ints;
}

extern "C" int bbd_syns_pred_edges(const float* pred, const int32_t* desc, int32_t* scratch, int scratch_ints,
                                   uint8_t* edge, double* stats, int n, int h, int w, int px_stride, int max_h,
                                   int max_w, double clamp_lo, double clamp_hi, int flags, void* stream) {
  if (!pred || !desc || !scratch || !edge || !stats || h < 1 || w < 1 || !sizes_ok(n, px_stride, max_h, max_w) ||
      (flags & ~BBD_EVAL_PRED_IS_DISP))
    return BBD_E_BADARG;
  if ((long)scratch_ints < 4L * n * px_stride) return BBD_E_BADARG;
  // the edges are taken on the prediction before any scaling (evaluate_depth.py:254-265): scale factor 1
  const PredArgs p = pred_args(pred, desc, h, w, px_stride, clamp_lo, clamp_hi, 1.0, flags);
  float* L = reinterpret_cast<float*>(scratch);
  float* B = L + (size_t)n * px_stride;
  double* mag = reinterpret_cast<double*>(B + (size_t)n * px_stride);   // 8-byte aligned: px_stride is a multiple of 4
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles_for((long)max_h * max_w), (unsigned)n);
  hipLaunchKernelGGL(syns_log_kernel, grid, dim3(PT), 0, st, p, L);
  hipLaunchKernelGGL(syns_blur_kernel, grid, dim3(PT), 0, st, desc, px_stride, (const float*)L, B);
  hipLaunchKernelGGL(syns_sobel_kernel, grid, dim3(PT), 0, st, desc, px_stride, (const float*)B, mag);
  hipLaunchKernelGGL(syns_thresh_kernel, dim3((unsigned)n), dim3(RT), 0, st, desc, px_stride, (const double*)mag, edge,
                     stats);
  return launch_status();
}

extern "C" int bbd_syns_edt(const uint8_t* map, const int32_t* desc, int32_t* out, int n, int px_stride, int max_h,
                            int max_w, void* stream) {
  if (!map || !desc || !out || !sizes_ok(n, px_stride, max_h, max_w)) return BBD_E_BADARG;
  const int rc = edt_size_status(max_h, max_w);
  if (rc) return rc;
  EdtArgs a;
  a.map = map; a.gt = nullptr; a.gt_edge = nullptr; a.desc = desc; a.out = out; a.mask_out = nullptr;
  a.px_stride = px_stride; a.lo = 0.0f; a.hi = 0.0f;
  launch_edt(a, n, max_h, max_w, static_cast<hipStream_t>(stream));
  return launch_status();
}

extern "C" int bbd_syns_edge_metrics(const float* pred, const float* gt, const uint8_t* gt_edge,
                                     const uint8_t* pred_edge, const int32_t* desc, const float* rows,
                                     int32_t* scratch, int scratch_ints, double* out, int n, int h, int w,
                                     int px_stride, int max_h, int max_w, double min_depth, double max_depth,
                                     double clamp_lo, double clamp_hi, double scale_factor, double th, int flags,
                                     void* stream) {
  if (!pred || !gt || !gt_edge || !pred_edge || !desc || !rows || !scratch || !out || h < 1 || w < 1 ||
      !sizes_ok(n, px_stride, max_h, max_w) || (flags & ~(BBD_EVAL_PRED_IS_DISP | BBD_EVAL_NO_MEDIAN_SCALING)))
    return BBD_E_BADARG;
  const int rc = edt_size_status(max_h, max_w);
  if (rc) return rc;
  if ((long)scratch_ints < (long)n * px_stride * 2L + (long)n * (px_stride / 4)) return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* d_t = scratch;
  int32_t* d_p = d_t + (size_t)n * px_stride;
  uint8_t* tgt = reinterpret_cast<uint8_t*>(d_p + (size_t)n * px_stride);
  EdtArgs e;
  e.map = nullptr; e.gt = gt; e.gt_edge = gt_edge; e.desc = desc; e.out = d_t; e.mask_out = tgt;
  e.px_stride = px_stride; e.lo = (float)min_depth; e.hi = (float)max_depth;
  launch_edt(e, n, max_h, max_w, st);
  e.map = pred_edge; e.out = d_p; e.mask_out = nullptr;
  launch_edt(e, n, max_h, max_w, st);
  ReduceArgs r;
  r.p = pred_args(pred, desc, h, w, px_stride, clamp_lo, clamp_hi, scale_factor, flags);
  r.gt = gt; r.rows = rows; r.pred_edge = pred_edge; r.tgt = tgt; r.d_t = d_t; r.d_p = d_p; r.out = out;
  r.lo = (float)min_depth; r.hi = (float)max_depth; r.th = th;
  hipLaunchKernelGGL(syns_edge_reduce_kernel, dim3((unsigned)n), dim3(RT), 0, st, r);
  return launch_status();
}

extern "C" int bbd_chamfer_nn(const float* a, const float* b, int na, int nb, float* nn_a, float* nn_b, void* stream) {
  if (na < 0 || nb < 0 || (na > 0 && (!a || !nn_a)) || (nb > 0 && (!b || !nn_b))) return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  if (na > 0) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(nn_a), 0x7f800000, (size_t)na, st);
  if (e == hipSuccess && nb > 0) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(nn_b), 0x7f800000, (size_t)nb, st);
  if (e != hipSuccess) return (int)e;
  if (na == 0 || nb == 0) return 0;                  // the minimum over nothing stays +inf
  NNArgs q;
  q.counts = nullptr; q.q_stride = q.t_stride = q.out_stride = 0; q.pt_floats = 3;
  q.q = a; q.t = b; q.nq = na; q.nt = nb; q.out = reinterpret_cast<uint32_t*>(nn_a);
  hipLaunchKernelGGL(syns_nn_kernel, dim3((unsigned)((na + NN_T * NN_Q - 1) / (NN_T * NN_Q)), NN_SPLIT, 1), dim3(NN_T), 0, st, q);
  q.q = b; q.t = a; q.nq = nb; q.nt = na; q.out = reinterpret_cast<uint32_t*>(nn_b);
  hipLaunchKernelGGL(syns_nn_kernel, dim3((unsigned)((nb + NN_T * NN_Q - 1) / (NN_T * NN_Q)), NN_SPLIT, 1), dim3(NN_T), 0, st, q);
  return launch_status();
}

extern "C" int bbd_syns_pointcloud(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                                   const float* inv_K, int32_t* scratch, int scratch_ints, float* out, int n, int h,
                                   int w, int px_stride, int max_h, int max_w, double min_depth, double max_depth,
                                   double clamp_lo, double clamp_hi, double th, int flags, void* stream) {
  const int eval_flags = flags & (BBD_EVAL_PRED_IS_DISP | BBD_EVAL_NO_MEDIAN_SCALING);
  if (!pred || !gt || !desc || !rows || !inv_K || !scratch || !out || h < 1 || w < 1 ||
      !sizes_ok(n, px_stride, max_h, max_w) || (flags & ~(eval_flags | BBD_SYNS_RAYS_PIXEL)))
    return BBD_E_BADARG;
  if ((long)scratch_ints < (long)n * (10L * px_stride + 16L)) return BBD_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float4* pts_p = reinterpret_cast<float4*>(scratch);                  // 16-byte aligned as the scratch itself must be
  float4* pts_t = pts_p + (size_t)n * px_stride;
  float* nn_p = reinterpret_cast<float*>(pts_t + (size_t)n * px_stride);
  float* nn_t = nn_p + (size_t)n * px_stride;
  int32_t* counts = reinterpret_cast<int32_t*>(nn_t + (size_t)n * px_stride);
  if (reinterpret_cast<uintptr_t>(scratch) & 15u) return BBD_E_BADARG;
  const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(nn_p), 0x7f800000, (size_t)2 * n * px_stride, st);
  if (e != hipSuccess) return (int)e;
  CloudArgs c;
  // the clouds take the median-scaled, clamped prediction without opt.pred_depth_scale_factor (evaluate_depth.py:255)
  c.p = pred_args(pred, desc, h, w, px_stride, clamp_lo, clamp_hi, 1.0, eval_flags);
  c.gt = gt; c.rows = rows; c.inv_K = inv_K; c.pts_p = pts_p; c.pts_t = pts_t; c.counts = counts;
  c.lo = (float)min_depth; c.hi = (float)max_depth; c.pixel_rays = (flags & BBD_SYNS_RAYS_PIXEL) ? 1 : 0;
  hipLaunchKernelGGL(syns_cloud_kernel, dim3((unsigned)n), dim3(RT), 0, st, c);
  NNArgs q;
  q.counts = counts; q.nq = q.nt = 0; q.pt_floats = 4;
  q.q_stride = q.t_stride = 4L * px_stride; q.out_stride = px_stride;
  const dim3 grid((unsigned)(((long)max_h * max_w + NN_T * NN_Q - 1) / (NN_T * NN_Q)), NN_SPLIT, (unsigned)n);
  q.q = reinterpret_cast<const float*>(pts_p); q.t = reinterpret_cast<const float*>(pts_t);
  q.out = reinterpret_cast<uint32_t*>(nn_p);
  hipLaunchKernelGGL(syns_nn_kernel, grid, dim3(NN_T), 0, st, q);
  q.q = reinterpret_cast<const float*>(pts_t); q.t = reinterpret_cast<const float*>(pts_p);
  q.out = reinterpret_cast<uint32_t*>(nn_t);
  hipLaunchKernelGGL(syns_nn_kernel, grid, dim3(NN_T), 0, st, q);
  CloudReduceArgs r;
  r.nn_p = nn_p; r.nn_t = nn_t; r.counts = counts; r.out = out; r.px_stride = px_stride; r.th = (float)th;
  hipLaunchKernelGGL(syns_cloud_reduce_kernel, dim3((unsigned)n), dim3(RT), 0, st, r);
  return launch_status();
}
