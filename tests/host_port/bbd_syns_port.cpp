// Host port of bbd_syns.hip for the CPU test tier: the same per-pixel functions (bbd_syns_math.h, bbd_eval_math.h),
// the same two-pass distance transform and the same fp64 summation order (1024 lane-strided accumulators, a tree over
// each group of 64, the 16 groups in order), run serially.  Same C signatures as the bbd_syns_* entries minus `stream`.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_eval_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_ragged_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_syns_math.h"

namespace {

struct Img {
  size_t off;
  int GH, GW, npx;
};

Img load_img(const int32_t* desc, int i, int px_stride) {
  const BbdEvalRow row = bbd_eval_row(desc, i);
  Img m;
  m.off = row.off;
  m.GH = row.GH;
  m.GW = row.GW;
  const bool ok = m.GH >= 1 && m.GW >= 1 && (long)m.GH * m.GW <= (long)px_stride;
  m.npx = ok ? m.GH * m.GW : 0;
  return m;
}

// the kernels' block_sum: element p goes to accumulator p % 1024
struct Sum1024 {
  double acc[1024];
  Sum1024() { std::fill(acc, acc + 1024, 0.0); }
  void add(int p, double v) { acc[p & 1023] += v; }
  double total() const {
    double s = 0;
    for (int wv = 0; wv < 16; ++wv) {
      double v[64];
      std::copy(acc + 64 * wv, acc + 64 * wv + 64, v);
      for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < 64; ++l) v[l] = v[l] + (l + o < 64 ? v[l + o] : v[l]);   // __shfl_down: own value past the end
      s += v[0];
    }
    return s;
  }
};

bool sizes_ok(int n, int px_stride, int max_h, int max_w) {
  return n > 0 && n <= 65535 && px_stride >= 4 && (px_stride & 3) == 0 && max_h >= 1 && max_w >= 1 &&
         (long)max_h * (long)max_w <= (long)px_stride;
}

int edt_size_status(int max_h, int max_w) {
  if (max_w > 8192 || max_h >= BBD_SYNS_EDT_FAR) return BBD_E_TOOMANY;
  if ((long)max_h * max_h + (long)max_w * max_w >= (long)BBD_SYNS_EDT_NONE) return BBD_E_TOOMANY;
  return 0;
}

void edt(const uint8_t* map, int GH, int GW, int32_t* out) {
  for (int x = 0; x < GW; ++x) {
    int d = BBD_SYNS_EDT_FAR;
    for (int y = 0; y < GH; ++y) {
      d = map[(size_t)y * GW + x] ? 0 : (d < BBD_SYNS_EDT_FAR ? d + 1 : BBD_SYNS_EDT_FAR);
      out[(size_t)y * GW + x] = d;
    }
    d = BBD_SYNS_EDT_FAR;
    for (int y = GH - 1; y >= 0; --y) {
      const int up = out[(size_t)y * GW + x];
      d = up == 0 ? 0 : (d < BBD_SYNS_EDT_FAR ? d + 1 : BBD_SYNS_EDT_FAR);
      out[(size_t)y * GW + x] = std::min(d, up);
    }
  }
  std::vector<int32_t> g2(GW);
  for (int y = 0; y < GH; ++y) {
    int32_t* row = out + (size_t)y * GW;
    for (int x = 0; x < GW; ++x) g2[x] = row[x] >= BBD_SYNS_EDT_FAR ? BBD_SYNS_EDT_NONE : row[x] * row[x];
    for (int x = 0; x < GW; ++x) {
      int best = BBD_SYNS_EDT_NONE + 8192 * 8192;
      for (int xp = 0; xp < GW; ++xp) best = std::min(best, (x - xp) * (x - xp) + g2[xp]);
      row[x] = best;
    }
  }
}

float pred_at(const float* pred, int img, int h, int w, float scale, float clo, float chi, int flags, int y, int x,
              int GH, int GW) {
  return bbd_eval_resample(pred + (size_t)img * h * w, h, w, scale, clo, chi, flags & BBD_EVAL_PRED_IS_DISP, y, x, GH, GW);
}

void nn_one_way(const float* q, const float* t, int nq, int nt, int pt_floats, float* out) {
  for (int i = 0; i < nq; ++i) {
    const float* a = q + (size_t)i * pt_floats;
    float best = std::numeric_limits<float>::infinity();
    for (int j = 0; j < nt; ++j) {
      const float* b = t + (size_t)j * pt_floats;
      best = fminf(best, bbd_syns_dist2(a[0], a[1], a[2], b[0], b[1], b[2]));
    }
    out[i] = best;
  }
}

}  // namespace

extern "C" int hp_syns_scratch_ints(int n, int px_stride) {
  if (n <= 0 || px_stride < 4 || (px_stride & 3)) return BBD_E_BADARG;
  const long ints = (long)n * (10L * px_stride + 16L);
  return ints > 0x7fffffffL ? BBD_E_TOOMANY : (int)ints;
}

extern "C" int hp_syns_pred_edges(const float* pred, const int32_t* desc, int32_t* scratch, int scratch_ints,
                                  uint8_t* edge, double* stats, int n, int h, int w, int px_stride, int max_h,
                                  int max_w, double clamp_lo, double clamp_hi, int flags) {
  if (!pred || !desc || !scratch || !edge || !stats || h < 1 || w < 1 || !sizes_ok(n, px_stride, max_h, max_w) ||
      (flags & ~BBD_EVAL_PRED_IS_DISP))
    return BBD_E_BADARG;
  if ((long)scratch_ints < 4L * n * px_stride) return BBD_E_BADARG;
  for (int i = 0; i < n; ++i) {
    const Img m = load_img(desc, i, px_stride);
    std::vector<float> L(m.npx), B(m.npx);
    std::vector<double> mag(m.npx);
    for (int p = 0; p < m.npx; ++p)
      L[p] = bbd_syns_log(pred_at(pred, i, h, w, 1.0f, (float)clamp_lo, (float)clamp_hi, flags, p / m.GW, p % m.GW, m.GH, m.GW));
    for (int p = 0; p < m.npx; ++p) B[p] = bbd_syns_blur(L.data(), p / m.GW, p % m.GW, m.GH, m.GW);
    Sum1024 s;
    for (int p = 0; p < m.npx; ++p) {
      mag[p] = bbd_syns_sobel_mag(B.data(), p / m.GW, p % m.GW, m.GH, m.GW);
      s.add(p, mag[p]);
    }
    const double mean = s.total() / (double)m.npx;
    long c = 0;
    for (int p = 0; p < m.npx; ++p) {
      edge[(size_t)i * px_stride + p] = mag[p] > mean ? 1 : 0;
      c += mag[p] > mean ? 1 : 0;
    }
    stats[2 * i] = mean;
    stats[2 * i + 1] = (double)c;
  }
  return 0;
}

extern "C" int hp_syns_edt(const uint8_t* map, const int32_t* desc, int32_t* out, int n, int px_stride, int max_h,
                           int max_w) {
  if (!map || !desc || !out || !sizes_ok(n, px_stride, max_h, max_w)) return BBD_E_BADARG;
  const int rc = edt_size_status(max_h, max_w);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    const Img m = load_img(desc, i, px_stride);
    if (m.npx) edt(map + (size_t)i * px_stride, m.GH, m.GW, out + (size_t)i * px_stride);
  }
  return 0;
}

extern "C" int hp_syns_edge_metrics(const float* pred, const float* gt, const uint8_t* gt_edge,
                                    const uint8_t* pred_edge, const int32_t* desc, const float* rows,
                                    int32_t* scratch, int scratch_ints, double* out, int n, int h, int w,
                                    int px_stride, int max_h, int max_w, double min_depth, double max_depth,
                                    double clamp_lo, double clamp_hi, double scale_factor, double th, int flags) {
  if (!pred || !gt || !gt_edge || !pred_edge || !desc || !rows || !scratch || !out || h < 1 || w < 1 ||
      !sizes_ok(n, px_stride, max_h, max_w) || (flags & ~(BBD_EVAL_PRED_IS_DISP | BBD_EVAL_NO_MEDIAN_SCALING)))
    return BBD_E_BADARG;
  const int rc = edt_size_status(max_h, max_w);
  if (rc) return rc;
  if ((long)scratch_ints < (long)n * px_stride * 2L + (long)n * (px_stride / 4)) return BBD_E_BADARG;
  const float lo = (float)min_depth, hi = (float)max_depth;
  for (int i = 0; i < n; ++i) {
    const Img m = load_img(desc, i, px_stride);
    const float* g = gt + m.off;
    const uint8_t* pe = pred_edge + (size_t)i * px_stride;
    std::vector<uint8_t> tgt(m.npx);
    std::vector<int32_t> d_t(m.npx), d_p(m.npx);
    for (int p = 0; p < m.npx; ++p) tgt[p] = (g[p] > lo && g[p] < hi && gt_edge[m.off + p]) ? 1 : 0;
    if (m.npx) {
      edt(tgt.data(), m.GH, m.GW, d_t.data());
      edt(pe, m.GH, m.GW, d_p.data());
    }
    const float ratio = rows[(size_t)i * BBD_EVAL_OUT + 7];
    Sum1024 s_acc, s_comp, s_err;
    long n_near = 0, n_tgt = 0, n_valid = 0, n_edge = 0;
    for (int p = 0; p < m.npx; ++p) {
      n_edge += pe[p] ? 1 : 0;
      if (pe[p]) {
        const double dt = sqrt((double)d_t[p]);
        if (dt < th) { s_acc.add(p, dt); ++n_near; }
      }
      if (tgt[p]) { s_comp.add(p, sqrt((double)d_p[p])); ++n_tgt; }
      if (g[p] > lo && g[p] < hi) {
        float v = pred_at(pred, i, h, w, (float)scale_factor, (float)clamp_lo, (float)clamp_hi, flags, p / m.GW, p % m.GW, m.GH, m.GW);
        if (!(flags & BBD_EVAL_NO_MEDIAN_SCALING)) v *= ratio;
        v = v < lo ? lo : v;
        v = v > hi ? hi : v;
        s_err.add(p, (double)fabsf(v - g[p]));
        ++n_valid;
      }
    }
    double* o = out + (size_t)i * BBD_SYNS_OUT;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    o[0] = n_tgt == 0 ? nan : (n_near ? s_acc.total() / (double)n_near : th);
    o[1] = n_tgt == 0 ? nan : (n_near ? s_comp.total() / (double)n_tgt : th);
    o[2] = s_err.total() / (double)n_valid;
    o[3] = (double)n_near; o[4] = (double)n_tgt; o[5] = (double)n_valid; o[6] = (double)n_edge; o[7] = 0.0;
  }
  return 0;
}

extern "C" int hp_chamfer_nn(const float* a, const float* b, int na, int nb, float* nn_a, float* nn_b) {
  if (na < 0 || nb < 0 || (na > 0 && (!a || !nn_a)) || (nb > 0 && (!b || !nn_b))) return BBD_E_BADARG;
  nn_one_way(a, b, na, nb, 3, nn_a);
  nn_one_way(b, a, nb, na, 3, nn_b);
  return 0;
}

extern "C" int hp_syns_pointcloud(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                                  const float* inv_K, int32_t* scratch, int scratch_ints, float* out, int n, int h,
                                  int w, int px_stride, int max_h, int max_w, double min_depth, double max_depth,
                                  double clamp_lo, double clamp_hi, double th, int flags) {
  const int eval_flags = flags & (BBD_EVAL_PRED_IS_DISP | BBD_EVAL_NO_MEDIAN_SCALING);
  if (!pred || !gt || !desc || !rows || !inv_K || !scratch || !out || h < 1 || w < 1 ||
      !sizes_ok(n, px_stride, max_h, max_w) || (flags & ~(eval_flags | BBD_SYNS_RAYS_PIXEL)))
    return BBD_E_BADARG;
  if ((long)scratch_ints < (long)n * (10L * px_stride + 16L)) return BBD_E_BADARG;
  const float lo = (float)min_depth, hi = (float)max_depth;
  for (int i = 0; i < n; ++i) {
    const Img m = load_img(desc, i, px_stride);
    const float* g = gt + m.off;
    const float ratio = rows[(size_t)i * BBD_EVAL_OUT + 7];
    std::vector<float> P, T;
    for (int p = 0; p < m.npx; ++p) {
      if (!(g[p] > lo && g[p] < hi)) continue;
      float v = pred_at(pred, i, h, w, 1.0f, (float)clamp_lo, (float)clamp_hi, eval_flags, p / m.GW, p % m.GW, m.GH, m.GW);
      if (!(flags & BBD_EVAL_NO_MEDIAN_SCALING)) v *= ratio;
      v = v < lo ? lo : v;
      v = v > hi ? hi : v;
      float q[3];
      bbd_syns_backproject(inv_K, p, m.GH, m.GW, (flags & BBD_SYNS_RAYS_PIXEL) ? 1 : 0, v, q);
      P.insert(P.end(), q, q + 3);
      bbd_syns_backproject(inv_K, p, m.GH, m.GW, (flags & BBD_SYNS_RAYS_PIXEL) ? 1 : 0, g[p], q);
      T.insert(T.end(), q, q + 3);
    }
    const int N = (int)(P.size() / 3);
    std::vector<float> nn_p(N), nn_t(N);
    nn_one_way(P.data(), T.data(), N, N, 3, nn_p.data());
    nn_one_way(T.data(), P.data(), N, N, 3, nn_t.data());
    long cp = 0, ct = 0;
    for (int k = 0; k < N; ++k) {
      cp += sqrtf(nn_p[k]) < (float)th ? 1 : 0;
      ct += sqrtf(nn_t[k]) < (float)th ? 1 : 0;
    }
    const float Pr = (float)cp / (float)N, R = (float)ct / (float)N;
    float f, iou;
    bbd_syns_f_iou(Pr, R, &f, &iou);
    float* o = out + (size_t)i * BBD_SYNS_CLOUD_OUT;
    o[0] = f; o[1] = iou; o[2] = Pr; o[3] = R; o[4] = (float)cp; o[5] = (float)ct; o[6] = (float)N; o[7] = 0.0f;
  }
  return 0;
}
