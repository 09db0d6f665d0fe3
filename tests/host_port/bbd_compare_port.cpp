// Host port of bbd_compare.hip for the CPU test tier: the same per-pixel functions (bbd_compare_math.h and what it
// includes) in plain loops.  Same C signatures as bbd_gt_viz / bbd_error_map minus `stream`.  hp_depth_metrics restates
// bbd_eval.hip's kernel the same way (its medians by sorting the order keys, its sums in float64 in pixel order), so that
// the rows bbd_error_map reads exist on the host too.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_panel_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_compare_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_ragged_math.h"

namespace {

struct Map : BbdEvalRow {
  size_t npx;
};

Map load_map(const int32_t* desc, int i) {
  Map m;
  static_cast<BbdEvalRow&>(m) = bbd_eval_row(desc, i);
  m.npx = m.GH > 0 && m.GW > 0 ? (size_t)m.GH * (size_t)m.GW : 0;
  return m;
}

void pack_lut(uint32_t* packed, const uint8_t* lut) {
  for (int i = 0; i < 256; ++i) packed[i] = bbd_pack_rgb(lut + 3 * i);
}

}  // namespace

extern "C" int hp_gt_viz_scratch_ints(int n) { return n > 0 && n <= 65535 ? 2 * n : 0; }

extern "C" int hp_gt_viz(const float* gt, const int32_t* desc, const uint8_t* lut, uint8_t* out_u8, float* stats,
                         int32_t* scratch, int n, double max_inv_d) {
  if (!gt || !desc || !lut || !out_u8 || !stats || !scratch || n < 1 || n > 65535) return BBD_E_BADARG;
  const float max_inv = (float)max_inv_d;
  uint32_t packed[256];
  pack_lut(packed, lut);
  for (int img = 0; img < n; ++img) {
    const Map m = load_map(desc, img);
    const float* g = gt + m.off;
    uint32_t inv_min = 0u, max_key = 0u;
    for (size_t i = 0; i < m.npx; ++i) bbd_panel_minmax_update(bbd_compare_gt_inverse(g[i], max_inv), &inv_min, &max_key);
    float vmin, vmax;
    bbd_panel_minmax_values(inv_min, max_key, &vmin, &vmax);
    stats[(size_t)img * 2] = vmin;
    stats[(size_t)img * 2 + 1] = vmax;
    for (size_t i = 0; i < m.npx; ++i)
      bbd_put_rgb(out_u8 + 3 * (m.off + i), packed[bbd_viz_lut_index(bbd_compare_gt_inverse(g[i], max_inv), vmin, vmax)]);
  }
  return 0;
}

extern "C" int hp_error_map(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                            const uint8_t* images, const uint8_t* lut, uint8_t* out_u8, float* out_float, int n, int h,
                            int w, double min_depth, double max_depth, double scale_factor, double err_max_d, int radius,
                            int flags) {
  if (!pred || !gt || !desc || !rows || !lut || !out_u8 || n < 1 || n > 65535 || h < 1 || w < 1) return BBD_E_BADARG;
  if (radius < 0 || radius > BBD_ERROR_MAP_MAX_RADIUS || (flags & ~BBD_EVAL_NO_MEDIAN_SCALING)) return BBD_E_BADARG;
  const float err_max = (float)err_max_d;
  uint32_t packed[256];
  pack_lut(packed, lut);
  for (int img = 0; img < n; ++img) {
    const Map m = load_map(desc, img);
    const float* row = rows + (size_t)img * BBD_EVAL_OUT;
    const bool scored = row[10] != 0.0f;
    BbdCompareMap cm;
    cm.gt = gt + m.off;
    cm.pred = pred + (size_t)img * h * w;
    cm.GH = m.GH; cm.GW = m.GW; cm.r0 = m.r0; cm.r1 = m.r1; cm.c0 = m.c0; cm.c1 = m.c1; cm.h = h; cm.w = w;
    cm.min_depth = (float)min_depth; cm.max_depth = (float)max_depth; cm.scale_factor = (float)scale_factor;
    cm.ratio = row[7]; cm.flags = flags; cm.radius = radius;
    for (int y = 0; y < m.GH; ++y)
      for (int x = 0; x < m.GW; ++x) {
        const size_t i = m.off + (size_t)y * m.GW + x;
        float e = 0.0f, own = 0.0f;
        const bool any = scored && bbd_compare_error_max(cm, y, x, &e);
        if (out_float) {
          const bool valid = scored && bbd_compare_error_at(cm, y, x, &own);
          out_float[i] = valid ? own : bbd_viz_bits_float(BBD_COMPARE_NAN_BITS);
        }
        uint32_t c = 0u;
        if (any) c = packed[bbd_viz_lut_index(e, 0.0f, err_max)];
        else if (images) c = bbd_compare_grey(images + 3 * i);
        bbd_put_rgb(out_u8 + 3 * i, c);
      }
  }
  return 0;
}

extern "C" int hp_depth_metrics(const float* pred, const float* gt, const int32_t* desc, float* out, int n, int h, int w,
                                double min_depth_d, double max_depth_d, double clamp_lo, double clamp_hi,
                                double scale_factor, int flags) {
  if (!pred || !gt || !desc || !out || n <= 0 || h < 1 || w < 1) return BBD_E_BADARG;
  const float min_depth = (float)min_depth_d, max_depth = (float)max_depth_d;
  for (int img = 0; img < n; ++img) {
    const Map m = load_map(desc, img);
    const float* g_map = gt + m.off;
    const float* pr = pred + (size_t)img * h * w;
    float* o = out + (size_t)img * BBD_EVAL_OUT;
    std::vector<float> gs, ps;
    for (int y = m.r0; y < m.r1; ++y)
      for (int x = m.c0; x < m.c1; ++x) {
        const float g = g_map[(size_t)y * m.GW + x];
        if (!(g > min_depth && g < max_depth)) continue;
        gs.push_back(g);
        ps.push_back(bbd_eval_resample(pr, h, w, (float)scale_factor, (float)clamp_lo, (float)clamp_hi, flags, y, x, m.GH,
                                       m.GW));
      }
    const size_t count = gs.size();
    if (count == 0) {
      for (int k = 0; k < BBD_EVAL_OUT; ++k) o[k] = k == 10 ? 0.0f : bbd_viz_bits_float(0x7fc00000u);
      continue;
    }
    auto median = [&](const std::vector<float>& v) {
      std::vector<uint32_t> keys(v.size());
      for (size_t i = 0; i < v.size(); ++i) keys[i] = bbd_viz_order_key(v[i]);
      std::sort(keys.begin(), keys.end());
      float med = bbd_viz_key_value(keys[(count - 1) / 2]);
      if (flags & BBD_EVAL_MEDIAN_MIDPOINT) med = (med + bbd_viz_key_value(keys[count / 2])) / 2.0f;
      return med;
    };
    const float med_gt = median(gs), med_pr = median(ps);
    const float ratio = (flags & BBD_EVAL_NO_MEDIAN_SCALING) ? 1.0f : med_gt / med_pr;
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < count; ++i) {
      const float g = gs[i];
      float p = ps[i];
      if (!(flags & BBD_EVAL_NO_MEDIAN_SCALING)) p *= ratio;
      p = p < min_depth ? min_depth : p;
      p = p > max_depth ? max_depth : p;
      const float t0 = g / p, t1 = p / g;
      const float th = t0 > t1 ? t0 : t1;
      s[4] += th < 1.25f ? 1.0 : 0.0;
      s[5] += th < 1.5625f ? 1.0 : 0.0;
      s[6] += th < 1.953125f ? 1.0 : 0.0;
      const float df = g - p;
      const float d2 = df * df;
      const float dl = logf(g) - logf(p);
      s[2] += (double)d2;
      s[3] += (double)(dl * dl);
      s[0] += (double)(fabsf(df) / g);
      s[1] += (double)(d2 / g);
    }
    for (int k = 0; k < 7; ++k) {
      double mean = s[k] / (double)count;
      if (k == 2 || k == 3) mean = sqrt(mean);
      o[k] = (float)mean;
    }
    o[7] = ratio; o[8] = med_gt; o[9] = med_pr; o[10] = (float)count; o[11] = 0.0f;
  }
  return 0;
}
