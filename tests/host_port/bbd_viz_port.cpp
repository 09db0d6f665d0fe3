// Host port of bbd_viz.hip for the CPU test tier: the same per-pixel functions (bbd_math.h, bbd_viz_math.h), the
// order statistics by std::nth_element instead of the radix select.  Same C signature as bbd_disp_viz minus `stream`.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_ragged_math.h"
#include "../../baseboostdepth_amd/csrc/bbd_viz_math.h"

extern "C" int hp_disp_viz_scratch_ints(int n) { return n > 0 ? n : 0; }

extern "C" int hp_disp_viz(const float* disp, const int32_t* desc, const uint8_t* lut, uint8_t* out_u8, float* out_float,
                           float* stats, int32_t* scratch, int n, int h, int w, double min_disp, double max_disp,
                           double percentile) {
  if (!disp || !desc || !lut || !out_u8 || !stats || !scratch || n <= 0 || h < 1 || w < 1) return BBD_E_BADARG;
  if (!(percentile > 0.0 && percentile <= 100.0)) return BBD_E_BADARG;
  const float lo = (float)min_disp, span = (float)(max_disp - min_disp), q = bbd_viz_quantile(percentile);
  for (int img = 0; img < n; ++img) {
    const int32_t* d = desc + (size_t)img * BBD_VIZ_DESC;
    const size_t off = bbd_join64(d[0], d[1]);
    const int H0 = d[2], W0 = d[3];
    const uint32_t npx = (uint32_t)H0 * (uint32_t)W0;
    if (npx == 0) continue;
    const float* src = disp + (size_t)img * h * w;
    std::vector<float> s(npx);
    for (int y = 0; y < H0; ++y) {
      int y0, y1;
      float ly0, ly1;
      bbd_viz_up_src(y, h, H0, &y0, &y1, &ly0, &ly1);
      for (int x = 0; x < W0; ++x) {
        int x0, x1;
        float lx0, lx1;
        bbd_viz_up_src(x, w, W0, &x0, &x1, &lx0, &lx1);
        const float* r0 = src + (size_t)y0 * w;
        const float* r1 = src + (size_t)y1 * w;
        const float v = bbd_up_blend(r0[x0], r0[x1], r1[x0], r1[x1], ly0, ly1, lx0, lx1, H0 + W0 <= 128);
        s[(size_t)y * W0 + x] = bbd_viz_scaled(v, lo, span);
      }
    }
    uint32_t rl, ru;
    float gamma;
    bbd_viz_ranks(npx, q, &rl, &ru, &gamma);
    std::vector<uint32_t> keys(npx);
    for (uint32_t i = 0; i < npx; ++i) keys[i] = bbd_viz_order_key(s[i]);
    std::nth_element(keys.begin(), keys.begin() + rl, keys.end());
    const float lower = bbd_viz_key_value(keys[rl]);
    std::nth_element(keys.begin(), keys.begin() + ru, keys.end());
    const float upper = bbd_viz_key_value(keys[ru]);
    const float vmin = bbd_viz_key_value(*std::min_element(keys.begin(), keys.end()));
    const float vmax = bbd_viz_lerp(lower, upper, gamma);
    float* st = stats + (size_t)img * 4;
    st[0] = vmin; st[1] = vmax; st[2] = lower; st[3] = upper;
    for (uint32_t i = 0; i < npx; ++i) {
      bbd_put_rgb(out_u8 + 3 * (off + i), bbd_pack_rgb(lut + 3 * bbd_viz_lut_index(s[i], vmin, vmax)));
      if (out_float) out_float[off + i] = s[i];
    }
  }
  return 0;
}
