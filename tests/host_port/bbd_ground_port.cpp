// Host port of bbd_ground.hip for the CPU test tier: the argument rules, the depth of a pixel, the ground test and the
// output row are bbd_ground_math.h, shared with the kernels; what the two launches compute - per pixel the scratch code
// and the mask byte, per image the counts and the element of rank (count - 1) / 2 of the ascending heights - is a
// serial loop and an nth_element here.  Same C signatures as the bbd_ground_scale* entries minus `stream`.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_ground_math.h"

extern "C" long hp_ground_scale_scratch_floats(int n, int h, int w) { return bbd_ground_scratch_floats(n, h, w); }

extern "C" int hp_ground_scale(const float* pred, const float* inv_K, float* rows, uint8_t* mask, float* scratch, int n,
                               int h, int w, double camera_height, double cos_threshold, int min_count, int flags) {
  const int rc = bbd_ground_args_status(pred, inv_K, rows, scratch, n, h, w, camera_height, cos_threshold, min_count,
                                        flags);
  if (rc) return rc;
  const size_t npx = (size_t)h * (size_t)w;
  std::vector<uint32_t> heights;
  for (int i = 0; i < n; ++i) {
    const float* p = pred + (size_t)i * npx;
    float* codes = scratch + (size_t)i * npx;
    uint32_t candidates = 0;
    heights.clear();
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        float code = 0.0f;
        if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
          const int rx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, ry[8] = {0, 1, 1, 1, 0, -1, -1, -1};
          float ring[8];
          for (int k = 0; k < 8; ++k) ring[k] = bbd_ground_depth(p[(size_t)(y + ry[k]) * w + (x + rx[k])], flags);
          code = bbd_ground_code(inv_K + (size_t)i * 9, x, y, bbd_ground_depth(p[(size_t)y * w + x], flags), ring,
                                 (float)cos_threshold);
        }
        const uint32_t bits = bbd_ground_float_bits(code);
        codes[(size_t)y * w + x] = code;
        if (mask) mask[(size_t)i * npx + (size_t)y * w + x] = code > 0.0f ? 1 : 0;
        if (bits != 0u) ++candidates;
        if (bits != 0u && bits != BBD_GROUND_CODE_CANDIDATE) heights.push_back(bits);    // positive floats: ordered as bits
      }
    const uint32_t count = (uint32_t)heights.size();
    uint32_t median = 0u;
    if (count) {
      std::nth_element(heights.begin(), heights.begin() + (count - 1) / 2, heights.end());
      median = heights[(count - 1) / 2];
    }
    for (int c = 0; c < BBD_EVAL_OUT; ++c)
      rows[(size_t)i * BBD_EVAL_OUT + c] = bbd_ground_row(c, median, count, candidates, min_count, (float)camera_height);
  }
  return 0;
}
