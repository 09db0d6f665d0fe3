// Host port of bbd_sgm.hip for the CPU test tier: every rule is bbd_sgm_math.h, shared with the kernels; the launches are
// serial loops here, a wave's lanes a loop over d, the cross-lane minimum a running minimum and the atomic add a plain
// addition.  The C signature of bbd_sgm_hints minus `stream`.
#include <cstdint>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_sgm_math.h"

extern "C" int hp_sgm_hints(const float* left, const float* right, const int32_t* side, int16_t* disp16,
                            int64_t* valid_count, void* scratch, long scratch_bytes, int B, int H, int W, int D,
                            int paths, int p1, int p2, int uniqueness, int fill) {
  const int rc = bbd_sgm_status(left, right, side, disp16, valid_count, scratch, scratch_bytes, B, H, W, D, paths, p1, p2,
                                uniqueness, fill);
  if (rc) return rc;
  BbdSgmScratch s;
  bbd_sgm_carve(scratch, B, H, W, D, &s);
  const size_t plane = (size_t)H * W;
  // grey and census of both images, in matching coordinates
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 2; ++i) {
      const float* img = (i ? right : left) + (size_t)b * 3 * plane;
      uint8_t* grey = s.grey + ((size_t)b * 2 + i) * plane;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const float* px = img + (size_t)y * W + bbd_sgm_column(x, W, side[b] != 0);
          grey[(size_t)y * W + x] = (uint8_t)bbd_sgm_luma(px[0], px[plane], px[2 * plane]);
        }
      uint64_t* census = s.census + ((size_t)b * 2 + i) * plane;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) census[(size_t)y * W + x] = bbd_sgm_census(grey, H, W, x, y);
    }
  // cost volume
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < H; ++y) {
      const uint64_t* cl = s.census + ((size_t)b * 2 * H + y) * W;
      const uint64_t* cr = cl + plane;
      for (int x = 0; x < W; ++x)
        for (int d = 0; d < D; ++d) s.cost[(((size_t)b * H + y) * W + x) * D + d] = (uint8_t)bbd_sgm_cost(cl, cr, x, d);
    }
  // paths: one line at a time, the previous pixel's L_r in `prev`
  std::vector<int> prev(D), cur(D);
  for (int r = 0; r < paths; ++r) {
    int dx, dy;
    bbd_sgm_direction(r, &dx, &dy);
    const int lines = bbd_sgm_lines(dy, H, W), steps = bbd_sgm_steps(dy, H, W);
    for (int b = 0; b < B; ++b)
      for (int line = 0; line < lines; ++line) {
        int m = 0;
        for (int t = 0; t < steps; ++t) {
          int x, y;
          const int start = bbd_sgm_line_pixel(dx, dy, H, W, line, t, &x, &y);
          const size_t at = (((size_t)b * H + y) * W + x) * D;
          for (int d = 0; d < D; ++d)
            cur[d] = start ? s.cost[at + d]
                           : bbd_sgm_step(s.cost[at + d], prev[d], d > 0 ? prev[d - 1] : 0, d + 1 < D ? prev[d + 1] : 0,
                                          d > 0, d + 1 < D, m, p1, p2);
          m = cur[0];
          for (int d = 0; d < D; ++d) {
            if (cur[d] < m) m = cur[d];
            s.S[at + d] = (uint16_t)((r ? s.S[at + d] : 0) + cur[d]);
          }
          prev.swap(cur);
        }
      }
  }
  // selection
  for (size_t p = 0; p < (size_t)B * plane; ++p) {
    const int x = (int)(p % W);
    const uint16_t* sp = s.S + p * D;
    uint32_t kl = 0xffffffffu, kr = 0xffffffffu;
    for (int d = 0; d < D; ++d) {
      const uint32_t k = bbd_sgm_key(sp[d], d);
      if (k < kl) kl = k;
      if (x + d < W) {
        const uint32_t q = bbd_sgm_key(s.S[(p + d) * D + d], d);
        if (q < kr) kr = q;
      }
    }
    const int best_s = (int)(kl >> 8), best_d = (int)(kl & 255u);
    int rival = 0;
    for (int d = 0; d < D; ++d) rival |= bbd_sgm_rivals(sp[d], d, best_s, best_d, uniqueness);
    s.sel[p] = bbd_sgm_sel(best_d, (int)(kr & 255u), rival);
  }
  // validity, sub-pixel value, store (mirrored back), count, fill
  for (int b = 0; b < B; ++b) {
    const int mirrored = side[b] != 0;
    int64_t count = 0;
    for (int y = 0; y < H; ++y) {
      const size_t row = ((size_t)b * H + y) * W;
      for (int x = 0; x < W; ++x) {
        const int valid = bbd_sgm_valid(s.sel + row, x);
        count += valid;
        disp16[row + bbd_sgm_column(x, W, mirrored)] =
            (int16_t)(valid ? bbd_sgm_disp16(s.S + (row + x) * D, (int)(s.sel[row + x] & 255u), D) : BBD_SGM_INVALID);
      }
      if (fill) {
        int carry = BBD_SGM_INVALID, first_x = W;
        for (int x = 0; x < W; ++x) {
          int16_t* v = disp16 + row + bbd_sgm_column(x, W, mirrored);
          if (*v != BBD_SGM_INVALID) {
            if (first_x == W) first_x = x;
            carry = *v;
          } else if (carry != BBD_SGM_INVALID) {
            *v = (int16_t)carry;
          }
        }
        if (first_x < W)
          for (int x = 0; x < first_x; ++x)
            disp16[row + bbd_sgm_column(x, W, mirrored)] = disp16[row + bbd_sgm_column(first_x, W, mirrored)];
      }
    }
    valid_count[b] = count;
  }
  return 0;
}
