// Host port of bbd_postproc.hip for the CPU test tier: the same per-pixel functions (bbd_postproc_math.h) in plain
// loops.  Same C signature as bbd_post_process_disp minus `stream`.
#include <cstddef>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_postproc_math.h"

extern "C" int hp_post_process_disp(const float* disp, float* out, int n, int h, int w) {
  if (!disp || !out || n < 1 || h < 1 || w < 1) return BBD_E_BADARG;
  const size_t rows = (size_t)n * (size_t)h;
  const float* flipped = disp + rows * (size_t)w;
  const double step = bbd_postproc_step(w);
  for (int x = 0; x < w; ++x) {
    const int xm = w - 1 - x;
    const double a = bbd_postproc_mask(x, w, step), b = bbd_postproc_mask(xm, w, step);
    for (size_t r = 0; r < rows; ++r) {
      const size_t base = r * (size_t)w;
      out[base + (size_t)x] = bbd_postproc_blend(disp[base + (size_t)x], flipped[base + (size_t)xm], a, b);
    }
  }
  return 0;
}
