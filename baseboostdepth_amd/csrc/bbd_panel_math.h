/* bbd_panel_math.h - per-pixel arithmetic of the training-log panel (bbd_panel.hip), shared with the host port of
 * the test tier (tests/host_port/bbd_panel_port.cpp).
 *
 *   COLOR   u8 = (int)(min(max(x, 0), 1) * 255 + 0.5)          round to nearest: k / 255.0f gives k back
 *   WARP    the fused forward's warp of one pixel (bbd_project, bbd_taps, bbd_fetch4, bbd_bilerp of bbd_math.h, called
 *           as warp_into_lds calls them for `warped_out`), quantised like COLOR
 *   SCALAR  lut[bbd_viz_lut_index(v, min, max)], min / max of the plane without its NaNs (order keys of bbd_viz_math.h)
 *   ARGMIN  palette[id] for a true-pose warp, palette[id - n_T] >> 1 for an error-induced one, black for an identity
 *
 * Colours travel as r | g << 8 | b << 16.  Compile with -ffp-contract=off. */
#ifndef BBD_PANEL_MATH_H
#define BBD_PANEL_MATH_H

#include <stdint.h>

#include "bbd_math.h"
#include "bbd_viz_math.h"

#define BBD_PANEL_PALETTE 20      /* entries of the categorical palette (= BBD_MAX_CAND) */

/* One channel in [0,1] -> 0..255.  A NaN takes 0 (both comparisons fail towards the bounds). */
BBD_HD uint32_t bbd_panel_quant(float x) {
  x = x > 0.0f ? x : 0.0f;
  x = x < 1.0f ? x : 1.0f;
  const float s = x * 255.0f;
  return (uint32_t)(int)(s + 0.5f);
}

BBD_HD uint32_t bbd_panel_pack(float r, float g, float b) {
  return bbd_panel_quant(r) | (bbd_panel_quant(g) << 8) | (bbd_panel_quant(b) << 16);
}

/* Pixel (x, y) of the planar image `src` [3, hw]. */
BBD_HD uint32_t bbd_panel_color(const float* src, size_t hw, size_t i) {
  return bbd_panel_pack(src[i], src[hw + i], src[2 * hw + i]);
}

/* Pixel (x, y) of `src` warped into the target view: pj = P (3x4) | inv_K[:3,:3] from bbd_make_proj.  The three floats
 * are the bits the fused forward writes to `warped_out`; they are returned through `val` for the callers that want them. */
BBD_HD uint32_t bbd_panel_warp(const float* src, const float* depth, const float* pj, const BbdDims& dm, int x, int y,
                               float val[3]) {
  const int hw = dm.H * dm.W;
  BbdSample sm;
  BbdTaps t;
  bbd_project(pj, x, y, depth[(size_t)y * dm.W + x], dm, &sm);
  bbd_taps(sm.ix, sm.iy, dm, &t);
  float v[3][4];
  for (int ch = 0; ch < 3; ++ch) bbd_fetch4(src + (size_t)ch * hw, &t, v[ch]);
  for (int ch = 0; ch < 3; ++ch) val[ch] = bbd_bilerp(v[ch], &t);
  return bbd_panel_pack(val[0], val[1], val[2]);
}

/* Running minimum / maximum of a plane as order keys; a NaN is skipped.  inv_min = ~key of the minimum, so that both
 * are maxima and 0 means "no value yet" (no float has the key 0 or 0xffffffff except NaNs). */
BBD_HD void bbd_panel_minmax_update(float v, uint32_t* inv_min, uint32_t* max_key) {
  if (v != v) return;
  const uint32_t k = bbd_viz_order_key(v);
  *inv_min = ~k > *inv_min ? ~k : *inv_min;
  *max_key = k > *max_key ? k : *max_key;
}
/* A plane without a value (all NaN) gives NaN for both, like numpy's nanmin / nanmax. */
BBD_HD void bbd_panel_minmax_values(uint32_t inv_min, uint32_t max_key, float* vmin, float* vmax) {
  *vmin = bbd_viz_key_value(~inv_min);
  *vmax = bbd_viz_key_value(max_key);
}

/* palette: BBD_PANEL_PALETTE packed colours. */
BBD_HD uint32_t bbd_panel_argmin_colour(const uint32_t* palette, int id, int n_t, int n_e) {
  if (id < n_t) return id < BBD_PANEL_PALETTE ? palette[id] : 0u;
  const int e = id - n_t;
  if (e < n_e && e < BBD_PANEL_PALETTE) return (palette[e] >> 1) & 0x7f7f7fu;
  return 0u;
}

#endif /* BBD_PANEL_MATH_H */
