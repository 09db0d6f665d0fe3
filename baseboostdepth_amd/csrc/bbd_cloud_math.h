/* bbd_cloud_math.h - everything of bbd_point_cloud that is not launch geometry, shared by bbd_cloud.hip and its host
 * port (tests/host_port/bbd_cloud_port.cpp): the argument rules, the candidate grid of an image, the depth of a
 * candidate and whether it is kept, and the 16-byte vertex.  Compiled with -ffp-contract=off: every product, sum and
 * quotient below is one IEEE float32 operation, rounded where it is written.
 *
 *   candidate c of image i (raster order):  cy = c / ncx, cx = c % ncx,  y = r0 + cy * stride, x = c0 + cx * stride,
 *                                           ncy = ceil((r1 - r0) / stride), ncx = ceil((c1 - c0) / stride)
 *   depth   d = bbd_eval_resample(pred[i], ..., y, x)         (bbd_eval_math.h)
 *           d = d * ratio                                     ratio = rows[i][7], only where rows is given
 *           BBD_CLOUD_FROM_GT: d = gt[y * GW + x] instead
 *   kept    BBD_CLOUD_MASK_GT: min_depth < gt < max_depth, else dropped
 *           d != d: dropped
 *           BBD_CLOUD_CLAMP:   d = d < min_depth ? min_depth : d;  d = d > max_depth ? max_depth : d;  kept
 *           otherwise:         kept when min_depth <= d <= max_depth (an infinity fails the comparison)
 *   xyz     bbd_syns_backproject(inv_K[i], y * GW + x, GH, GW, pixel_rays, d)          (bbd_syns_math.h)
 *   colour  the three bytes of rgb at the pixel, or lut[idx]:
 *           a = 1.0f / max_depth;  t = (1.0f / d - a) / (1.0f / min_depth - a);  u = t * 256.0f
 *           idx = 0 unless u > 0 (a NaN t, from min_depth == max_depth, lands here), 255 where u >= 255, else (int)u
 *           - min(max((int)(t * 256), 0), 255) wherever that conversion is defined
 *   vertex  {bits(x), bits(y), bits(z), r | g << 8 | b << 16 | 255 << 24}: four 32-bit words, stored as one
 */
#ifndef BBD_CLOUD_MATH_H
#define BBD_CLOUD_MATH_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bbd_hip.h"
#include "bbd_eval_math.h"
#include "bbd_ragged_math.h"
#include "bbd_syns_math.h"

#define BBD_CLOUD_CHUNK 256 /* candidates per chunk: one workgroup of four waves */
/* Pixels of the largest image a call takes: a candidate index rounded up to a whole chunk still fits an int. */
#define BBD_CLOUD_MAX_PIXELS (0x7fffffffL - BBD_CLOUD_CHUNK)
#define BBD_CLOUD_FLAGS \
  (BBD_EVAL_PRED_IS_DISP | BBD_CLOUD_FROM_GT | BBD_CLOUD_CLAMP | BBD_CLOUD_MASK_GT | BBD_CLOUD_RAYS_REFERENCE)

/* What the per-candidate functions read; the same struct travels to the kernels by value. */
struct BbdCloudParams {
  const float* pred;    /* [n,h,w] */
  const float* gt;      /* ragged, may be NULL */
  const int32_t* desc;  /* [n, BBD_CLOUD_DESC] */
  const float* rows;    /* [n, BBD_EVAL_OUT], may be NULL */
  const float* inv_K;   /* [n,3,3] */
  const uint8_t* rgb;   /* ragged at 3 * offset, may be NULL */
  const uint8_t* lut;   /* [256,3] */
  int h, w, max_h, max_w, stride, flags;
  float lo, hi, clamp_lo, clamp_hi, scale_factor;
};

/* One BBD_CLOUD_DESC row as the kernels use it.  The window is cut to the image; an image larger than max_h x max_w
 * (the sizes the launch and the scratch were made for) or without pixels has no candidates. */
struct BbdCloudImg {
  size_t off, out; /* element offset of the maps; first vertex of the region */
  int GH, GW, r0, c0, ncy, ncx, cap;
};

BBD_HD BbdCloudImg bbd_cloud_img(const int32_t* desc, int i, int stride, int max_h, int max_w) {
  const int32_t* d = desc + (size_t)i * BBD_CLOUD_DESC;
  const BbdEvalRow row = bbd_eval_row(d, 0);
  BbdCloudImg m;
  m.off = row.off;
  m.out = bbd_join64(d[8], d[9]);
  m.GH = row.GH;
  m.GW = row.GW;
  const int ok = m.GH >= 1 && m.GW >= 1 && m.GH <= max_h && m.GW <= max_w;
  const int r0 = row.r0 < 0 ? 0 : row.r0, r1 = row.r1 > m.GH ? m.GH : row.r1;
  const int c0 = row.c0 < 0 ? 0 : row.c0, c1 = row.c1 > m.GW ? m.GW : row.c1;
  m.r0 = r0;
  m.c0 = c0;
  m.ncy = ok && r1 > r0 ? (r1 - r0 - 1) / stride + 1 : 0;
  m.ncx = ok && c1 > c0 ? (c1 - c0 - 1) / stride + 1 : 0;
  m.cap = m.ncy * m.ncx; /* <= GH * GW <= max_h * max_w, at most BBD_CLOUD_MAX_PIXELS */
  return m;
}

/* Chunks of the largest candidate grid a max_h x max_w image can have: the per-image stride of the chunk table. */
BBD_HD long bbd_cloud_chunk_stride(int max_h, int max_w, int stride) {
  const long cand = (long)((max_h - 1) / stride + 1) * (long)((max_w - 1) / stride + 1);
  return (cand + BBD_CLOUD_CHUNK - 1) / BBD_CLOUD_CHUNK;
}

/* Status of a call's arguments: 0, BBD_E_BADARG or BBD_E_TOOMANY.  (The scratch size is checked next to it.) */
BBD_HD int bbd_cloud_args_status(const void* pred, const void* gt, const void* desc, const void* inv_K,
                                 const void* rgb, const void* lut, const void* vertices, const void* counts,
                                 const void* scratch, int n, int h, int w, int max_h, int max_w, int stride,
                                 int flags) {
  if (!pred || !desc || !inv_K || !vertices || !counts || !scratch || (!rgb && !lut)) return BBD_E_BADARG;
  if (n < 1 || h < 1 || w < 1 || max_h < 1 || max_w < 1 || stride < 1) return BBD_E_BADARG;
  if (flags & ~BBD_CLOUD_FLAGS) return BBD_E_BADARG;
  if ((flags & (BBD_CLOUD_FROM_GT | BBD_CLOUD_MASK_GT)) && !gt) return BBD_E_BADARG;
  if (((uintptr_t)vertices & (BBD_CLOUD_VERTEX - 1)) != 0) return BBD_E_BADARG;
  if (n > 65535) return BBD_E_TOOMANY;
  if ((long)max_h * (long)max_w > BBD_CLOUD_MAX_PIXELS || (long)h * (long)w > 0x7fffffffL) return BBD_E_TOOMANY;
  if ((long)n * bbd_cloud_chunk_stride(max_h, max_w, stride) > 0x7fffffffL) return BBD_E_TOOMANY;
  return 0;
}

/* Depth of candidate c of image i; returns whether the candidate is kept.  *pixel = y * GW + x. */
BBD_HD int bbd_cloud_depth(const BbdCloudParams* a, const BbdCloudImg* m, int i, int c, int* pixel, float* depth) {
  const int cy = c / m->ncx, cx = c - cy * m->ncx;
  const int y = m->r0 + cy * a->stride, x = m->c0 + cx * a->stride;
  const int k = y * m->GW + x;
  *pixel = k;
  float g = 0.0f;
  if (a->flags & (BBD_CLOUD_FROM_GT | BBD_CLOUD_MASK_GT)) g = a->gt[m->off + (size_t)k];
  if ((a->flags & BBD_CLOUD_MASK_GT) && !(g > a->lo && g < a->hi)) return 0;
  float d;
  if (a->flags & BBD_CLOUD_FROM_GT) {
    d = g;
  } else {
    d = bbd_eval_resample(a->pred + (size_t)i * a->h * a->w, a->h, a->w, a->scale_factor, a->clamp_lo, a->clamp_hi,
                          a->flags & BBD_EVAL_PRED_IS_DISP, y, x, m->GH, m->GW);
    if (a->rows) d *= a->rows[(size_t)i * BBD_EVAL_OUT + 7];
  }
  if (d != d) return 0;
  if (a->flags & BBD_CLOUD_CLAMP) {
    d = d < a->lo ? a->lo : d;
    d = d > a->hi ? a->hi : d;
  } else if (!(d >= a->lo && d <= a->hi)) {
    return 0;
  }
  *depth = d;
  return 1;
}

BBD_HD int bbd_cloud_lut_index(float d, float lo, float hi) {
  const float a = 1.0f / hi;
  const float t = (1.0f / d - a) / (1.0f / lo - a);
  const float u = t * 256.0f;
  if (!(u > 0.0f)) return 0;
  return u >= 255.0f ? 255 : (int)u;
}

BBD_HD uint32_t bbd_cloud_float_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

/* The vertex of a kept candidate: pixel and depth as bbd_cloud_depth returned them. */
BBD_HD void bbd_cloud_vertex(const BbdCloudParams* a, const BbdCloudImg* m, int i, int pixel, float depth,
                             uint32_t v[4]) {
  float p[3];
  bbd_syns_backproject(a->inv_K + (size_t)i * 9, pixel, m->GH, m->GW, (a->flags & BBD_CLOUD_RAYS_REFERENCE) ? 0 : 1,
                       depth, p);
  const uint8_t* c = a->rgb ? a->rgb + 3 * (m->off + (size_t)pixel)
                            : a->lut + 3 * bbd_cloud_lut_index(depth, a->lo, a->hi);
  v[0] = bbd_cloud_float_bits(p[0]);
  v[1] = bbd_cloud_float_bits(p[1]);
  v[2] = bbd_cloud_float_bits(p[2]);
  v[3] = bbd_pack_rgb(c) | 0xff000000u;
}

#endif /* BBD_CLOUD_MATH_H */
