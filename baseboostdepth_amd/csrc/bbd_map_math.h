/* bbd_map_math.h - everything of the bbd_map_* entries that is not launch geometry or an atomic, shared by bbd_map.hip
 * and its host port (tests/host_port/bbd_map_port.cpp): the argument rules, the candidate grid, what a candidate pixel
 * becomes (a voxel key, three 16-bit offsets inside the voxel, three colour bytes), the hash, and the vertex of a
 * finished voxel.  Compiled with -ffp-contract=off: every product, sum and quotient below is one IEEE operation,
 * rounded where it is written; `float` lines are float32, `double` lines float64.
 *
 *   candidate g of a call (frame-major, raster order inside a frame):  i = g / cap, c = g % cap, cap = ncy * ncx,
 *             cy = c / ncx, cx = c % ncx, y = r0 + cy * stride, x = c0 + cx * stride, k = y * w + x
 *             (the window is cut to the image first; ncy = ceil((r1 - r0) / stride), ncx = ceil((c1 - c0) / stride))
 *   1 depth   d = 1.0f / disp[i][k]                    float32 (BBD_MAP_INPUT_IS_DEPTH: d = disp[i][k])
 *   2 ray     x = bbd_syns_backproject(inv_K, k, h, w, pixel rays, d)          float32 (bbd_syns_math.h)
 *   3 keep    dm = scale * (double)d;  kept when dm is finite and min_depth <= dm <= max_depth, else REJECTED
 *   4 world   s_j = scale * (double)x_j;  X_r = ((P[4r] * s_0 + P[4r+1] * s_1) + P[4r+2] * s_2) + P[4r+3], r = 0, 1, 2
 *             with P = poses[i], row-major 4x4 camera-to-world
 *   5 voxel   u = X / voxel;  v = floor(u);  q = (uint32)((u - v) * 65536.0)       per axis (u - v is exact; it is 1.0
 *             for a negative u smaller than half an ulp of 1, q is then 65536: the sums hold it)
 *   6 range   a point with a non-finite X or |v| >= 2^20 on any axis is OUT OF RANGE
 *   7 key     ((v_x + 2^20) << 42) | ((v_y + 2^20) << 21) | (v_z + 2^20): 63 bits, never the empty key (all ones)
 *   8 colour  t = c * 255.0f + 0.5f;  byte = 0 unless t > 0, 255 where t >= 255, else (int)t
 *             - min(max((int)t, 0), 255) wherever that conversion is defined
 *   hash      splitmix64's finaliser: z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb;
 *             z ^= z >> 31; first slot = z & (T - 1), then linear probing
 *   vertex    n = count;  axis: (float)(((double)v + ((double)sum_q / (double)n + 0.5) / 65536.0) * voxel)
 *             channel: (sum + n / 2) / n in integers; {bits(x), bits(y), bits(z), r | g << 8 | b << 16 | 255 << 24}
 */
#ifndef BBD_MAP_MATH_H
#define BBD_MAP_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_cloud_math.h" /* bbd_cloud_float_bits; brings bbd_syns_math.h (bbd_syns_backproject) */

#define BBD_MAP_EMPTY 0xffffffffffffffffull
#define BBD_MAP_HALF 1048576 /* 2^20: voxel indices lie in (-2^20, 2^20) */
#define BBD_MAP_CHUNK 256 /* slots per chunk of the compaction: one workgroup of four waves */

/* bbd_map_point's verdicts */
#define BBD_MAP_REJECTED 0
#define BBD_MAP_KEPT 1
#define BBD_MAP_OUT_OF_RANGE 2

/* What the per-candidate function reads; the same struct travels to the kernel by value. */
struct BbdMapParams {
  const float* disp;    /* [n,h,w] */
  const float* rgb;     /* [n,3,h,w] */
  const double* poses;  /* [n,16] */
  const float* inv_K;   /* [3,3] */
  const double* scale;  /* one double, or NULL = 1 */
  int n, h, w, r0, c0, ncy, ncx, stride, flags;
  double lo, hi, voxel;
};

struct BbdMapPoint {
  uint64_t key;
  uint32_t q[3];
  uint32_t rgb[3];
};

BBD_HD int bbd_map_pow2(int T) { return T >= 1 && (T & (T - 1)) == 0; }

/* Status of the state's arguments: 0, BBD_E_BADARG or BBD_E_TOOMANY. */
BBD_HD int bbd_map_state_status(const void* keys, const void* pos, const void* col, int T) {
  if (!keys || !pos || !col) return BBD_E_BADARG;
  if (T < 1) return BBD_E_BADARG;
  if (T > BBD_MAP_MAX_T) return BBD_E_TOOMANY;
  return bbd_map_pow2(T) ? 0 : BBD_E_BADARG;
}

BBD_HD int bbd_map_chunks(int T) { return (T + BBD_MAP_CHUNK - 1) / BBD_MAP_CHUNK; }

/* The candidate grid of a call's window, cut to the image. */
BBD_HD void bbd_map_grid(int h, int w, int r0, int r1, int c0, int c1, int stride, BbdMapParams* a) {
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > h ? h : r1;
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > w ? w : c1;
  a->r0 = r0;
  a->c0 = c0;
  a->ncy = r1 > r0 ? (r1 - r0 - 1) / stride + 1 : 0;
  a->ncx = c1 > c0 ? (c1 - c0 - 1) / stride + 1 : 0;
}

BBD_HD int bbd_map_finite(double v) { return v - v == 0.0; }

/* Status of bbd_map_accumulate's arguments beyond the state's. */
BBD_HD int bbd_map_accumulate_status(const void* counters, const void* disp, const void* rgb, const void* poses,
                                     const void* inv_K, int n, int h, int w, int stride, double min_depth,
                                     double max_depth, double voxel, int flags) {
  if (!counters || !disp || !rgb || !poses || !inv_K) return BBD_E_BADARG;
  if (n < 1 || h < 1 || w < 1 || stride < 1) return BBD_E_BADARG;
  if (!(voxel > 0.0) || !bbd_map_finite(voxel)) return BBD_E_BADARG;
  if (!(min_depth <= max_depth)) return BBD_E_BADARG; /* a NaN limit lands here */
  if (flags & ~(BBD_MAP_INPUT_IS_DEPTH | BBD_MAP_NO_MERGE)) return BBD_E_BADARG;
  if ((long)n * (long)h * (long)w > 0x7fffffffL) return BBD_E_TOOMANY;
  return 0;
}

BBD_HD uint64_t bbd_map_hash(uint64_t z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

BBD_HD uint32_t bbd_map_byte(float c) {
  const float t = c * 255.0f + 0.5f;
  if (!(t > 0.0f)) return 0u;
  return t >= 255.0f ? 255u : (uint32_t)(int)t;
}

/* Candidate c of frame i: steps 1 to 8 above.  `scale` is the value the call read once. */
BBD_HD int bbd_map_point(const BbdMapParams* a, double scale, int i, int c, BbdMapPoint* o) {
  const int cy = c / a->ncx, cx = c - cy * a->ncx;
  const int y = a->r0 + cy * a->stride, x = a->c0 + cx * a->stride;
  const int k = y * a->w + x;
  const size_t plane = (size_t)a->h * (size_t)a->w;
  const float raw = a->disp[(size_t)i * plane + (size_t)k];
  const float d = (a->flags & BBD_MAP_INPUT_IS_DEPTH) ? raw : 1.0f / raw;
  const double dm = scale * (double)d;
  if (!(bbd_map_finite(dm) && dm >= a->lo && dm <= a->hi)) return BBD_MAP_REJECTED;
  float p[3];
  bbd_syns_backproject(a->inv_K, k, a->h, a->w, 1, d, p);
  const double s0 = scale * (double)p[0], s1 = scale * (double)p[1], s2 = scale * (double)p[2];
  const double* P = a->poses + (size_t)i * 16;
  uint64_t key = 0;
  for (int r = 0; r < 3; ++r) {
    const double X = ((P[4 * r] * s0 + P[4 * r + 1] * s1) + P[4 * r + 2] * s2) + P[4 * r + 3];
    const double u = X / a->voxel;
    const double v = floor(u);
    if (!(fabs(v) < (double)BBD_MAP_HALF)) return BBD_MAP_OUT_OF_RANGE; /* NaN and the infinities land here too */
    o->q[r] = (uint32_t)((u - v) * 65536.0);
    key = (key << 21) | (uint64_t)((int64_t)v + BBD_MAP_HALF);
  }
  o->key = key;
  const float* col = a->rgb + (size_t)i * 3 * plane + (size_t)k;
  for (int ch = 0; ch < 3; ++ch) o->rgb[ch] = bbd_map_byte(col[(size_t)ch * plane]);
  return BBD_MAP_KEPT;
}

/* The vertex of a finished voxel: its key, the three offset sums, {sum r, sum g, sum b, count}. */
BBD_HD void bbd_map_vertex(uint64_t key, const uint64_t* sum_q, const uint32_t* col, double voxel, uint32_t out[4]) {
  const uint32_t n = col[3];
  for (int r = 0; r < 3; ++r) {
    const int64_t v = (int64_t)((key >> (21 * (2 - r))) & 0x1fffffu) - BBD_MAP_HALF;
    const double off = ((double)sum_q[r] / (double)n + 0.5) / 65536.0;
    out[r] = bbd_cloud_float_bits((float)(((double)v + off) * voxel));
  }
  const uint32_t h = n / 2u;
  const uint32_t r8 = (col[0] + h) / n, g8 = (col[1] + h) / n, b8 = (col[2] + h) / n;
  out[3] = r8 | (g8 << 8) | (b8 << 16) | 0xff000000u;
}

#endif /* BBD_MAP_MATH_H */
