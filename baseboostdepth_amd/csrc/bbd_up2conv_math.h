// bbd_up2conv_math.h - the index arithmetic of the sub-pixel form of "nearest x2 up-sample + ReflectionPad2d(1) + 3x3
// convolution" (bbd_up2conv.hip), shared with the host program that walks every address of a launch
// (tests/sanitize/up2conv_index_main.cpp).  No arithmetic on data here.
//
// With up[Y][X] = y[Y >> 1][X >> 1] and xp = ReflectionPad2d(1)(up), output pixel (2i + a, 2j + b) of the 3x3 convolution
// reads tap r at source row i + floor((a + r - 1) / 2): offsets -1, 0, 0 for a = 0 and 0, 0, 1 for a = 1; columns alike.
// The reflection border of `up` is a clamp on the source: xp[-1] = up[1] = y[0], xp[2h] = up[2h - 2] = y[h - 1].
//
// FORWARD.  Taps that fall on one source pixel add their weights (in double, rounded once), so each output parity (a, b)
// is a 2x2 convolution of the source: tap (dy, dx) stands at source offset (a - 1 + dy, b - 1 + dx) and carries the
// kernel rows bbd_up2conv_taps(a, dy) and the kernel columns bbd_up2conv_taps(b, dx).  A workgroup of BBD_UP2CONV_WAVES
// waves takes a TILE of BBD_UP2CONV_TR x BBD_UP2CONV_TC source pixels of one image: ELU(z + bias) of the tile and its
// 1-pixel clamped halo goes to LDS once ([16 channels][TR + 2][TC + 2], channel stride BBD_UP2CONV_CSTRIDE words so that
// the four 16-lane groups of a ds_read hit distinct banks); wave v owns the tile rows 2v, 2v + 1 and, per row, the
// STRIPS of 16 source pixels.  v_mfma_f32_16x16x4_f32 contracts 4 input channels: A = weights [k = lane & 15][c = 4q +
// (lane >> 4)], B = data [c][pixel = lane & 15], D [k = 4 (lane >> 4) + reg][pixel]; a lane writes its two column
// parities as one 8-byte store, 16 lanes a 128-byte row segment of `out`.
//
// BACKWARD (data).  grad_y[c][i][j] gathers the output rows Y = 2i - 1 + u, u = 0..3, with the kernel rows
// bbd_up2conv_bwd_taps(u) (w2 | w1 + w2 | w0 + w1 | w0); the clamp adds kernel row 0 to u = 1 where i = 0 and kernel row 2
// to u = 2 where i = h - 1 - the same for the whole strip, so those are extra MFMAs with weights the lane already holds.
// Along a row the border differs from lane to lane, so there the DATA are summed, per kernel column s:
//   s = 0: g[2j + 1] + g[2j + 2] (+ g[0] where j = 0);  s = 1: g[2j] + g[2j + 1];  s = 2: g[2j - 1] + g[2j] (+ g[2w - 1]
//   where j = w - 1), elements outside the row counting as zero.  A lane fetches the four floats g[2j - 1 .. 2j + 2].
// Workgroup `group` = one source row (n, i); its waves take the strips wave, wave + WAVES, ...  grad_bias: per-lane
// doubles over the wave's strips, 16 lanes, then the waves in order -> scratch[c * groups + group]; a second launch adds
// the groups of a channel in a fixed order.
#ifndef BBD_UP2CONV_MATH_H
#define BBD_UP2CONV_MATH_H

#ifdef __HIPCC__
#define BBD_U2_HD __host__ __device__ inline
#else
#define BBD_U2_HD inline
#endif

#define BBD_UP2CONV_CH 16          /* input and output channels the kernels take */
#define BBD_UP2CONV_WAVES 4        /* waves of a workgroup, both kernels */
#define BBD_UP2CONV_TR 8           /* source rows of a forward tile */
#define BBD_UP2CONV_TC 32          /* source columns of a forward tile */
#define BBD_UP2CONV_STRIP 16       /* source pixels of a strip: the N side of one MFMA */
#define BBD_UP2CONV_PITCH (BBD_UP2CONV_TC + 2)
#define BBD_UP2CONV_CSTRIDE 400    /* >= (TR + 2) * PITCH = 340 and = 16 mod 64 */
#define BBD_UP2CONV_LDS_WORDS (BBD_UP2CONV_CH * BBD_UP2CONV_CSTRIDE)
#define BBD_UP2CONV_FINAL_THREADS 64

struct bbd_up2conv_plan {
  int N, h, w;
  int tiles_x, tiles_y, blocks;   // forward: blocks = N * tiles_y * tiles_x
  int strips;                     // strips of a source row
  int groups;                     // backward: workgroups = N * h = bias partials per channel
};

// 0 = not taken.  C = K = 16; N, h, w >= 1; `out` below 2^31 elements.
BBD_U2_HD int bbd_up2conv_make_plan(int N, int C, int K, int h, int w, bbd_up2conv_plan* p) {
  if (N < 1 || h < 1 || w < 1 || C != BBD_UP2CONV_CH || K != BBD_UP2CONV_CH) return 0;
  if ((long)N * BBD_UP2CONV_CH * 4 * h * w > 0x7fffffffL) return 0;
  p->N = N; p->h = h; p->w = w;
  p->tiles_x = (w + BBD_UP2CONV_TC - 1) / BBD_UP2CONV_TC;
  p->tiles_y = (h + BBD_UP2CONV_TR - 1) / BBD_UP2CONV_TR;
  p->blocks = N * p->tiles_y * p->tiles_x;
  p->strips = (w + BBD_UP2CONV_STRIP - 1) / BBD_UP2CONV_STRIP;
  p->groups = N * h;
  return 1;
}

BBD_U2_HD int bbd_up2conv_plan_scratch_doubles(const bbd_up2conv_plan* p) { return BBD_UP2CONV_CH * p->groups; }

BBD_U2_HD int bbd_up2conv_clamp(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

// Workgroups are dealt round-robin over the chip's 8 L2 domains (b and b + 8 share one), so launch index b takes work
// item x * (total / 8) + min(x, total % 8) + b / 8 with x = b % 8: a domain gets one contiguous run of items, and the
// rows and columns that neighbouring items both read stay in one L2.  A permutation of [0, total); for speed only.
#define BBD_UP2CONV_DOMAINS 8
BBD_U2_HD int bbd_up2conv_spread(int b, int total) {
  const int base = total / BBD_UP2CONV_DOMAINS, rem = total % BBD_UP2CONV_DOMAINS, x = b % BBD_UP2CONV_DOMAINS;
  return x * base + (x < rem ? x : rem) + b / BBD_UP2CONV_DOMAINS;
}

// ---- the parity -> offset table -------------------------------------------------------------------------------------
// source offset of tap d (0 or 1) of output parity a (0 or 1)
BBD_U2_HD int bbd_up2conv_tap_offset(int a, int d) { return a - 1 + d; }
// kernel rows (columns) that tap d of parity a carries, as a bit mask over r = 0, 1, 2
BBD_U2_HD int bbd_up2conv_taps(int a, int d) { return a == 0 ? (d == 0 ? 1 : 6) : (d == 0 ? 3 : 4); }
// backward: kernel rows that output row 2i - 1 + u hands to source row i, borders aside
BBD_U2_HD int bbd_up2conv_bwd_taps(int u) { return u == 0 ? 4 : u == 1 ? 6 : u == 2 ? 3 : 1; }

// ---- forward --------------------------------------------------------------------------------------------------------
struct bbd_up2conv_tile { int n, i0, j0; };
BBD_U2_HD bbd_up2conv_tile bbd_up2conv_decode(const bbd_up2conv_plan* p, int block) {
  bbd_up2conv_tile t;
  const int item = bbd_up2conv_spread(block, p->blocks);
  const int tx = item % p->tiles_x, rest = item / p->tiles_x;
  t.j0 = tx * BBD_UP2CONV_TC;
  t.i0 = (rest % p->tiles_y) * BBD_UP2CONV_TR;
  t.n = rest / p->tiles_y;
  return t;
}
// element e of the LDS tile, 0 <= e < CH * (TR + 2) * PITCH: its channel, tile row and tile column ...
BBD_U2_HD void bbd_up2conv_fill_decode(int e, int* c, int* lr, int* lc) {
  const int plane = (BBD_UP2CONV_TR + 2) * BBD_UP2CONV_PITCH;
  *c = e / plane;
  const int rem = e - *c * plane;
  *lr = rem / BBD_UP2CONV_PITCH;
  *lc = rem - *lr * BBD_UP2CONV_PITCH;
}
// ... the word of LDS it goes to, and the element of z it comes from (tile row lr is source row i0 - 1 + lr, clamped)
BBD_U2_HD int bbd_up2conv_lds_index(int c, int lr, int lc) { return c * BBD_UP2CONV_CSTRIDE + lr * BBD_UP2CONV_PITCH + lc; }
BBD_U2_HD long bbd_up2conv_src_offset(const bbd_up2conv_plan* p, int n, int c, int i, int j) {
  return (((long)n * BBD_UP2CONV_CH + c) * p->h + i) * p->w + j;
}
BBD_U2_HD long bbd_up2conv_fill_src(const bbd_up2conv_plan* p, const bbd_up2conv_tile* t, int c, int lr, int lc) {
  return bbd_up2conv_src_offset(p, t->n, c, bbd_up2conv_clamp(t->i0 - 1 + lr, p->h), bbd_up2conv_clamp(t->j0 - 1 + lc, p->w));
}
// B operand of MFMA q (0..3) for lane `lane`: channel 4q + (lane >> 4) at tile row lr, tile column lc0 + (lane & 15)
BBD_U2_HD int bbd_up2conv_b_index(int q, int lane, int lr, int lc0) {
  return bbd_up2conv_lds_index(4 * q + (lane >> 4), lr, lc0 + (lane & 15));
}
// out[n][k][Y][X], [N, 16, 2h, 2w]; a lane stores X = 2j and 2j + 1 together
BBD_U2_HD long bbd_up2conv_out_offset(const bbd_up2conv_plan* p, int n, int k, int Y, int X) {
  return (((long)n * BBD_UP2CONV_CH + k) * (2 * p->h) + Y) * (2 * p->w) + X;
}

// ---- backward -------------------------------------------------------------------------------------------------------
// launch index `block` -> the group it takes (the index of its partials in scratch) and the group's source row (n, i)
BBD_U2_HD int bbd_up2conv_group(const bbd_up2conv_plan* p, int block, int* n, int* i) {
  const int group = bbd_up2conv_spread(block, p->groups);
  *n = group / p->h;
  *i = group - *n * p->h;
  return group;
}
// the lane's four floats of grad_out row Y: columns 2j - 1 + t, t = 0..3; bbd_up2conv_g_live says which exist
BBD_U2_HD long bbd_up2conv_g_offset(const bbd_up2conv_plan* p, int n, int k, int Y, int j) {
  return bbd_up2conv_out_offset(p, n, k, Y, 2 * j - 1);
}
BBD_U2_HD int bbd_up2conv_g_live(const bbd_up2conv_plan* p, int j, int t) {
  const int X = 2 * j - 1 + t;
  return j < p->w && X >= 0 && X < 2 * p->w;
}
BBD_U2_HD int bbd_up2conv_row_live(const bbd_up2conv_plan* p, int i, int u) {
  const int Y = 2 * i - 1 + u;
  return Y >= 0 && Y < 2 * p->h;
}
BBD_U2_HD long bbd_up2conv_scratch_index(const bbd_up2conv_plan* p, int c, int group) { return (long)c * p->groups + group; }

#endif  // BBD_UP2CONV_MATH_H
