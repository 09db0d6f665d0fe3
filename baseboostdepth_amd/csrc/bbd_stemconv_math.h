// bbd_stemconv_math.h - the index arithmetic of the encoder stems' 7x7, stride-2, pad-3 convolution and of its weight
// gradient (bbd_stemconv.hip), shared with the host program that walks every offset of both launches
// (tests/sanitize/stemconv_index_main.cpp).  No arithmetic on data here: which workgroup, wave and lane touches which
// element of x, w, out, grad_out, the LDS tile, scratch and grad_w, and nothing else.
//
//   out[n][k][oy][ox] = sum over (c, r, s) of w[k][c][r][s] * x[n][c][2 oy + r - 3][2 ox + s - 3]        (0 outside x)
//
// A TILE is BBD_STEM_TH x BBD_STEM_TW output pixels of one image; tile id = (n * tiles_y + ty) * tiles_x + tx.  It needs
// BBD_STEM_ROWS x (2 TW + 5) input pixels per channel, staged in LDS with the zero border written out.  A staged row
// holds its even local columns in one plane and its odd ones in another (BBD_STEM_PW words each): the 16 neighbouring
// output pixels a wave reads for one tap are then 16 neighbouring words.  Local column lx = 2 oxl + s of output column
// oxl and tap s is word oxl + (s >> 1) of plane s & 1.
//
// Forward: wave kb of the 4 waves of a workgroup owns the output channels [16 kb, 16 kb + 16) and keeps their weights
// in registers.  One v_mfma_f32_16x16x4_f32 takes, for one (c, r) and one parity of s, the 4 taps s = parity + 2 q,
// q = lane >> 4 (s = 7 has weight zero): A = weights of lane (channel lane & 15, tap q), B = the word of pixel lane & 15
// at plane position pixel + q - one LDS read whose lane part, (lane & 15) + (lane >> 4), is the same for every tap.
//
// Weight gradient: the reduction runs over pixels.  A = grad_out (channel lane & 15 of block kb, pixel 4 (lane >> 4) + j
// of a strip of 16), B = the patch column (c, r, s) = 16 ct + (lane & 15) at that pixel.  Wave w of 8 owns channel block
// w & 3 and the column tiles [(w >> 2) nct, (w >> 2) nct + nct): no two waves share an element.  A workgroup walks
// `per` neighbouring tiles; a fp32 accumulator takes BBD_STEM_RUN_STRIPS * 16 = BBD_WGRAD_RUN products and is then
// added to the lane's own double.  The workgroup's doubles are record `group` of scratch; a second launch adds the
// records in a fixed order.
#ifndef BBD_STEMCONV_MATH_H
#define BBD_STEMCONV_MATH_H

#ifdef __HIPCC__
#define BBD_ST_HD __host__ __device__ inline
#else
#define BBD_ST_HD inline
#endif

#define BBD_STEM_K 64                              /* output channels */
#define BBD_STEM_TH 8                              /* tile, output rows ... */
#define BBD_STEM_TW 32                             /* ... and columns */
#define BBD_STEM_ROWS (2 * BBD_STEM_TH + 5)        /* input rows of a tile */
#define BBD_STEM_PW 36                             /* words of one parity plane of a staged row (>= TW + 3) */
#define BBD_STEM_PITCH (2 * BBD_STEM_PW)           /* words of a staged row = local columns that are staged */
#define BBD_STEM_FWD_WAVES 4
#define BBD_STEM_WGRAD_WAVES 8
#define BBD_STEM_WGRAD_GROUPS 256                  /* most workgroups of the weight gradient's first launch */
#define BBD_STEM_STRIPS (BBD_STEM_TH * BBD_STEM_TW / 16)   /* strips of 16 pixels in a tile */
#define BBD_STEM_RUN_STRIPS 8                      /* strips per fp32 run: 128 products */
#define BBD_STEM_FINAL_E 16                        /* record elements of one workgroup of the final launch ... */
#define BBD_STEM_FINAL_G 16                        /* ... and the slices its groups are dealt into */

struct bbd_stem_plan {
  int N, C, H, W, Ho, Wo;
  int tiles_x, tiles_y, tiles;   // tiles = N * tiles_y * tiles_x
  int cols;                      // C * 49: columns of the weight gradient's GEMM
  int ctiles;                    // ceil(cols / 16)
  int nct;                       // column tiles per wave: ceil(ctiles / 2)
  int groups, per;               // weight gradient: workgroups, tiles per workgroup
  int record;                    // doubles of one workgroup's record: 8 * nct * 256
};

BBD_ST_HD int bbd_stem_lds_words(int C) { return C * BBD_STEM_ROWS * BBD_STEM_PITCH; }

// 0 = not taken.  K = 64, C 3 or 6, a 7 x 7 kernel, every tensor and the scratch below 2^31 elements.
BBD_ST_HD int bbd_stem_make_plan(int N, int C, int K, int H, int W, int R, int S, bbd_stem_plan* p) {
  if (N < 1 || H < 1 || W < 1 || K != BBD_STEM_K || (C != 3 && C != 6) || R != 7 || S != 7) return 0;
  const long limit = 0x7fffffffL;
  if ((long)N * K > limit || (long)N * C * H > limit || (long)N * C * H * W > limit) return 0;   // (each a value below 2^31
  const int Ho = (int)(((long)H + 1) / 2), Wo = (int)(((long)W + 1) / 2);        // times an int: no overflow of long)
  if ((long)N * K * Ho > limit || (long)N * K * Ho * Wo > limit) return 0;
  p->N = N; p->C = C; p->H = H; p->W = W; p->Ho = Ho; p->Wo = Wo;
  p->tiles_x = (Wo + BBD_STEM_TW - 1) / BBD_STEM_TW;
  p->tiles_y = (Ho + BBD_STEM_TH - 1) / BBD_STEM_TH;
  p->tiles = N * p->tiles_y * p->tiles_x;          // no more than out has elements
  p->cols = C * 49;
  p->ctiles = (p->cols + 15) / 16;
  p->nct = (p->ctiles + 1) / 2;
  const int most = p->tiles < BBD_STEM_WGRAD_GROUPS ? p->tiles : BBD_STEM_WGRAD_GROUPS;
  p->per = (p->tiles + most - 1) / most;
  p->groups = (p->tiles + p->per - 1) / p->per;
  p->record = BBD_STEM_WGRAD_WAVES * p->nct * 256;
  return 1;
}

BBD_ST_HD int bbd_stem_plan_scratch_doubles(const bbd_stem_plan* p) { return p->groups * p->record; }

struct bbd_stem_tile { int n, oy0, ox0; };

BBD_ST_HD bbd_stem_tile bbd_stem_decode(const bbd_stem_plan* p, int tile) {
  bbd_stem_tile t;
  const int row = tile / p->tiles_x;
  t.ox0 = (tile - row * p->tiles_x) * BBD_STEM_TW;
  t.n = row / p->tiles_y;
  t.oy0 = (row - t.n * p->tiles_y) * BBD_STEM_TH;
  return t;
}

// ---- staging: element e of [C][ROWS][PITCH local columns] -> LDS word and the element of x it shows (-1: zero border)
BBD_ST_HD void bbd_stem_fill_decode(int e, int* c, int* ly, int* lx) {
  *c = e / (BBD_STEM_ROWS * BBD_STEM_PITCH);
  const int rem = e - *c * (BBD_STEM_ROWS * BBD_STEM_PITCH);
  *ly = rem / BBD_STEM_PITCH;
  *lx = rem - *ly * BBD_STEM_PITCH;
}
BBD_ST_HD int bbd_stem_lds_index(int c, int ly, int lx) {
  return (c * BBD_STEM_ROWS + ly) * BBD_STEM_PITCH + (lx & 1) * BBD_STEM_PW + (lx >> 1);
}
BBD_ST_HD long bbd_stem_fill_src(const bbd_stem_plan* p, const bbd_stem_tile* t, int c, int ly, int lx) {
  const int iy = 2 * t->oy0 - 3 + ly, ix = 2 * t->ox0 - 3 + lx;
  if (iy < 0 || iy >= p->H || ix < 0 || ix >= p->W) return -1;
  return (((long)t->n * p->C + c) * p->H + iy) * p->W + ix;
}

// ---- forward
// the weight lane `lane` of wave kb holds for the MFMA (c, r, parity): -1 where the tap is s = 7 (zero)
BBD_ST_HD int bbd_stem_fwd_w_index(int C, int kb, int lane, int c, int r, int parity) {
  const int s = parity + 2 * (lane >> 4);
  if (s > 6) return -1;
  return (((kb * 16 + (lane & 15)) * C + c) * 7 + r) * 7 + s;
}
// the lane's part of every B read, and the part of MFMA (c, r, parity) for output row oyl, pixel group pg of the tile
BBD_ST_HD int bbd_stem_fwd_b_lane(int lane) { return (lane & 15) + (lane >> 4); }
BBD_ST_HD int bbd_stem_fwd_b_tap(int c, int r, int parity, int oyl, int pg) {
  return (c * BBD_STEM_ROWS + 2 * oyl + r) * BBD_STEM_PITCH + parity * BBD_STEM_PW + pg * 16;
}
BBD_ST_HD long bbd_stem_out_offset(const bbd_stem_plan* p, int n, int k, int oy, int ox) {
  return (((long)n * BBD_STEM_K + k) * p->Ho + oy) * p->Wo + ox;
}

// ---- weight gradient
BBD_ST_HD void bbd_stem_group_range(const bbd_stem_plan* p, int group, int* first, int* last) {
  const long a = (long)group * p->per, b = a + p->per;
  *first = (int)(a > p->tiles ? p->tiles : a);
  *last = (int)(b > p->tiles ? p->tiles : b);
}
// column tile ct (0 .. nct) of wave `wave`: the global tile, and is it one of the ctiles that exist?
BBD_ST_HD int bbd_stem_wave_ctile(const bbd_stem_plan* p, int wave, int ct) { return (wave >> 2) * p->nct + ct; }
// the lane's part of the B reads of column tile `ctile`: LDS word of (c, r, s) at output pixel (0, 4 (lane >> 4)) of the
// tile; a column past the last one reads word 0 + the pixel part (its results are never used)
BBD_ST_HD int bbd_stem_wgrad_b_lane(const bbd_stem_plan* p, int ctile, int lane) {
  const int col = ctile * 16 + (lane & 15);
  int at = 0;
  if (col < p->cols) {
    const int c = col / 49, rs = col - c * 49, r = rs / 7, s = rs - r * 7;
    at = (c * BBD_STEM_ROWS + r) * BBD_STEM_PITCH + (s & 1) * BBD_STEM_PW + (s >> 1);
  }
  return at + 4 * (lane >> 4);
}
// ... and the strip's part: strip st of a tile = output row st / 2, pixel group st & 1; pixel j of the lane adds j
BBD_ST_HD int bbd_stem_strip_row(int st) { return st / (BBD_STEM_TW / 16); }
BBD_ST_HD int bbd_stem_strip_pg(int st) { return st % (BBD_STEM_TW / 16); }
BBD_ST_HD int bbd_stem_wgrad_b_strip(int st) {
  return 2 * bbd_stem_strip_row(st) * BBD_STEM_PITCH + bbd_stem_strip_pg(st) * 16;
}
// grad_out: the lane's first pixel of a strip, how many of its 4 pixels exist, and the offset of the first
BBD_ST_HD int bbd_stem_go_pixels(const bbd_stem_plan* p, const bbd_stem_tile* t, int st, int lane) {
  if (t->oy0 + bbd_stem_strip_row(st) >= p->Ho) return 0;
  const int left = p->Wo - (t->ox0 + bbd_stem_strip_pg(st) * 16 + 4 * (lane >> 4));
  return left < 0 ? 0 : left > 4 ? 4 : left;
}
BBD_ST_HD long bbd_stem_go_offset(const bbd_stem_plan* p, const bbd_stem_tile* t, int st, int kb, int lane) {
  return bbd_stem_out_offset(p, t->n, kb * 16 + (lane & 15), t->oy0 + bbd_stem_strip_row(st),
                             t->ox0 + bbd_stem_strip_pg(st) * 16 + 4 * (lane >> 4));
}
// record element of accumulator register reg of lane `lane`, column tile ct of wave `wave`, and where it goes in grad_w
// [64, C, 7, 7] (-1: a padded column)
BBD_ST_HD int bbd_stem_record_index(const bbd_stem_plan* p, int wave, int ct, int lane, int reg) {
  return ((wave * p->nct + ct) * 64 + lane) * 4 + reg;
}
BBD_ST_HD int bbd_stem_record_to_weight(const bbd_stem_plan* p, int e) {
  const int reg = e & 3, lane = (e >> 2) & 63, t = e >> 8;
  const int wave = t / p->nct, ct = t - wave * p->nct;
  const int k = (wave & 3) * 16 + 4 * (lane >> 4) + reg, col = bbd_stem_wave_ctile(p, wave, ct) * 16 + (lane & 15);
  return col < p->cols ? k * p->cols + col : -1;
}
BBD_ST_HD long bbd_stem_record_offset(const bbd_stem_plan* p, int group) { return (long)group * p->record; }

#endif  // BBD_STEMCONV_MATH_H
