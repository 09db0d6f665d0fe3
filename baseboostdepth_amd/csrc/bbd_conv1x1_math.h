// bbd_conv1x1_math.h - the index arithmetic of the ResNet shortcut convolution (1x1, stride 2, no padding, no bias) in its
// three directions (bbd_conv1x1.hip), shared with the host program that walks every offset of every launch
// (tests/sanitize/conv1x1_index_main.cpp).  No arithmetic on data here: which workgroup, wave and lane touches which
// element of x, w, y, dy, dx, the LDS tile, scratch and dw, and nothing else.
//
//   y[n][k][oy][ox] = sum over c of w[k][c] * x[n][c][2 oy][2 ox]          Ho = (H + 1) / 2, Wo = (W + 1) / 2, P = Ho * Wo
//
// Output pixels are numbered FLAT over the batch, g = n * P + oy * Wo + ox, and every launch cuts that one range: a TILE
// is BBD_C1_TP neighbouring g (forward, data gradient), a STRIP 16 of them (weight gradient).  Neither assumes that P is
// a multiple of anything: a tile or a strip may cross from one sample into the next and may end past the last pixel.
//
// Forward and data gradient are the same GEMM, out (M x pixels) = A (M x R) * B (R x pixels): the B operand (x at the
// even positions, or dy) of a tile sits in LDS, BBD_C1_RC rows of the reduction at a time, a row BBD_C1_PITCH words
// apart; wave `wave` of a workgroup owns the 16 output channels of block blockIdx.y * 4 + wave and four accumulator tiles
// of 16 pixels.  One v_mfma_f32_16x16x4_f32 contracts the reduction rows s + 4 q + j, q = lane >> 4: lane (q, i = lane &
// 15) reads word (s + 4 q + j) * PITCH + 16 pg + i, and PITCH = 4 mod 16 puts the four q on four bank groups.
//
// Weight gradient: dw (K x C) reduces over the pixels.  A workgroup owns a block of 64 x 64 of dw (wave: 32 x 32 of it,
// two blocks of 16 each way) and a range of strips; lane (q, i) holds channel i of its blocks at the strip's pixels
// 4 q + j.  A fp32 accumulator takes BBD_C1_RUN_STRIPS * 16 = BBD_WGRAD_RUN products and is then added to the lane's own
// double; the workgroup's doubles are record `split` of scratch, [K][C] each, and a second launch adds the records in a
// fixed order.  The number of records depends on K and C only.
#ifndef BBD_CONV1X1_MATH_H
#define BBD_CONV1X1_MATH_H

#ifdef __HIPCC__
#define BBD_C1_HD __host__ __device__ inline
#else
#define BBD_C1_HD inline
#endif

#define BBD_C1_TP 64                 /* flat output pixels of a tile */
#define BBD_C1_PITCH 68              /* words between two reduction rows of the LDS tile */
#define BBD_C1_RC 64                 /* reduction rows staged at a time */
#define BBD_C1_WAVES 4               /* waves of a workgroup: 64 output channels, or 64 x 64 of dw */
#define BBD_C1_WGRAD_GROUPS 512      /* workgroups the weight gradient's first launch aims at */
#define BBD_C1_RUN_STRIPS 8          /* strips per fp32 run: 128 products */
#define BBD_C1_FINAL_E 16            /* record elements of one workgroup of the final launch ... */
#define BBD_C1_FINAL_G 16            /* ... and the slices its records are dealt into */

struct bbd_c1_plan {
  int N, C, K, H, W, Ho, Wo, P;
  int pixels;                    // N * P
  int tiles;                     // ceil(pixels / TP)
  int mblocks_fwd, mblocks_bwd;  // ceil(K / 64), ceil(C / 64): blockIdx.y of forward and data gradient
  int strips;                    // ceil(pixels / 16)
  int kblocks, cblocks;          // ceil(K / 64), ceil(C / 64): the 64 x 64 blocks of dw
  int splits, per;               // weight gradient: records, and strips per record
};

// 0 = not taken.  N, H, W >= 1; C and K multiples of 16; every tensor and the scratch below 2^31 elements.
BBD_C1_HD int bbd_c1_make_plan(int N, int C, int K, int H, int W, bbd_c1_plan* p) {
  if (N < 1 || H < 1 || W < 1 || C < 16 || K < 16 || C % 16 || K % 16) return 0;
  const long limit = 0x7fffffffL;
  if ((long)C * K > limit || (long)N * C > limit || (long)N * K > limit) return 0;
  if ((long)N * C * H > limit || (long)N * C * H * W > limit) return 0;            // (each a value below 2^31 times an int)
  const int Ho = (int)(((long)H + 1) / 2), Wo = (int)(((long)W + 1) / 2);
  if ((long)Ho * Wo > limit || (long)N * Ho * Wo > limit || (long)N * K * Ho > limit || (long)N * K * Ho * Wo > limit)
    return 0;
  p->N = N; p->C = C; p->K = K; p->H = H; p->W = W; p->Ho = Ho; p->Wo = Wo; p->P = Ho * Wo;
  p->pixels = N * p->P;
  p->tiles = (int)(((long)p->pixels + BBD_C1_TP - 1) / BBD_C1_TP);
  p->mblocks_fwd = (K + 63) / 64;
  p->mblocks_bwd = (C + 63) / 64;
  p->strips = (int)(((long)p->pixels + 15) / 16);
  p->kblocks = (K + 63) / 64;
  p->cblocks = (C + 63) / 64;
  const long blocks = (long)p->kblocks * p->cblocks;
  if (blocks > 65535) return 0;                                                    // (blockIdx.y)
  p->splits = blocks >= BBD_C1_WGRAD_GROUPS ? 1 : (int)(BBD_C1_WGRAD_GROUPS / blocks);
  p->per = (p->strips + p->splits - 1) / p->splits;
  if ((long)p->splits * C * K > limit) return 0;
  return 1;
}

BBD_C1_HD int bbd_c1_plan_scratch_doubles(const bbd_c1_plan* p) { return p->splits * p->C * p->K; }

struct bbd_c1_pixel { int n, pp, oy, ox; };        // pp = oy * Wo + ox

BBD_C1_HD bbd_c1_pixel bbd_c1_decode(const bbd_c1_plan* p, int g) {
  bbd_c1_pixel q;
  q.n = g / p->P;
  q.pp = g - q.n * p->P;
  q.oy = q.pp / p->Wo;
  q.ox = q.pp - q.oy * p->Wo;
  return q;
}

// x / dx [N][C][H][W]: the element under output pixel q of channel c
BBD_C1_HD long bbd_c1_x_offset(const bbd_c1_plan* p, const bbd_c1_pixel* q, int c) {
  return (((long)q->n * p->C + c) * p->H + 2 * q->oy) * p->W + 2 * q->ox;
}
// y / dy [N][K][Ho][Wo]
BBD_C1_HD long bbd_c1_y_offset(const bbd_c1_plan* p, const bbd_c1_pixel* q, int k) {
  return ((long)q->n * p->K + k) * p->P + q->pp;
}
// do the `count` pixels from g on exist, lie in one row of one sample, and do the 2 * count input columns under them?
// Then x[off .. off + 2 count) (off = the first pixel's offset) is one run of a row: whole 16-byte accesses.
BBD_C1_HD int bbd_c1_x_run(const bbd_c1_plan* p, int g, const bbd_c1_pixel* q, int count) {
  return (long)g + count <= p->pixels && q->ox + count <= p->Wo && 2 * (q->ox + count) <= p->W;
}
// do the 4 pixels from g on exist in one sample?  Then y[off .. off + 4) is one run.
BBD_C1_HD int bbd_c1_y_run(const bbd_c1_plan* p, int g, const bbd_c1_pixel* q) {
  return (long)g + 4 <= p->pixels && q->pp + 4 <= p->P;
}

// ---- the LDS tile of forward and data gradient: reduction row r (0 .. RC), pixel i (0 .. TP) of the tile
BBD_C1_HD int bbd_c1_lds_index(int r, int i) { return r * BBD_C1_PITCH + i; }
BBD_C1_HD int bbd_c1_lds_words() { return BBD_C1_RC * BBD_C1_PITCH; }
// the lane's part of every B read, and the part of MFMA j of step s (rows s + 4 q + j) for pixel group pg
BBD_C1_HD int bbd_c1_b_lane(int lane) { return 4 * (lane >> 4) * BBD_C1_PITCH + (lane & 15); }
BBD_C1_HD int bbd_c1_b_step(int s, int j, int pg) { return (s + j) * BBD_C1_PITCH + 16 * pg; }
// rows of the reduction staged in the round that starts at r0 of R
BBD_C1_HD int bbd_c1_round_rows(int R, int r0) { return R - r0 < BBD_C1_RC ? R - r0 : BBD_C1_RC; }
// the weights a lane loads for step s of the round at r0: forward, w[k][r0 + s + 4 q .. + 4) of its channel k (16 bytes,
// aligned: C is a multiple of 16); data gradient, w[r0 + s + 4 q + j][c] for j = 0 .. 3
BBD_C1_HD long bbd_c1_w_fwd(const bbd_c1_plan* p, int mb, int lane, int r0, int s) {
  return ((long)mb * 16 + (lane & 15)) * p->C + r0 + s + 4 * (lane >> 4);
}
BBD_C1_HD long bbd_c1_w_bwd(const bbd_c1_plan* p, int mb, int lane, int r0, int s, int j) {
  return ((long)r0 + s + 4 * (lane >> 4) + j) * p->C + mb * 16 + (lane & 15);
}
// output channel of accumulator register reg of a lane of block mb, and its pixel of group pg of the tile
BBD_C1_HD int bbd_c1_out_channel(int mb, int lane, int reg) { return mb * 16 + 4 * (lane >> 4) + reg; }
BBD_C1_HD int bbd_c1_out_pixel(int tile, int pg, int lane) { return tile * BBD_C1_TP + 16 * pg + (lane & 15); }

// ---- weight gradient
BBD_C1_HD void bbd_c1_split_range(const bbd_c1_plan* p, int split, int* first, int* last) {
  const long a = (long)split * p->per, b = a + p->per;
  *first = (int)(a > p->strips ? p->strips : a);
  *last = (int)(b > p->strips ? p->strips : b);
}
// the two blocks of 16 output (which = 0) or input (1) channels of wave `wave` in block `block` = kblk * cblocks + cblk
BBD_C1_HD int bbd_c1_wave_block(const bbd_c1_plan* p, int block, int wave, int which, int i) {
  const int kblk = block / p->cblocks, cblk = block - kblk * p->cblocks;
  return which == 0 ? kblk * 4 + 2 * (wave >> 1) + i : cblk * 4 + 2 * (wave & 1) + i;
}
BBD_C1_HD int bbd_c1_strip_pixel(int strip, int lane) { return strip * 16 + 4 * (lane >> 4); }   // the lane's first of 4
BBD_C1_HD long bbd_c1_record_index(const bbd_c1_plan* p, int split, int kb, int cb, int lane, int reg) {
  return ((long)split * p->K + kb * 16 + 4 * (lane >> 4) + reg) * p->C + cb * 16 + (lane & 15);
}

#endif  // BBD_CONV1X1_MATH_H
