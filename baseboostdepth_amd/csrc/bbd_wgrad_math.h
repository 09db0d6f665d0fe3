// bbd_wgrad_math.h - the index arithmetic of the 3x3 weight-gradient kernels (bbd_wgrad.hip), shared with the host
// program that walks every offset of a launch (tests/sanitize/wgrad_index_main.cpp).  No arithmetic on data here: which
// workgroup, wave and lane touches which element of xp, grad_z, scratch and grad_w, and nothing else.
//
// The weight gradient of a 3x3, stride-1 convolution of a pre-padded input is a GEMM whose reduction runs over pixels:
//   dw[k][c][r][s] = sum over (n, y, x) of grad_z[n][k][y][x] * xp[n][c][y + r][x + s].
// A STRIP is 16 neighbouring output pixels of one row: strip id = (n * H + y) * SW + xs, SW = ceil(W / 16), first column
// x0 = 16 xs.  One v_mfma_f32_16x16x4_f32 contracts 4 pixels of 16 output channels (A) with 16 input channels (B):
// lane l holds channel l & 15 of both operands at the pixels x0 + 4 (l >> 4) + j, j = 0..3, and MFMA j takes component j.
// A ROLE is one block of 16 output channels with NCB (1 or 2) blocks of 16 input channels: 9 NCB accumulator tiles of 4
// registers.  Workgroup (group, role) of BBD_WGRAD_WAVES waves owns the strips [group * WAVES * per, (group + 1) * WAVES *
// per) of that role, `per` neighbouring strips per wave; every BBD_WGRAD_RUN products a wave's fp32 tiles are widened
// and added into the workgroup's doubles, which end as record (group, role) of `scratch`.
#ifndef BBD_WGRAD_MATH_H
#define BBD_WGRAD_MATH_H

#ifdef __HIPCC__
#define BBD_WG_HD __host__ __device__ inline
#else
#define BBD_WG_HD inline
#endif

#define BBD_WGRAD_WAVES 8          /* waves of a workgroup */
#define BBD_WGRAD_STRIP 16         /* pixels of a strip = products one strip adds to an accumulator */
#define BBD_WGRAD_MIN_PER 12       /* strips per wave below which a launch takes fewer workgroups instead */
#define BBD_WGRAD_MAX_BLOCKS 512   /* workgroups of a launch (all roles): two per CU */
#define BBD_WGRAD_TILE 256         /* elements of one 16 x 16 accumulator tile */
#define BBD_WGRAD_FINAL_E 16       /* record elements of one workgroup of the final launch ... */
#define BBD_WGRAD_FINAL_G 16       /* ... and the slices its groups are dealt into */

struct bbd_wgrad_plan {
  int N, C, K, H, W;
  int ncb;      // blocks of 16 input channels per role: 2 where C / 16 is even, else 1
  int roles;    // (K / 16) * (C / 16 / ncb)
  int sw;       // strips per row
  int strips;   // N * H * sw (below 2^31: no more than grad_z has elements)
  int groups;   // workgroups per role
  int per;      // strips per wave
  int run;      // strips per fp32 run: BBD_WGRAD_RUN / 16
  int record;   // doubles of one (group, role) record: 9 * ncb * 256
};

// 0 = not taken.  Channels in whole blocks of 16, every tensor and the scratch below 2^31 elements.
BBD_WG_HD int bbd_wgrad_make_plan(int N, int C, int K, int H, int W, int run_products, bbd_wgrad_plan* p) {
  if (N < 1 || C < 16 || K < 16 || H < 1 || W < 1 || (C & 15) || (K & 15) || C > 1024 || K > 1024) return 0;
  const long limit = 0x7fffffffL;
  if ((long)N * C * (H + 2) * (W + 2) > limit || (long)N * K * H * W > limit) return 0;
  p->N = N; p->C = C; p->K = K; p->H = H; p->W = W;
  p->ncb = ((C / 16) & 1) ? 1 : 2;
  p->roles = (K / 16) * (C / 16 / p->ncb);
  p->sw = (W + BBD_WGRAD_STRIP - 1) / BBD_WGRAD_STRIP;
  p->strips = N * H * p->sw;
  const long per_group = (long)BBD_WGRAD_WAVES * BBD_WGRAD_MIN_PER;
  long groups = ((long)p->strips + per_group - 1) / per_group;
  const long most = BBD_WGRAD_MAX_BLOCKS / p->roles > 1 ? BBD_WGRAD_MAX_BLOCKS / p->roles : 1;
  groups = groups > most ? most : groups;
  p->groups = (int)groups;
  const long slots = groups * BBD_WGRAD_WAVES;
  const long per = (p->strips + slots - 1) / slots;
  if (per > limit) return 0;
  p->per = (int)per;
  p->run = run_products / BBD_WGRAD_STRIP;
  p->record = 9 * p->ncb * BBD_WGRAD_TILE;
  if (groups * p->roles * p->record > limit) return 0;
  return 1;
}

BBD_WG_HD int bbd_wgrad_plan_scratch_doubles(const bbd_wgrad_plan* p) { return p->groups * p->roles * p->record; }

// the block of output channels and the first block of input channels of a role
BBD_WG_HD void bbd_wgrad_role(const bbd_wgrad_plan* p, int role, int* kb, int* cb0) {
  const int pairs = p->C / 16 / p->ncb;
  *kb = role / pairs;
  *cb0 = (role - *kb * pairs) * p->ncb;
}

// strips [first, last) of wave `wave` of workgroup `group` (an empty range past the end of the image list)
BBD_WG_HD void bbd_wgrad_wave_range(const bbd_wgrad_plan* p, int group, int wave, int* first, int* last) {
  const long slot = (long)group * BBD_WGRAD_WAVES + wave;
  long a = slot * p->per, b = a + p->per;
  a = a > p->strips ? p->strips : a;
  b = b > p->strips ? p->strips : b;
  *first = (int)a; *last = (int)b;
}

// Does an fp32 run end after step i (0 <= i < per) of a wave's range?  After every `run` strips and after the last
// step: the waves of a workgroup then widen their tiles, so no accumulator ever takes more than run * 16 products.
BBD_WG_HD int bbd_wgrad_run_ends(const bbd_wgrad_plan* p, int i) { return (i + 1) % p->run == 0 || i + 1 == p->per; }

struct bbd_wgrad_strip {
  int n, y, x0;
  int full;   // all 16 pixels inside the row: every lane takes its 16-byte accesses
};

BBD_WG_HD bbd_wgrad_strip bbd_wgrad_decode(const bbd_wgrad_plan* p, int strip) {
  bbd_wgrad_strip s;
  const int row = strip / p->sw;
  s.x0 = (strip - row * p->sw) * BBD_WGRAD_STRIP;
  s.n = row / p->H;
  s.y = row - s.n * p->H;
  s.full = s.x0 + BBD_WGRAD_STRIP <= p->W;
  return s;
}
// the strip after `s` without a division: what a wave does between two strips of its range
BBD_WG_HD bbd_wgrad_strip bbd_wgrad_next(const bbd_wgrad_plan* p, bbd_wgrad_strip s) {
  s.x0 += BBD_WGRAD_STRIP;
  if (s.x0 >= p->W) {
    s.x0 = 0;
    if (++s.y == p->H) { s.y = 0; ++s.n; }
  }
  s.full = s.x0 + BBD_WGRAD_STRIP <= p->W;
  return s;
}

// lane's first pixel of a strip, and how many of its 4 pixels lie inside the row (0..4)
BBD_WG_HD int bbd_wgrad_lane_x(const bbd_wgrad_strip* s, int lane) { return s->x0 + 4 * (lane >> 4); }
BBD_WG_HD int bbd_wgrad_lane_pixels(const bbd_wgrad_plan* p, const bbd_wgrad_strip* s, int lane) {
  const int left = p->W - bbd_wgrad_lane_x(s, lane);
  return left < 0 ? 0 : left > 4 ? 4 : left;
}
// offset of grad_z[n][16 kb + (lane & 15)][y][lane's first pixel]; the lane reads bbd_wgrad_lane_pixels floats from it
// = a part that is the same for the whole wave + a part that is the lane's for every strip (below 2^31: inside one image)
BBD_WG_HD long bbd_wgrad_gz_base(const bbd_wgrad_plan* p, const bbd_wgrad_strip* s, int kb) {
  return (((long)s->n * p->K + kb * 16) * p->H + s->y) * p->W + s->x0;
}
BBD_WG_HD int bbd_wgrad_gz_lane(const bbd_wgrad_plan* p, int lane) { return (lane & 15) * p->H * p->W + 4 * (lane >> 4); }
BBD_WG_HD long bbd_wgrad_gz_offset(const bbd_wgrad_plan* p, const bbd_wgrad_strip* s, int kb, int lane) {
  return bbd_wgrad_gz_base(p, s, kb) + bbd_wgrad_gz_lane(p, lane);
}
// offset of xp[n][16 cb + (lane & 15)][y + r][lane's first pixel]: the lane reads its pixels + 2 floats from it (6 in
// a full strip: one 16-byte and one 8-byte access), none where it has no pixel
BBD_WG_HD long bbd_wgrad_xp_base(const bbd_wgrad_plan* p, const bbd_wgrad_strip* s, int cb, int r) {
  return (((long)s->n * p->C + cb * 16) * (p->H + 2) + s->y + r) * (p->W + 2) + s->x0;
}
BBD_WG_HD int bbd_wgrad_xp_lane(const bbd_wgrad_plan* p, int lane) {
  return (lane & 15) * (p->H + 2) * (p->W + 2) + 4 * (lane >> 4);
}
BBD_WG_HD long bbd_wgrad_xp_offset(const bbd_wgrad_plan* p, const bbd_wgrad_strip* s, int cb, int r, int lane) {
  return bbd_wgrad_xp_base(p, s, cb, r) + bbd_wgrad_xp_lane(p, lane);
}

// Record element of accumulator register `reg` (0..3) of lane `lane`, tap (r, s), local channel block cbl.  A record is
// [ncb][3 rows r][3 taps s][64 lanes][4 registers]; the tile's element is D[16 kb + 4 (lane >> 4) + reg][16 cb + (lane & 15)].
BBD_WG_HD int bbd_wgrad_record_index(int cbl, int r, int s, int lane, int reg) {
  return (((cbl * 3 + r) * 3 + s) * 64 + lane) * 4 + reg;
}
// ... and where that element goes in grad_w [K, C, 3, 3]
BBD_WG_HD long bbd_wgrad_record_to_weight(const bbd_wgrad_plan* p, int role, int e) {
  int kb, cb0;
  bbd_wgrad_role(p, role, &kb, &cb0);
  const int reg = e & 3, lane = (e >> 2) & 63, t = e >> 8;      // t = (cbl * 3 + r) * 3 + s
  const int cbl = t / 9, tap = t - cbl * 9;
  const int k = kb * 16 + 4 * (lane >> 4) + reg, c = (cb0 + cbl) * 16 + (lane & 15);
  return ((long)k * p->C + c) * 9 + tap;
}
BBD_WG_HD long bbd_wgrad_record_offset(const bbd_wgrad_plan* p, int group, int role) {
  return ((long)group * p->roles + role) * p->record;
}

#endif  // BBD_WGRAD_MATH_H
