// Stand-alone walk of one bbd_up2conv3x3_fwd and one bbd_up2conv3x3_bwd call on the host, with the kernels' own index
// arithmetic (baseboostdepth_amd/csrc/bbd_up2conv_math.h) and nothing of the GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 \
//       tests/sanitize/up2conv_index_main.cpp -o up2conv_index_main
//   ./up2conv_index_main N h w [N h w ...]          (C = K = 16)
//
// Every workgroup, wave, strip and lane of both launches is visited in the kernels' order.  Each offset a lane would form
// into z, the LDS tile, out, grad_out, grad_z and scratch is checked against its tensor's size (the tensors are heap
// allocations of exactly that size, so a miss of these checks is a sanitizer report); every element of out, grad_z and
// scratch must be written exactly once.  For shapes of up to BBD_WALK_ARITH source pixels the MFMAs are played as what they
// are, fp32 fma chains over the 4 channel groups of a wave, on small integers and with the identity in place of ELU, so
// both results must equal the plain loops over conv3x3(ReflectionPad2d(1)(nearest_x2(y))) exactly: the lane maps of the
// operands and of the accumulator tile, the summed weights, the clamps and the border terms are inside that comparison.
// Nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_up2conv_math.h"

#define BBD_WALK_ARITH 4096

static int failures = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (failures++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    }                                                                       \
  } while (0)

static const int CH = BBD_UP2CONV_CH;

static float tap_sum(const float* f, int rows, int cols) {
  double s = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      if (((rows >> r) & 1) && ((cols >> c) & 1)) s += (double)f[r * 3 + c];
  return (float)s;
}

// source index that row (column) P of the padded, up-sampled map shows: n = size of the source
static int padded_to_src(int P, int n) {
  int u = P - 1;
  if (u < 0) u = -u;
  if (u >= 2 * n) u = 2 * (2 * n) - 2 - u;
  return u >> 1;
}

static int walk(int N, int h, int w) {
  bbd_up2conv_plan p;
  if (!bbd_up2conv_make_plan(N, CH, CH, h, w, &p)) { fprintf(stderr, "shape not supported\n"); return 1; }
  const bool arith = (long)N * h * w <= BBD_WALK_ARITH;
  const long src_size = (long)N * CH * h * w, out_size = 4 * src_size, scratch_size = bbd_up2conv_plan_scratch_doubles(&p);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> z((size_t)src_size), wt((size_t)CH * CH * 9), out((size_t)out_size, nan), gout((size_t)out_size);
  std::vector<float> gz((size_t)src_size, nan);
  std::vector<unsigned char> out_writes((size_t)out_size, 0), gz_writes((size_t)src_size, 0), scratch_writes((size_t)scratch_size, 0);
  unsigned state = 12345u;
  for (auto& v : z) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 29) - 4); }
  for (auto& v : wt) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 30) - 2); }
  for (auto& v : gout) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 29) - 4); }

  CHECK(p.blocks == N * p.tiles_x * p.tiles_y && p.tiles_x * BBD_UP2CONV_TC >= w && p.tiles_y * BBD_UP2CONV_TR >= h, "plan");
  CHECK(scratch_size == (long)CH * N * h && p.strips * BBD_UP2CONV_STRIP >= w, "plan (backward)");
  CHECK(BBD_UP2CONV_CSTRIDE >= (BBD_UP2CONV_TR + 2) * BBD_UP2CONV_PITCH && BBD_UP2CONV_TR == 2 * BBD_UP2CONV_WAVES, "tile");

  // ---- forward ------------------------------------------------------------------------------------------------------
  std::vector<float> tile((size_t)BBD_UP2CONV_LDS_WORDS);
  std::vector<unsigned char> tile_set((size_t)BBD_UP2CONV_LDS_WORDS);
  const int strips_per_row = BBD_UP2CONV_TC / BBD_UP2CONV_STRIP;
  for (int block = 0; block < p.blocks; ++block) {
    const bbd_up2conv_tile t = bbd_up2conv_decode(&p, block);
    CHECK(t.n >= 0 && t.n < N && t.i0 >= 0 && t.i0 < h && t.j0 >= 0 && t.j0 < w, "block %d -> %d %d %d", block, t.n, t.i0, t.j0);
    std::fill(tile_set.begin(), tile_set.end(), 0);
    for (int e = 0; e < CH * (BBD_UP2CONV_TR + 2) * BBD_UP2CONV_PITCH; ++e) {
      int c, lr, lc;
      bbd_up2conv_fill_decode(e, &c, &lr, &lc);
      const int at = bbd_up2conv_lds_index(c, lr, lc);
      const long from = bbd_up2conv_fill_src(&p, &t, c, lr, lc);
      CHECK(c >= 0 && c < CH && at >= 0 && at < BBD_UP2CONV_LDS_WORDS && !tile_set[(size_t)at], "fill %d -> LDS %d", e, at);
      CHECK(from >= 0 && from < src_size, "fill %d <- z %ld", e, from);
      tile[(size_t)at] = z[(size_t)from];
      tile_set[(size_t)at] = 1;
    }
    for (int wave = 0; wave < BBD_UP2CONV_WAVES; ++wave)
      for (int task = 0; task < 2 * strips_per_row; ++task) {
        const int row = 2 * wave + task / strips_per_row, col0 = (task % strips_per_row) * BBD_UP2CONV_STRIP;
        const int i = t.i0 + row;
        if (i >= h || t.j0 + col0 >= w) continue;
        float acc[2][2][64][4] = {};
        for (int q = 0; q < 4; ++q) {
          float v[64][3][3];
          for (int lane = 0; lane < 64; ++lane)
            for (int dr = 0; dr < 3; ++dr)
              for (int dc = 0; dc < 3; ++dc) {
                const int at = bbd_up2conv_b_index(q, lane, row + dr, col0 + dc);
                CHECK(at >= 0 && at < BBD_UP2CONV_LDS_WORDS && tile_set[(size_t)at], "B operand at LDS %d", at);
                v[lane][dr][dc] = tile[(size_t)at];
              }
          if (!arith) continue;
          for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b)
              for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx)
                  // D[k][pixel] += sum over kk of A[k][kk] B[kk][pixel]: A of lane (k, kk), B of lane (pixel, kk)
                  for (int k = 0; k < 16; ++k)
                    for (int px = 0; px < 16; ++px)
                      for (int kk = 0; kk < 4; ++kk) {
                        const float wa = tap_sum(&wt[(size_t)((k * CH + 4 * q + kk) * 9)], bbd_up2conv_taps(a, dy), bbd_up2conv_taps(b, dx));
                        const float d = v[kk * 16 + px][1 + bbd_up2conv_tap_offset(a, dy)][1 + bbd_up2conv_tap_offset(b, dx)];
                        acc[a][b][(k >> 2) * 16 + px][k & 3] += wa * d;
                      }
        }
        for (int lane = 0; lane < 64; ++lane) {
          const int j = t.j0 + col0 + (lane & 15);
          if (j >= w) continue;
          for (int a = 0; a < 2; ++a)
            for (int reg = 0; reg < 4; ++reg)
              for (int b = 0; b < 2; ++b) {
                const long o = bbd_up2conv_out_offset(&p, t.n, 4 * (lane >> 4) + reg, 2 * i + a, 2 * j) + b;
                CHECK(o >= 0 && o < out_size, "out offset %ld", o);
                if (o >= 0 && o < out_size) { out[(size_t)o] = acc[a][b][lane][reg]; ++out_writes[(size_t)o]; }
              }
        }
      }
  }
  for (long o = 0; o < out_size; ++o) CHECK(out_writes[(size_t)o] == 1, "out %ld written %d times", o, out_writes[(size_t)o]);

  // ---- backward -----------------------------------------------------------------------------------------------------
  for (int block = 0; block < p.groups; ++block) {
    int n, i;
    const int group = bbd_up2conv_group(&p, block, &n, &i);
    CHECK(group >= 0 && group < p.groups && n >= 0 && n < N && i >= 0 && i < h, "block %d -> group %d: %d %d", block, group, n, i);
    for (int wave = 0; wave < BBD_UP2CONV_WAVES; ++wave)
      for (int strip = wave; strip < p.strips; strip += BBD_UP2CONV_WAVES) {
        float acc[64][4] = {};
        for (int u = 0; u < 4; ++u) {
          if (!bbd_up2conv_row_live(&p, i, u)) continue;
          float d[64][3][4];
          for (int lane = 0; lane < 64; ++lane) {
            const int j = strip * BBD_UP2CONV_STRIP + (lane & 15);
            for (int q = 0; q < 4; ++q) {
              const long g = bbd_up2conv_g_offset(&p, n, 4 * q + (lane >> 4), 2 * i - 1 + u, j);
              float v[4];
              for (int tt = 0; tt < 4; ++tt) {
                const bool live = bbd_up2conv_g_live(&p, j, tt);
                if (live) CHECK(g + tt >= 0 && g + tt < out_size, "grad_out offset %ld", g + tt);
                v[tt] = live ? gout[(size_t)(g + tt)] : 0.0f;
              }
              if (j > 0 && j < w - 1) CHECK(bbd_up2conv_g_live(&p, j, 0) && bbd_up2conv_g_live(&p, j, 3), "16-byte load at j %d", j);
              d[lane][0][q] = v[2] + v[3] + (j == 0 ? v[1] : 0.0f);
              d[lane][1][q] = v[1] + v[2];
              d[lane][2][q] = v[0] + v[1] + (j == w - 1 ? v[2] : 0.0f);
            }
          }
          if (!arith) continue;
          for (int pass = 0; pass < 2; ++pass) {                       // 0: the row's own taps; 1: the clamp's extra kernel row
            int rows = bbd_up2conv_bwd_taps(u);
            if (pass == 1) {
              if (u == 1 && i == 0) rows = bbd_up2conv_bwd_taps(3);
              else if (u == 2 && i == h - 1) rows = bbd_up2conv_bwd_taps(0);
              else continue;
            }
            for (int s = 0; s < 3; ++s)
              for (int q = 0; q < 4; ++q)
                for (int c = 0; c < 16; ++c)
                  for (int px = 0; px < 16; ++px)
                    for (int kk = 0; kk < 4; ++kk) {
                      const float wb = tap_sum(&wt[(size_t)(((4 * q + kk) * CH + c) * 9)], rows, 1 << s);
                      acc[(c >> 2) * 16 + px][c & 3] += wb * d[kk * 16 + px][s][q];
                    }
          }
        }
        for (int lane = 0; lane < 64; ++lane) {
          const int j = strip * BBD_UP2CONV_STRIP + (lane & 15);
          if (j >= w) continue;
          for (int reg = 0; reg < 4; ++reg) {
            const long o = bbd_up2conv_src_offset(&p, n, 4 * (lane >> 4) + reg, i, j);
            CHECK(o >= 0 && o < src_size, "grad_z offset %ld", o);
            if (o >= 0 && o < src_size) { gz[(size_t)o] = acc[lane][reg]; ++gz_writes[(size_t)o]; }
          }
        }
      }
    for (int c = 0; c < CH; ++c) {
      const long s = bbd_up2conv_scratch_index(&p, c, group);
      CHECK(s >= 0 && s < scratch_size, "scratch offset %ld", s);
      if (s >= 0 && s < scratch_size) ++scratch_writes[(size_t)s];
    }
  }
  for (long o = 0; o < src_size; ++o) CHECK(gz_writes[(size_t)o] == 1, "grad_z %ld written %d times", o, gz_writes[(size_t)o]);
  for (long s = 0; s < scratch_size; ++s) CHECK(scratch_writes[(size_t)s] == 1, "scratch %ld written %d times", s, scratch_writes[(size_t)s]);
  for (int c = 0; c < CH; ++c)                                         // the final launch: lane l reads groups l, l + 64, ...
    for (int lane = 0; lane < BBD_UP2CONV_FINAL_THREADS; ++lane)
      for (int g = lane; g < p.groups; g += BBD_UP2CONV_FINAL_THREADS) {
        const long s = bbd_up2conv_scratch_index(&p, c, g);
        CHECK(s >= 0 && s < scratch_size && scratch_writes[(size_t)s] == 1, "final read %ld", s);
      }

  // ---- the plain loops ----------------------------------------------------------------------------------------------
  if (arith) {
    std::vector<float> ref_gz((size_t)src_size, 0.0f);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < CH; ++k)
        for (int Y = 0; Y < 2 * h; ++Y)
          for (int X = 0; X < 2 * w; ++X) {
            float sum = 0.0f;
            const long o = bbd_up2conv_out_offset(&p, n, k, Y, X);
            for (int c = 0; c < CH; ++c)
              for (int r = 0; r < 3; ++r)
                for (int s = 0; s < 3; ++s) {
                  const long from = bbd_up2conv_src_offset(&p, n, c, padded_to_src(Y + r, h), padded_to_src(X + s, w));
                  const float wv = wt[(size_t)((k * CH + c) * 9 + r * 3 + s)];
                  sum += wv * z[(size_t)from];
                  ref_gz[(size_t)from] += wv * gout[(size_t)o];
                }
            CHECK(out[(size_t)o] == sum, "out[%d][%d][%d][%d] = %g, plain loop %g", n, k, Y, X, out[(size_t)o], sum);
          }
    for (long o = 0; o < src_size; ++o) CHECK(gz[(size_t)o] == ref_gz[(size_t)o], "grad_z[%ld] = %g, plain loop %g", o, gz[(size_t)o], ref_gz[(size_t)o]);
  }
  printf("N %d h %d w %d: %d tiles, %d groups, %ld scratch doubles, %s: %s\n", N, h, w, p.blocks, p.groups, scratch_size,
         arith ? "values compared" : "addresses only", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3) { fprintf(stderr, "usage: %s N h w [N h w ...]\n", argv[0]); return 2; }
  int rc = 0;
  for (int a = 1; a + 2 < argc; a += 3) rc |= walk(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]));
  return rc;
}
