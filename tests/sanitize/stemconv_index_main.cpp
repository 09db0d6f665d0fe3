// Stand-alone walk of one bbd_stem_conv7s2_fwd and one bbd_stem_conv7s2_wgrad call on the host, with the kernels' own
// index arithmetic (baseboostdepth_amd/csrc/bbd_stemconv_math.h) and nothing of the GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 \
//       tests/sanitize/stemconv_index_main.cpp -o stemconv_index_main
//   ./stemconv_index_main N C H W [N C H W ...]          (K = 64, 7 x 7)
//
// Every workgroup, wave, strip and lane of both launches is visited in the kernels' order.  Each offset a lane would form
// into x, w, the LDS tile, out, grad_out, scratch and grad_w is checked against its tensor's size (the tensors are heap
// allocations of exactly that size, so a miss of these checks is a sanitizer report); every element of out, scratch and
// grad_w must be written exactly once and no word of the tile read before it is staged (the operands' LDS offsets are
// the same in every tile: a shape too large for the arithmetic walks them in its first tile).  For shapes of up to
// BBD_WALK_ARITH input pixels the MFMAs are played as what they are, fp32 fma chains over the 4 k-groups of a wave, on
// small integers, so both results must equal the plain loops exactly: the lane maps of the operands and of the
// accumulator tile, the two planes, the zero border and the record layout are inside that comparison.
// Nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_stemconv_math.h"

#define BBD_WALK_ARITH 32768

static int failures = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (failures++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    }                                                                       \
  } while (0)

static const int K = BBD_STEM_K;

static int walk(int N, int C, int H, int W) {
  bbd_stem_plan p;
  if (!bbd_stem_make_plan(N, C, K, H, W, 7, 7, &p)) { fprintf(stderr, "shape not supported\n"); return 1; }
  const bool arith = (long)N * C * H * W <= BBD_WALK_ARITH;
  const long x_size = (long)N * C * H * W, out_size = (long)N * K * p.Ho * p.Wo, w_size = (long)K * C * 49;
  const long scratch_size = bbd_stem_plan_scratch_doubles(&p);
  const int words = bbd_stem_lds_words(C);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> x((size_t)x_size), wt((size_t)w_size), out((size_t)out_size, nan), go((size_t)out_size);
  std::vector<float> gw((size_t)w_size, nan);
  std::vector<double> scratch((size_t)scratch_size, (double)nan);
  std::vector<unsigned char> out_writes((size_t)out_size, 0), scratch_writes((size_t)scratch_size, 0), gw_writes((size_t)w_size, 0);
  unsigned state = 12345u;
  for (auto& v : x) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 29) - 4); }
  for (auto& v : wt) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 30) - 2); }
  for (auto& v : go) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 29) - 4); }

  CHECK(p.Ho == (H + 1) / 2 && p.Wo == (W + 1) / 2 && p.tiles == N * p.tiles_x * p.tiles_y, "plan");
  CHECK(p.tiles_x * BBD_STEM_TW >= p.Wo && p.tiles_y * BBD_STEM_TH >= p.Ho, "plan (tiles)");
  CHECK(p.cols == C * 49 && p.ctiles * 16 >= p.cols && 2 * p.nct >= p.ctiles, "plan (columns)");
  CHECK(p.groups >= 1 && p.groups <= BBD_STEM_WGRAD_GROUPS && (long)p.groups * p.per >= p.tiles &&
        (long)(p.groups - 1) * p.per < p.tiles, "plan (groups)");
  CHECK(p.record == BBD_STEM_WGRAD_WAVES * p.nct * 256 && p.record % BBD_STEM_FINAL_E == 0, "plan (record)");
  CHECK(BBD_STEM_RUN_STRIPS * 16 <= BBD_WGRAD_RUN && BBD_STEM_STRIPS % BBD_STEM_RUN_STRIPS == 0, "fp32 run");

  std::vector<float> tile((size_t)words);
  std::vector<unsigned char> tile_set((size_t)words);
  auto stage = [&](const bbd_stem_tile& t) {
    std::fill(tile_set.begin(), tile_set.end(), 0);
    for (int e = 0; e < C * BBD_STEM_ROWS * BBD_STEM_PITCH; ++e) {
      int c, ly, lx;
      bbd_stem_fill_decode(e, &c, &ly, &lx);
      const int at = bbd_stem_lds_index(c, ly, lx);
      const long from = bbd_stem_fill_src(&p, &t, c, ly, lx);
      CHECK(c >= 0 && c < C && ly >= 0 && ly < BBD_STEM_ROWS && at >= 0 && at < words && !tile_set[(size_t)at], "fill %d -> LDS %d", e, at);
      CHECK(from >= -1 && from < x_size, "fill %d <- x %ld", e, from);
      if (at < 0 || at >= words) continue;
      tile[(size_t)at] = from >= 0 && from < x_size ? x[(size_t)from] : 0.0f;
      tile_set[(size_t)at] = 1;
    }
  };

  // ---- forward ------------------------------------------------------------------------------------------------------
  for (int block = 0; block < p.tiles; ++block) {
    const bbd_stem_tile t = bbd_stem_decode(&p, block);
    CHECK(t.n >= 0 && t.n < N && t.oy0 >= 0 && t.oy0 < p.Ho && t.ox0 >= 0 && t.ox0 < p.Wo, "block %d -> %d %d %d", block, t.n, t.oy0, t.ox0);
    stage(t);
    const bool operands = arith || block == 0;       // the operands' LDS offsets do not depend on the tile
    for (int kb = 0; kb < BBD_STEM_FWD_WAVES; ++kb)
      for (int pair = 0; pair < BBD_STEM_TH / 2; ++pair) {
        const int oyl = 2 * pair;
        if (t.oy0 + oyl >= p.Ho) break;
        float acc[2][2][64][4] = {};
        for (int c = 0; c < C; ++c)
          for (int r = 0; r < 7; ++r)
            for (int par = 0; operands && par < 2; ++par)
              for (int a = 0; a < 2; ++a)
                for (int g = 0; g < 2; ++g) {
                  float A[64], B[64];
                  for (int lane = 0; lane < 64; ++lane) {
                    const int wi = bbd_stem_fwd_w_index(C, kb, lane, c, r, par);
                    CHECK(wi >= -1 && wi < w_size, "weight offset %d", wi);
                    A[lane] = wi >= 0 && wi < w_size ? wt[(size_t)wi] : 0.0f;
                    const int at = bbd_stem_fwd_b_lane(lane) + bbd_stem_fwd_b_tap(0, 0, 0, oyl, 0) + bbd_stem_fwd_b_tap(c, r, par, a, g);
                    CHECK(at >= 0 && at < words && tile_set[(size_t)at], "B operand at LDS %d", at);
                    B[lane] = at >= 0 && at < words ? tile[(size_t)at] : 0.0f;
                  }
                  if (!arith) continue;
                  // D[i][j] += sum over q of A[i][q] B[q][j]: A of lane (i, q) = 16 q + i, B of lane 16 q + j
                  for (int i = 0; i < 16; ++i)
                    for (int j = 0; j < 16; ++j)
                      for (int q = 0; q < 4; ++q) acc[a][g][(i >> 2) * 16 + j][i & 3] += A[16 * q + i] * B[16 * q + j];
                }
        for (int a = 0; a < 2; ++a)
          for (int g = 0; g < 2; ++g)
            for (int lane = 0; lane < 64; ++lane) {
              const int oy = t.oy0 + oyl + a, ox = t.ox0 + (lane & 15) + 16 * g;
              if (oy >= p.Ho || ox >= p.Wo) continue;
              for (int reg = 0; reg < 4; ++reg) {
                const long o = bbd_stem_out_offset(&p, t.n, kb * 16 + 4 * (lane >> 4) + reg, oy, ox);
                CHECK(o >= 0 && o < out_size, "out offset %ld", o);
                if (o >= 0 && o < out_size) { out[(size_t)o] = acc[a][g][lane][reg]; ++out_writes[(size_t)o]; }
              }
            }
      }
  }
  for (long o = 0; o < out_size; ++o) CHECK(out_writes[(size_t)o] == 1, "out %ld written %d times", o, out_writes[(size_t)o]);

  // ---- weight gradient ----------------------------------------------------------------------------------------------
  const int nct = p.nct;
  for (int group = 0; group < p.groups; ++group) {
    int first, last;
    bbd_stem_group_range(&p, group, &first, &last);
    CHECK(first >= 0 && first < last && last <= p.tiles && (group == 0 || first == group * p.per), "group %d: tiles %d..%d", group, first, last);
    if (group == p.groups - 1) CHECK(last == p.tiles, "the last group ends at tile %d of %d", last, p.tiles);
    std::vector<float> acc((size_t)BBD_STEM_WGRAD_WAVES * nct * 256, 0.0f);
    std::vector<double> total((size_t)BBD_STEM_WGRAD_WAVES * nct * 256, 0.0);
    for (int id = first; id < last; ++id) {
      const bbd_stem_tile t = bbd_stem_decode(&p, id);
      stage(t);
      int products = 0;
      for (int st = 0; st < BBD_STEM_STRIPS; ++st) {
        for (int wave = 0; wave < BBD_STEM_WGRAD_WAVES; ++wave) {
          const int kb = wave & 3;
          float g[64][4];
          for (int lane = 0; lane < 64; ++lane) {
            const int pixels = bbd_stem_go_pixels(&p, &t, st, lane);
            const long from = bbd_stem_go_offset(&p, &t, st, kb, lane);
            CHECK(pixels >= 0 && pixels <= 4, "pixels %d", pixels);
            for (int j = 0; j < 4; ++j) {
              if (j < pixels) CHECK(from + j >= 0 && from + j < out_size, "grad_out offset %ld", from + j);
              g[lane][j] = j < pixels && from + j >= 0 && from + j < out_size ? go[(size_t)(from + j)] : 0.0f;
            }
          }
          for (int ct = 0; (arith || id == 0) && ct < nct; ++ct) {
            const int ctile = bbd_stem_wave_ctile(&p, wave, ct);
            if (ctile >= p.ctiles) continue;
            for (int j = 0; j < 4; ++j) {
              float B[64];
              for (int lane = 0; lane < 64; ++lane) {
                const int at = bbd_stem_wgrad_b_strip(st) + bbd_stem_wgrad_b_lane(&p, ctile, lane) + j;
                CHECK(at >= 0 && at < words && tile_set[(size_t)at], "B operand at LDS %d", at);
                B[lane] = at >= 0 && at < words ? tile[(size_t)at] : 0.0f;
              }
              if (!arith) continue;
              for (int i = 0; i < 16; ++i)
                for (int col = 0; col < 16; ++col)
                  for (int q = 0; q < 4; ++q)
                    acc[(size_t)bbd_stem_record_index(&p, wave, ct, (i >> 2) * 16 + col, i & 3)] += g[16 * q + i][j] * B[16 * q + col];
            }
          }
        }
        products += 16;
        CHECK(products <= BBD_WGRAD_RUN, "an accumulator with %d products", products);
        if ((st + 1) % BBD_STEM_RUN_STRIPS == 0) {
          for (size_t e = 0; e < acc.size(); ++e) { total[e] += (double)acc[e]; acc[e] = 0.0f; }
          products = 0;
        }
      }
      CHECK(products == 0, "a tile ends inside an fp32 run");
    }
    for (int wave = 0; wave < BBD_STEM_WGRAD_WAVES; ++wave)
      for (int ct = 0; ct < nct; ++ct)
        for (int lane = 0; lane < 64; ++lane)
          for (int reg = 0; reg < 4; ++reg) {
            const int e = bbd_stem_record_index(&p, wave, ct, lane, reg);
            const long s = bbd_stem_record_offset(&p, group) + e;
            CHECK(e >= 0 && e < p.record && s >= 0 && s < scratch_size, "scratch offset %ld", s);
            if (s >= 0 && s < scratch_size) { scratch[(size_t)s] = total[(size_t)e]; ++scratch_writes[(size_t)s]; }
          }
  }
  for (long s = 0; s < scratch_size; ++s) CHECK(scratch_writes[(size_t)s] == 1, "scratch %ld written %d times", s, scratch_writes[(size_t)s]);
  for (int block = 0; block < p.record / BBD_STEM_FINAL_E; ++block)          // the final launch
    for (int e16 = 0; e16 < BBD_STEM_FINAL_E; ++e16) {
      const int e = block * BBD_STEM_FINAL_E + e16;
      double part[BBD_STEM_FINAL_G];
      for (int slice = 0; slice < BBD_STEM_FINAL_G; ++slice) {
        part[slice] = 0.0;
        for (int g = slice; g < p.groups; g += BBD_STEM_FINAL_G) {
          const long s = bbd_stem_record_offset(&p, g) + e;
          CHECK(s >= 0 && s < scratch_size && scratch_writes[(size_t)s] == 1, "final read %ld", s);
          if (s >= 0 && s < scratch_size) part[slice] += scratch[(size_t)s];
        }
      }
      double sum = 0.0;
      for (int q = 0; q < BBD_STEM_FINAL_G; ++q) sum += part[q];
      const int at = bbd_stem_record_to_weight(&p, e);
      CHECK(at >= -1 && at < w_size, "grad_w offset %d", at);
      if (at >= 0 && at < w_size) { gw[(size_t)at] = (float)sum; ++gw_writes[(size_t)at]; }
    }
  for (long o = 0; o < w_size; ++o) CHECK(gw_writes[(size_t)o] == 1, "grad_w %ld written %d times", o, gw_writes[(size_t)o]);

  // ---- the plain loops ----------------------------------------------------------------------------------------------
  if (arith) {
    std::vector<float> ref_gw((size_t)w_size, 0.0f);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k)
        for (int oy = 0; oy < p.Ho; ++oy)
          for (int ox = 0; ox < p.Wo; ++ox) {
            float sum = 0.0f;
            const long o = bbd_stem_out_offset(&p, n, k, oy, ox);
            for (int c = 0; c < C; ++c)
              for (int r = 0; r < 7; ++r)
                for (int s = 0; s < 7; ++s) {
                  const int iy = 2 * oy + r - 3, ix = 2 * ox + s - 3;
                  if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                  const float xv = x[(size_t)((((long)n * C + c) * H + iy) * W + ix)];
                  const size_t wi = (size_t)(((k * C + c) * 7 + r) * 7 + s);
                  sum += wt[wi] * xv;
                  ref_gw[wi] += go[(size_t)o] * xv;
                }
            CHECK(out[(size_t)o] == sum, "out[%d][%d][%d][%d] = %g, plain loop %g", n, k, oy, ox, out[(size_t)o], sum);
          }
    for (long o = 0; o < w_size; ++o) CHECK(gw[(size_t)o] == ref_gw[(size_t)o], "grad_w[%ld] = %g, plain loop %g", o, gw[(size_t)o], ref_gw[(size_t)o]);
  }
  printf("N %d C %d H %d W %d: %d tiles, %d groups, %ld scratch doubles, %s: %s\n", N, C, H, W, p.tiles, p.groups, scratch_size,
         arith ? "values compared" : "addresses only", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) { fprintf(stderr, "usage: %s N C H W [N C H W ...]\n", argv[0]); return 2; }
  int rc = 0;
  for (int a = 1; a + 3 < argc; a += 4) rc |= walk(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]));
  return rc;
}
