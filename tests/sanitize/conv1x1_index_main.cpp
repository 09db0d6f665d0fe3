// conv1x1_index_main.cpp - a stand-alone host walk of every launch of bbd_conv1x1s2_fwd / _bwd_data / _wgrad
// (baseboostdepth_amd/csrc/bbd_conv1x1.hip) through the kernels' own index arithmetic (bbd_conv1x1_math.h), meant to be
// built with -fsanitize=address,undefined: every tensor, the LDS tile and the scratch are heap blocks of exactly their
// size, so an offset outside one is an error of the sanitizer.  The walk repeats the kernels' control flow lane by lane
// on small integers (every sum is exact in float), so besides addresses it checks that every element of y, of dx in
// plain mode, of every scratch record and of dw is written exactly once, that accumulate mode touches the even positions
// only, that no LDS word and no scratch double is read before it was written, and the values against the plain loops.
//
//   conv1x1_index_main N C K H W [N C K H W ...]      one line per shape, ending in ": ok"; exit status 1 on a mismatch
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../baseboostdepth_amd/csrc/bbd_conv1x1_math.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

struct Buf {                       // a tensor: exact-size heap block + how often each element was written
  float* v;
  int* writes;
  long n;
  explicit Buf(long count) : v(new float[count]), writes(new int[count]()), n(count) {}
  ~Buf() { delete[] v; delete[] writes; }
  void put(long at, float value) { v[at] = value; ++writes[at]; }
};

int small(long i, int mod, int off) { return (int)((i * 2654435761u >> 7) % (unsigned)mod) - off; }

// D[4 q + r][i] += sum over q' of A[lane q' * 16 + (4 q + r)] * B[lane q' * 16 + i], lane = 16 q + i
void mfma(const float* a, const float* b, float (*d)[4]) {
  for (int lane = 0; lane < 64; ++lane)
    for (int reg = 0; reg < 4; ++reg) {
      const int row = 4 * (lane >> 4) + reg, col = lane & 15;
      float s = d[lane][reg];
      for (int q = 0; q < 4; ++q) s += a[q * 16 + row] * b[q * 16 + col];
      d[lane][reg] = s;
    }
}

// forward (dgrad == 0) and data gradient (1: plain, 2: accumulate) share the tile; `in` is x or dy, `out` y or dx
void walk_gemm(const bbd_c1_plan& p, int dgrad, const Buf& in, const Buf& w, Buf& out) {
  const int R = dgrad ? p.K : p.C, M = dgrad ? p.C : p.K, mblocks = dgrad ? p.mblocks_bwd : p.mblocks_fwd;
  const int threads = BBD_C1_WAVES * 64;
  for (int tile_id = 0; tile_id < p.tiles; ++tile_id)
    for (int by = 0; by < mblocks; ++by) {
      float* tile = new float[bbd_c1_lds_words()];
      std::vector<int> round_of(bbd_c1_lds_words(), -1);
      std::vector<float> acc(BBD_C1_WAVES * 4 * 64 * 4, 0.f);           // [wave][pg][lane][reg]
      const int g0 = tile_id * BBD_C1_TP;
      int round = 0;
      for (int r0 = 0; r0 < R; r0 += BBD_C1_RC, ++round) {
        const int rows = bbd_c1_round_rows(R, r0);
        for (int t = 0; t < threads; ++t) {
          if (!dgrad) {
            const int pr = t & 31, g = g0 + 2 * pr;
            const bbd_c1_pixel q0 = bbd_c1_decode(&p, g < p.pixels ? g : 0), q1 = bbd_c1_decode(&p, g + 1 < p.pixels ? g + 1 : 0);
            const bool run = bbd_c1_x_run(&p, g, &q0, 2);
            for (int i = 0; i < BBD_C1_RC * 32 / threads; ++i) {
              const int cc = (t >> 5) + i * (threads / 32);
              if (cc >= rows) continue;
              float v0 = 0.f, v1 = 0.f;
              if (run) {
                const long at = bbd_c1_x_offset(&p, &q0, r0 + cc);
                v0 = in.v[at]; (void)in.v[at + 1]; v1 = in.v[at + 2]; (void)in.v[at + 3];
              } else {
                if (g < p.pixels) v0 = in.v[bbd_c1_x_offset(&p, &q0, r0 + cc)];
                if (g + 1 < p.pixels) v1 = in.v[bbd_c1_x_offset(&p, &q1, r0 + cc)];
              }
              const int at = bbd_c1_lds_index(cc, 2 * pr);
              CHECK(at % 2 == 0, "forward: LDS store of 8 bytes at word %d", at);
              tile[at] = v0; tile[at + 1] = v1;
              round_of[at] = round_of[at + 1] = round;
            }
          } else {
            const int qd = t & 15, g = g0 + 4 * qd;
            bbd_c1_pixel qs[4];
            for (int j = 0; j < 4; ++j) qs[j] = bbd_c1_decode(&p, g + j < p.pixels ? g + j : 0);
            const bool run = bbd_c1_y_run(&p, g, &qs[0]);
            for (int i = 0; i < BBD_C1_RC * 16 / threads; ++i) {
              const int kk = (t >> 4) + i * (threads / 16);
              if (kk >= rows) continue;
              float v[4] = {0.f, 0.f, 0.f, 0.f};
              if (run) {
                const long at = bbd_c1_y_offset(&p, &qs[0], r0 + kk);
                for (int j = 0; j < 4; ++j) v[j] = in.v[at + j];
              } else {
                for (int j = 0; j < 4; ++j)
                  if (g + j < p.pixels) v[j] = in.v[bbd_c1_y_offset(&p, &qs[j], r0 + kk)];
              }
              const int at = bbd_c1_lds_index(kk, 4 * qd);
              CHECK(at % 4 == 0, "data gradient: LDS store of 16 bytes at word %d", at);
              for (int j = 0; j < 4; ++j) { tile[at + j] = v[j]; round_of[at + j] = round; }
            }
          }
        }
        for (int wave = 0; wave < BBD_C1_WAVES; ++wave) {
          const int mb = by * BBD_C1_WAVES + wave;
          if (mb * 16 >= M) continue;
          for (int s = 0; s < rows; s += 16)
            for (int j = 0; j < 4; ++j) {
              float a[64];
              for (int lane = 0; lane < 64; ++lane) {
                if (!dgrad) {
                  const long at = bbd_c1_w_fwd(&p, mb, lane, r0, s);
                  CHECK(at % 4 == 0, "forward: weight load of 16 bytes at element %ld", at);
                  (void)w.v[at + 3];
                  a[lane] = w.v[at + j];
                } else {
                  a[lane] = w.v[bbd_c1_w_bwd(&p, mb, lane, r0, s, j)];
                }
              }
              for (int pg = 0; pg < 4; ++pg) {
                float b[64];
                for (int lane = 0; lane < 64; ++lane) {
                  const int at = bbd_c1_b_lane(lane) + bbd_c1_b_step(s, j, pg);
                  CHECK(round_of[at] == round, "LDS word %d read in round %d, written in %d", at, round, round_of[at]);
                  b[lane] = tile[at];
                }
                mfma(a, b, reinterpret_cast<float(*)[4]>(&acc[((wave * 4 + pg) * 64) * 4]));
              }
            }
        }
      }
      for (int wave = 0; wave < BBD_C1_WAVES; ++wave) {
        const int mb = by * BBD_C1_WAVES + wave;
        if (mb * 16 >= M) continue;
        for (int pg = 0; pg < 4; ++pg)
          for (int lane = 0; lane < 64; ++lane) {
            const int go = bbd_c1_out_pixel(tile_id, pg, lane);
            const bool exists = go < p.pixels;
            const bbd_c1_pixel q = bbd_c1_decode(&p, exists ? go : 0);
            const float* mine = &acc[((wave * 4 + pg) * 64 + lane) * 4];
            if (!dgrad) {
              if (!exists) continue;
              for (int reg = 0; reg < 4; ++reg) out.put(bbd_c1_y_offset(&p, &q, bbd_c1_out_channel(mb, lane, reg)), mine[reg]);
              continue;
            }
            const long plane = (long)p.H * p.W, at = bbd_c1_x_offset(&p, &q, bbd_c1_out_channel(mb, lane, 0));
            if (dgrad == 2) {
              if (exists)
                for (int reg = 0; reg < 4; ++reg) out.put(at + reg * plane, out.v[at + reg * plane] + mine[reg]);
              continue;
            }
            const int even = lane & ~1, ge = bbd_c1_out_pixel(tile_id, pg, even);
            const bbd_c1_pixel qe = bbd_c1_decode(&p, ge < p.pixels ? ge : 0);
            const bool paired = ge < p.pixels && bbd_c1_x_run(&p, ge, &qe, 2);
            const bool col1 = 2 * q.ox + 1 < p.W, row1 = 2 * q.oy + 1 < p.H;
            for (int reg = 0; reg < 4; ++reg) {
              const long o = at + reg * plane;
              if (paired) {
                if (!(lane & 1)) {
                  const float next = acc[((wave * 4 + pg) * 64 + lane + 1) * 4 + reg];
                  out.put(o, mine[reg]); out.put(o + 1, 0.f); out.put(o + 2, next); out.put(o + 3, 0.f);
                } else if (row1) {
                  for (int e = 0; e < 4; ++e) out.put(o + p.W - 2 + e, 0.f);
                }
              } else if (exists) {
                out.put(o, mine[reg]);
                if (col1) out.put(o + 1, 0.f);
                if (row1) {
                  out.put(o + p.W, 0.f);
                  if (col1) out.put(o + p.W + 1, 0.f);
                }
              }
            }
          }
      }
      delete[] tile;
    }
}

void walk_wgrad(const bbd_c1_plan& p, const Buf& x, const Buf& dy, Buf& dw, long* scratch_doubles) {
  const long doubles = bbd_c1_plan_scratch_doubles(&p);
  *scratch_doubles = doubles;
  double* scratch = new double[doubles];
  std::vector<int> written(doubles, 0);
  for (int split = 0; split < p.splits; ++split)
    for (int block = 0; block < p.kblocks * p.cblocks; ++block)
      for (int wave = 0; wave < BBD_C1_WAVES; ++wave) {
        int kb[2], cb[2], kl[2], cl[2];
        for (int i = 0; i < 2; ++i) {
          kb[i] = bbd_c1_wave_block(&p, block, wave, 0, i);
          cb[i] = bbd_c1_wave_block(&p, block, wave, 1, i);
          kl[i] = kb[i] * 16 < p.K ? kb[i] : 0;
          cl[i] = cb[i] * 16 < p.C ? cb[i] : 0;
        }
        float acc[2][2][64][4] = {};
        double total[2][2][64][4] = {};
        int first, last, in_run = 0;
        bbd_c1_split_range(&p, split, &first, &last);
        CHECK(first <= last && last <= p.strips, "split %d: strips %d .. %d of %d", split, first, last, p.strips);
        for (int st = first; st < last; ++st) {
          float a[2][4][64], b[2][4][64];
          for (int lane = 0; lane < 64; ++lane) {
            const int g = bbd_c1_strip_pixel(st, lane), ch = lane & 15;
            bbd_c1_pixel qs[4];
            bool has[4];
            for (int j = 0; j < 4; ++j) {
              has[j] = g + j < p.pixels;
              qs[j] = bbd_c1_decode(&p, has[j] ? g + j : 0);
            }
            const bool yrun = bbd_c1_y_run(&p, g, &qs[0]), xrun = bbd_c1_x_run(&p, g, &qs[0], 4);
            for (int i = 0; i < 2; ++i)
              for (int j = 0; j < 4; ++j) {
                if (yrun) a[i][j][lane] = dy.v[bbd_c1_y_offset(&p, &qs[0], kl[i] * 16 + ch) + j];
                else a[i][j][lane] = has[j] ? dy.v[bbd_c1_y_offset(&p, &qs[j], kl[i] * 16 + ch)] : 0.f;
                if (xrun) {
                  const long at = bbd_c1_x_offset(&p, &qs[0], cl[i] * 16 + ch);
                  (void)x.v[at + 7];
                  b[i][j][lane] = x.v[at + 2 * j];
                } else {
                  b[i][j][lane] = has[j] ? x.v[bbd_c1_x_offset(&p, &qs[j], cl[i] * 16 + ch)] : 0.f;
                }
              }
          }
          for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 2; ++i)
              for (int i2 = 0; i2 < 2; ++i2) mfma(a[i][j], b[i2][j], acc[i][i2]);
          if (++in_run == BBD_C1_RUN_STRIPS || st + 1 == last) {
            in_run = 0;
            for (int i = 0; i < 2; ++i)
              for (int i2 = 0; i2 < 2; ++i2)
                for (int lane = 0; lane < 64; ++lane)
                  for (int reg = 0; reg < 4; ++reg) {
                    total[i][i2][lane][reg] += (double)acc[i][i2][lane][reg];
                    acc[i][i2][lane][reg] = 0.f;
                  }
          }
        }
        for (int i = 0; i < 2; ++i)
          for (int i2 = 0; i2 < 2; ++i2) {
            if (kb[i] * 16 >= p.K || cb[i2] * 16 >= p.C) continue;
            for (int lane = 0; lane < 64; ++lane)
              for (int reg = 0; reg < 4; ++reg) {
                const long at = bbd_c1_record_index(&p, split, kb[i], cb[i2], lane, reg);
                scratch[at] = total[i][i2][lane][reg];
                ++written[at];
              }
          }
      }
  for (long at = 0; at < doubles; ++at) CHECK(written[at] == 1, "scratch double %ld written %d times", at, written[at]);
  const long record = (long)p.K * p.C;
  CHECK(record % BBD_C1_FINAL_E == 0, "K * C = %ld is no multiple of the final launch's %d", record, BBD_C1_FINAL_E);
  for (long blk = 0; blk < record / BBD_C1_FINAL_E; ++blk) {
    double part[BBD_C1_FINAL_G][BBD_C1_FINAL_E];
    for (int t = 0; t < BBD_C1_FINAL_E * BBD_C1_FINAL_G; ++t) {
      const int e16 = t & (BBD_C1_FINAL_E - 1), slice = t / BBD_C1_FINAL_E;
      double v = 0.0;
      for (int z = slice; z < p.splits; z += BBD_C1_FINAL_G) v += scratch[z * record + blk * BBD_C1_FINAL_E + e16];
      part[slice][e16] = v;
    }
    for (int e16 = 0; e16 < BBD_C1_FINAL_E; ++e16) {
      double sum = 0.0;
      for (int s = 0; s < BBD_C1_FINAL_G; ++s) sum += part[s][e16];
      dw.put(blk * BBD_C1_FINAL_E + e16, (float)sum);
    }
  }
  delete[] scratch;
}

int one_shape(int N, int C, int K, int H, int W) {
  bbd_c1_plan p;
  if (!bbd_c1_make_plan(N, C, K, H, W, &p)) {
    std::printf("%d %d %d %d %d: refused\n", N, C, K, H, W);
    return 1;
  }
  const int before = failures;
  const long nx = (long)N * C * H * W, ny = (long)N * K * p.P, nw = (long)K * C;
  Buf x(nx), w(nw), y(ny), dy(ny), dx(nx), dxa(nx), dw(nw);
  for (long i = 0; i < nx; ++i) x.v[i] = (float)small(i, 7, 3);
  for (long i = 0; i < nw; ++i) w.v[i] = (float)small(i + 11, 5, 2);
  for (long i = 0; i < ny; ++i) dy.v[i] = (float)small(i + 5, 7, 3);
  for (long i = 0; i < nx; ++i) dxa.v[i] = (float)small(i + 3, 9, 4);
  std::vector<float> before_acc(dxa.v, dxa.v + nx);

  walk_gemm(p, 0, x, w, y);
  walk_gemm(p, 1, dy, w, dx);
  walk_gemm(p, 2, dy, w, dxa);
  long doubles = 0;
  walk_wgrad(p, x, dy, dw, &doubles);

  long compared = 0;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k)
      for (int pp = 0; pp < p.P; ++pp) {
        const int oy = pp / p.Wo, ox = pp % p.Wo;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += w.v[(long)k * C + c] * x.v[(((long)n * C + c) * H + 2 * oy) * W + 2 * ox];
        const long at = ((long)n * K + k) * p.P + pp;
        CHECK(y.writes[at] == 1 && y.v[at] == s, "y[%ld] written %d times, %g against %g", at, y.writes[at], y.v[at], s);
        ++compared;
      }
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int iy = 0; iy < H; ++iy)
        for (int ix = 0; ix < W; ++ix) {
          const long at = (((long)n * C + c) * H + iy) * W + ix;
          const bool even = !(iy & 1) && !(ix & 1);
          float s = 0.f;
          if (even)
            for (int k = 0; k < K; ++k) s += w.v[(long)k * C + c] * dy.v[((long)n * K + k) * p.P + (iy / 2) * p.Wo + ix / 2];
          CHECK(dx.writes[at] == 1 && dx.v[at] == s, "dx[%ld] written %d times, %g against %g", at, dx.writes[at], dx.v[at], s);
          CHECK(dxa.writes[at] == (even ? 1 : 0) && dxa.v[at] == before_acc[at] + s, "accumulate: dx[%ld] written %d times, %g",
                at, dxa.writes[at], dxa.v[at]);
          compared += 2;
        }
  for (int k = 0; k < K; ++k)
    for (int c = 0; c < C; ++c) {
      double s = 0.0;
      for (int n = 0; n < N; ++n)
        for (int pp = 0; pp < p.P; ++pp)
          s += (double)dy.v[((long)n * K + k) * p.P + pp] * x.v[(((long)n * C + c) * H + 2 * (pp / p.Wo)) * W + 2 * (pp % p.Wo)];
      const long at = (long)k * C + c;
      CHECK(dw.writes[at] == 1 && dw.v[at] == (float)s, "dw[%ld] written %d times, %g against %g", at, dw.writes[at], dw.v[at], s);
      ++compared;
    }
  const bool ok = failures == before;
  std::printf("%d %d %d %d %d: %d tiles, %d strips, %d splits of %d, %ld scratch doubles, %ld values compared: %s\n", N, C, K,
              H, W, p.tiles, p.strips, p.splits, p.per, doubles, compared, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5) {
    std::fprintf(stderr, "usage: %s N C K H W [N C K H W ...]\n", argv[0]);
    return 2;
  }
  int bad = 0;
  for (int i = 1; i + 4 < argc; i += 5)
    bad += one_shape(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4]));
  return bad ? 1 : 0;
}
