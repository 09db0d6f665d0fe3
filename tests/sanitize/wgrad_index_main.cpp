// Stand-alone walk of one bbd_conv3x3_wgrad call on the host, with the kernels' own index arithmetic
// (baseboostdepth_amd/csrc/bbd_wgrad_math.h) and nothing of the GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 \
//       tests/sanitize/wgrad_index_main.cpp -o wgrad_index_main
//   ./wgrad_index_main N C K H W [N C K H W ...]
//
// Every workgroup, wave, strip and lane of the launch is visited in the kernel's order.  Each offset a lane would load
// from xp / grad_z, each record element a workgroup would store to scratch and each element the final launch would read
// or write is checked against its tensor's size (and the tensors are heap allocations of exactly that size, so a miss of
// these checks is a sanitizer report); every output pixel must be taken exactly once per role, every scratch element
// written exactly once before it is read, every weight written exactly once.  The MFMA is played as what it is, an fp32
// fma chain over the 4 pixel groups of the wave, on small integers, so the result must equal the plain triple loop
// exactly: the lane maps of the operands, of the accumulator tile and of the record are all inside that comparison.
// Nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_wgrad_math.h"

static int failures = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (failures++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    }                                                                       \
  } while (0)

struct Lane { float g[4]; float x[2][3][6]; };

static int walk(int N, int C, int K, int H, int W) {
  bbd_wgrad_plan p;
  if (!bbd_wgrad_make_plan(N, C, K, H, W, BBD_WGRAD_RUN, &p)) { fprintf(stderr, "shape not supported\n"); return 1; }
  const long xp_size = (long)N * C * (H + 2) * (W + 2), gz_size = (long)N * K * H * W, gw_size = (long)K * C * 9;
  const long scratch_size = bbd_wgrad_plan_scratch_doubles(&p);
  std::vector<float> xp((size_t)xp_size), gz((size_t)gz_size), gw((size_t)gw_size, std::numeric_limits<float>::quiet_NaN());
  std::vector<double> scratch((size_t)scratch_size, std::numeric_limits<double>::quiet_NaN());
  std::vector<int> scratch_writes((size_t)scratch_size, 0), gw_writes((size_t)gw_size, 0);
  unsigned state = 12345u;
  for (auto& v : xp) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 28) - 8); }
  for (auto& v : gz) { state = state * 1664525u + 1013904223u; v = (float)((int)(state >> 29) - 4); }

  CHECK(p.run >= 1 && p.per >= 1 && p.groups >= 1 && (long)p.groups * BBD_WGRAD_WAVES * p.per >= p.strips, "plan");
  CHECK(p.roles * p.record == 9 * C * K && p.record % BBD_WGRAD_FINAL_E == 0, "record %d roles %d", p.record, p.roles);

  std::vector<int> taken((size_t)gz_size);             // per role: how often each grad_z element was multiplied
  std::vector<double> total((size_t)p.record);
  for (int role = 0; role < p.roles; ++role) {
    int kb, cb0;
    bbd_wgrad_role(&p, role, &kb, &cb0);
    CHECK(kb >= 0 && kb < K / 16 && cb0 >= 0 && cb0 + p.ncb <= C / 16, "role %d -> kb %d cb0 %d", role, kb, cb0);
    std::fill(taken.begin(), taken.end(), 0);
    for (int group = 0; group < p.groups; ++group) {
      std::fill(total.begin(), total.end(), 0.0);
      // the waves' runs end together (step i of every wave, then the widening in wave order): the order of `total`
      std::vector<std::vector<float>> accs(BBD_WGRAD_WAVES, std::vector<float>((size_t)p.record, 0.f));
      std::vector<int> products(BBD_WGRAD_WAVES, 0);
      for (int i = 0; i < p.per; ++i) {
        for (int wave = 0; wave < BBD_WGRAD_WAVES; ++wave) {
          int first, last;
          bbd_wgrad_wave_range(&p, group, wave, &first, &last);
          CHECK(first >= 0 && first <= last && last <= p.strips, "range");
          const int strip = first + i;
          if (strip >= last) continue;
          const bbd_wgrad_strip s = bbd_wgrad_decode(&p, strip);
          CHECK(s.n >= 0 && s.n < N && s.y >= 0 && s.y < H && s.x0 >= 0 && s.x0 < W, "strip %d", strip);
          if (strip > first) {                       // the kernel steps from strip to strip: the same place
            const bbd_wgrad_strip t = bbd_wgrad_next(&p, bbd_wgrad_decode(&p, strip - 1));
            CHECK(t.n == s.n && t.y == s.y && t.x0 == s.x0 && t.full == s.full, "step to strip %d", strip);
          }
          Lane lanes[64];
          int pixels[64];
          for (int lane = 0; lane < 64; ++lane) {
            Lane& f = lanes[lane];
            const int px = s.full ? 4 : bbd_wgrad_lane_pixels(&p, &s, lane);
            pixels[lane] = px;
            CHECK(!s.full || bbd_wgrad_lane_pixels(&p, &s, lane) == 4, "a full strip with a short lane");
            const long go = bbd_wgrad_gz_offset(&p, &s, kb, lane);
            CHECK(px == 0 || (go >= 0 && go + px <= gz_size), "grad_z offset %ld + %d", go, px);
            for (int j = 0; j < 4; ++j) {
              f.g[j] = j < px ? gz[(size_t)(go + j)] : 0.f;
              if (j < px) {
                taken[(size_t)(go + j)]++;
                // the element is the one the strip and lane stand for
                const long want = (((long)s.n * K + kb * 16 + (lane & 15)) * H + s.y) * W + s.x0 + 4 * (lane >> 4) + j;
                CHECK(go + j == want && s.x0 + 4 * (lane >> 4) + j < W, "grad_z element");
              }
            }
            const int cols = px ? px + 2 : 0;
            for (int cb = 0; cb < p.ncb; ++cb)
              for (int r = 0; r < 3; ++r) {
                const long xo = bbd_wgrad_xp_offset(&p, &s, cb0 + cb, r, lane);
                CHECK(cols == 0 || (xo >= 0 && xo + cols <= xp_size), "xp offset %ld + %d", xo, cols);
                const long row_end = ((((long)s.n * C + (cb0 + cb) * 16 + (lane & 15)) * (H + 2) + s.y + r) + 1) * (W + 2);
                CHECK(cols == 0 || xo + cols <= row_end, "xp access leaves its row");
                for (int c6 = 0; c6 < 6; ++c6) f.x[cb][r][c6] = c6 < cols ? xp[(size_t)(xo + c6)] : 0.f;
              }
          }
          // MFMA j: D[row][col] = fma chain over the pixel groups g = 0..3 of A[row][g] * B[g][col]
          std::vector<float>& a = accs[wave];
          for (int j = 0; j < 4; ++j)
            for (int cb = 0; cb < p.ncb; ++cb)
              for (int r = 0; r < 3; ++r)
                for (int t = 0; t < 3; ++t)
                  for (int lane = 0; lane < 64; ++lane)
                    for (int reg = 0; reg < 4; ++reg) {
                      const int row = 4 * (lane >> 4) + reg, col = lane & 15;
                      float d = a[(size_t)bbd_wgrad_record_index(cb, r, t, lane, reg)];
                      for (int g = 0; g < 4; ++g) {
                        const Lane& la = lanes[g * 16 + row];
                        const Lane& lb = lanes[g * 16 + col];
                        const float b = j < pixels[g * 16 + col] ? lb.x[cb][r][j + t] : 0.f;
                        d = fmaf(la.g[j], b, d);
                      }
                      a[(size_t)bbd_wgrad_record_index(cb, r, t, lane, reg)] = d;
                    }
          products[wave] += BBD_WGRAD_STRIP;
          CHECK(products[wave] <= BBD_WGRAD_RUN, "an accumulator with %d products", products[wave]);
        }
        if (bbd_wgrad_run_ends(&p, i)) {             // the kernel's own predicate: where its waves widen
          for (int e = 0; e < p.record; ++e)
            for (int wave = 0; wave < BBD_WGRAD_WAVES; ++wave) {
              total[(size_t)e] += (double)accs[wave][(size_t)e];
              accs[wave][(size_t)e] = 0.f;
            }
          std::fill(products.begin(), products.end(), 0);
        }
      }
      const long ro = bbd_wgrad_record_offset(&p, group, role);
      CHECK(ro >= 0 && ro + p.record <= scratch_size, "record offset %ld", ro);
      for (int e = 0; e < p.record; ++e) { scratch[(size_t)(ro + e)] = total[(size_t)e]; scratch_writes[(size_t)(ro + e)]++; }
    }
    for (long q = 0; q < gz_size; ++q) {
      const int k = (int)((q / ((long)H * W)) % K);
      CHECK(taken[(size_t)q] == (k / 16 == kb ? 1 : 0), "role %d takes grad_z[%ld] %d times", role, q, taken[(size_t)q]);
    }
  }
  for (long q = 0; q < scratch_size; ++q) CHECK(scratch_writes[(size_t)q] == 1, "scratch[%ld] written %d times", q, scratch_writes[(size_t)q]);

  // the final launch
  const int blocks = p.roles * p.record / BBD_WGRAD_FINAL_E;
  for (int b = 0; b < blocks; ++b)
    for (int e16 = 0; e16 < BBD_WGRAD_FINAL_E; ++e16) {
      const int idx = b * BBD_WGRAD_FINAL_E + e16, role = idx / p.record, e = idx - role * p.record;
      double part[BBD_WGRAD_FINAL_G];
      for (int slice = 0; slice < BBD_WGRAD_FINAL_G; ++slice) {
        double v = 0.0;
        for (int g = slice; g < p.groups; g += BBD_WGRAD_FINAL_G) {
          const long o = bbd_wgrad_record_offset(&p, g, role) + e;
          CHECK(o >= 0 && o < scratch_size, "final read %ld", o);
          v += scratch[(size_t)o];
        }
        part[slice] = v;
      }
      double sum = 0.0;
      for (int q = 0; q < BBD_WGRAD_FINAL_G; ++q) sum += part[q];
      const long o = bbd_wgrad_record_to_weight(&p, role, e);
      CHECK(o >= 0 && o < gw_size, "weight offset %ld", o);
      gw[(size_t)o] = (float)sum;
      gw_writes[(size_t)o]++;
    }
  for (long q = 0; q < gw_size; ++q) CHECK(gw_writes[(size_t)q] == 1, "grad_w[%ld] written %d times", q, gw_writes[(size_t)q]);

  // small integers: every product and every sum above is exact, so is this one
  for (int k = 0; k < K; ++k)
    for (int c = 0; c < C; ++c)
      for (int r = 0; r < 3; ++r)
        for (int t = 0; t < 3; ++t) {
          double want = 0.0;
          for (int n = 0; n < N; ++n)
            for (int y = 0; y < H; ++y)
              for (int x = 0; x < W; ++x)
                want += (double)gz[(size_t)((((long)n * K + k) * H + y) * W + x)] *
                        (double)xp[(size_t)((((long)n * C + c) * (H + 2) + y + r) * (W + 2) + x + t)];
          const float got = gw[(size_t)((((long)k * C + c) * 3 + r) * 3 + t)];
          CHECK((double)got == want, "grad_w[%d][%d][%d][%d] = %g, exact %g", k, c, r, t, (double)got, want);
        }
  printf("N%d C%d K%d H%d W%d: %d roles x %d groups, %d strips per wave, %ld scratch doubles: %s\n", N, C, K, H, W, p.roles,
         p.groups, p.per, scratch_size, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5) { fprintf(stderr, "usage: %s N C K H W [N C K H W ...]\n", argv[0]); return 2; }
  for (int a = 1; a + 4 < argc; a += 5)
    if (walk(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), atoi(argv[a + 4]))) return 1;
  return 0;
}
