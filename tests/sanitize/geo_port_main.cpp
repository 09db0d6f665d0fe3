// The geometry-consistency host port (tests/host_port/geo.cpp) as a stand-alone program, for a build with
// -fsanitize=address,undefined (tests/test_geo_port.py).  Nothing here is loaded into Python.
//   geo_port_main case.bin out.bin
// case.bin: int32 B, H, W, V; float32 q_tgt [B,H,W], q_src [V,B,H,W], T [V,B,12], K [B,16], inv_K [B,16]; float64 g [V,B].
// out.bin:  pair_sum f64 [V,B], pair_count i64 [V,B], err f32 [V,B,H,W], code u8 [V,B,H,W], grad_q_tgt f32 [B,H,W],
//           grad_q_src f32 [V,B,H,W], grad_T f32 [V,B,12].  Every buffer has exactly the size the header states.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../baseboostdepth_amd/csrc/bbd_geo_math.h"

extern "C" int hp_geo_fwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                          double* pair_sum, int64_t* pair_count, float* err, uint8_t* code, int64_t* scratch,
                          long scratch_words, int B, int H, int W, int V);
extern "C" int hp_geo_bwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                          const double* g, float* grad_q_tgt, float* grad_q_src, float* grad_T, int64_t* scratch,
                          long scratch_words, int B, int H, int W, int V);

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<int32_t> dims(4);
  if (!get(in, dims)) return 4;
  const int B = dims[0], H = dims[1], W = dims[2], V = dims[3];
  if (bbd_geo_shape_status(B, H, W, V)) return 5;
  const size_t plane = (size_t)H * W, pairs = (size_t)V * B;
  std::vector<float> q_tgt(B * plane), q_src(pairs * plane), T(pairs * 12), K((size_t)B * 16), inv_K((size_t)B * 16);
  std::vector<double> g(pairs);
  if (!(get(in, q_tgt) && get(in, q_src) && get(in, T) && get(in, K) && get(in, inv_K) && get(in, g))) return 6;
  fclose(in);
  std::vector<double> pair_sum(pairs);
  std::vector<int64_t> pair_count(pairs);
  std::vector<float> err(pairs * plane), grad_q_tgt(B * plane), grad_q_src(pairs * plane), grad_T(pairs * 12);
  std::vector<uint8_t> code(pairs * plane);
  const long fw = bbd_geo_fwd_words(B, H, W, V), bw = bbd_geo_bwd_words(B, H, W, V);
  std::vector<int64_t> fwd_scratch(fw), bwd_scratch(bw);
  if (hp_geo_fwd(q_tgt.data(), q_src.data(), T.data(), K.data(), inv_K.data(), pair_sum.data(), pair_count.data(),
                 err.data(), code.data(), fwd_scratch.data(), fw, B, H, W, V))
    return 7;
  if (hp_geo_bwd(q_tgt.data(), q_src.data(), T.data(), K.data(), inv_K.data(), g.data(), grad_q_tgt.data(),
                 grad_q_src.data(), grad_T.data(), bwd_scratch.data(), bw, B, H, W, V))
    return 8;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 9;
  const bool ok = put(out, pair_sum) && put(out, pair_count) && put(out, err) && put(out, code) && put(out, grad_q_tgt) &&
                  put(out, grad_q_src) && put(out, grad_T);
  return fclose(out) == 0 && ok ? 0 : 10;
}
