// The stereo-matcher host port (tests/host_port/sgm.cpp) as a stand-alone program, for a build with
// -fsanitize=address,undefined (tests/test_sgm_port.py).  Nothing here is loaded into Python.
//   sgm_port_main case.bin out.bin
// case.bin: int32 B, H, W, D, paths, p1, p2, uniqueness, fill; float32 left [B,3,H,W], right [B,3,H,W]; int32 side [B].
// out.bin:  disp16 i16 [B,H,W], valid_count i64 [B].  Every buffer has exactly the size the header states.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../baseboostdepth_amd/csrc/bbd_sgm_math.h"

extern "C" int hp_sgm_hints(const float* left, const float* right, const int32_t* side, int16_t* disp16,
                            int64_t* valid_count, void* scratch, long scratch_bytes, int B, int H, int W, int D,
                            int paths, int p1, int p2, int uniqueness, int fill);

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<int32_t> dims(9);
  if (!get(in, dims)) return 4;
  const int B = dims[0], H = dims[1], W = dims[2], D = dims[3], paths = dims[4];
  const long bytes = bbd_sgm_bytes(B, H, W, D, paths);
  if (bytes <= 0) return 5;
  const size_t plane = (size_t)H * W;
  std::vector<float> left(B * 3 * plane), right(B * 3 * plane);
  std::vector<int32_t> side(B);
  if (!(get(in, left) && get(in, right) && get(in, side))) return 6;
  fclose(in);
  std::vector<int16_t> disp16(B * plane);
  std::vector<int64_t> valid_count(B);
  std::vector<uint64_t> scratch((size_t)bytes / 8);               // 8-byte aligned; the formula is a multiple of 8
  if ((long)scratch.size() * 8 != bytes) return 7;
  if (hp_sgm_hints(left.data(), right.data(), side.data(), disp16.data(), valid_count.data(), scratch.data(), bytes, B, H,
                   W, D, paths, dims[5], dims[6], dims[7], dims[8]))
    return 8;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 9;
  const bool ok = put(out, disp16) && put(out, valid_count);
  return fclose(out) == 0 && ok ? 0 : 10;
}
