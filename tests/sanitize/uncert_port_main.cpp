// Stand-alone driver of the uncertainty host port (tests/host_port/bbd_uncert_port.cpp) for a sanitizer build:
//
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 \
//       tests/sanitize/uncert_port_main.cpp tests/host_port/bbd_uncert_port.cpp -o uncert_port_main
//   ./uncert_port_main case.bin out.bin
//
// case.bin (little endian, written by tests/test_uncert_sanitize.py): int32 {n, h, w, K, flags, gt elements}, float64
// {min_depth, max_depth, scale_factor}, then pred float32 [n,h,w], uncert float32 [n,h,w], gt float32 [elements], desc
// int32 [n,8], rows float32 [n,12].  out.bin receives the float64 [n, 8 + 6 (K + 1)] rows.  Every buffer is a heap
// allocation of exactly its size, so a read or write past one is a report.  Nothing here is loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/bbd_hip.h"

extern "C" int hp_sparsification(const float* pred, const float* uncert, const float* gt, const int32_t* desc,
                                 const float* rows, double* out, void* scratch, long scratch_bytes, int n, int h, int w,
                                 int intervals, double min_depth, double max_depth, double scale_factor, int flags);
extern "C" int hp_post_process_uncert(const float* disp, float* out, float* uncert, int n, int h, int w);

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "short case file\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const std::vector<int32_t> head = take<int32_t>(f, 6);
  const std::vector<double> range = take<double>(f, 3);
  const int n = head[0], h = head[1], w = head[2], K = head[3], flags = head[4];
  const size_t plane = (size_t)n * h * w;
  const std::vector<float> pred = take<float>(f, plane), uncert = take<float>(f, plane), gt = take<float>(f, (size_t)head[5]);
  const std::vector<int32_t> desc = take<int32_t>(f, (size_t)n * BBD_EVAL_DESC);
  const std::vector<float> rows = take<float>(f, (size_t)n * BBD_EVAL_OUT);
  fclose(f);
  long pixels = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* d = desc.data() + (size_t)i * BBD_EVAL_DESC;
    const long r = (d[5] < d[2] ? d[5] : d[2]) - (d[4] > 0 ? d[4] : 0), c = (d[7] < d[3] ? d[7] : d[3]) - (d[6] > 0 ? d[6] : 0);
    pixels += (r > 0 && c > 0) ? r * c : 0;
  }
  const long bytes = BBD_SPARS_SCRATCH_CALL + (long)n * BBD_SPARS_SCRATCH_IMAGE + pixels * BBD_SPARS_SCRATCH_PIXEL;
  std::vector<double> scratch((size_t)(bytes + 7) / 8), out((size_t)n * (BBD_SPARS_SUMMARY + 6 * (K + 1)));
  int rc = hp_sparsification(pred.data(), uncert.data(), gt.data(), desc.data(), rows.data(), out.data(), scratch.data(),
                             bytes, n, h, w, K, range[0], range[1], range[2], flags);
  if (rc) { fprintf(stderr, "hp_sparsification: %d\n", rc); return 1; }
  if (n % 2 == 0) {                              // the flip pass on the same planes: n / 2 images and their twins
    std::vector<float> blend(plane / 2), u(plane / 2);
    rc = hp_post_process_uncert(pred.data(), blend.data(), u.data(), n / 2, h, w);
    if (rc) { fprintf(stderr, "hp_post_process_uncert: %d\n", rc); return 1; }
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { perror(argv[2]); return 2; }
  fclose(f);
  return 0;
}
