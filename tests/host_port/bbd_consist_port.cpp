// Host port of bbd_consist.hip for the CPU test tier: the argument rules, the transform of a pair and what a pixel
// becomes are bbd_consist_math.h, shared with the kernels; the two launches are serial loops here and the wave sums and
// atomics plain additions.  The C signature of bbd_depth_consistency minus `stream`.
#include <cstdint>
#include <cstring>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_consist_math.h"

extern "C" int hp_depth_consistency(const float* disp, const double* poses, const double* scale, const float* K,
                                    const float* inv_K, const int32_t* sources, double* transforms, uint8_t* seen,
                                    uint8_t* agree, float* err, float* filtered, int64_t* counters, int n, int h, int w,
                                    int V, double threshold, int min_views, int flags) {
  const int rc = bbd_consist_status(disp, poses, K, inv_K, sources, transforms, seen, agree, counters, n, h, w, V,
                                    threshold, min_views, flags);
  if (rc) return rc;
  BbdConsistParams a;
  a.disp = disp; a.K = K; a.inv_K = inv_K;
  a.n = n; a.h = h; a.w = w; a.V = V; a.flags = flags; a.min_views = min_views; a.threshold = threshold;
  const double s = scale ? *scale : 1.0;
  double K9[9];
  for (int e = 0; e < 9; ++e) K9[e] = (double)K[e];
  const int plane = h * w;
  for (int i = 0; i < n; ++i) {
    int src[BBD_CONSIST_MAX_VIEWS];
    double* M = transforms + (size_t)i * V * 12;
    for (int v = 0; v < V; ++v) {
      src[v] = bbd_consist_source(sources, n, V, i, v);
      bbd_consist_transform(poses, i, src[v], M + 12 * v);
    }
    int64_t* c = counters + (size_t)i * BBD_CONSIST_COUNTERS;
    memset(c, 0, BBD_CONSIST_COUNTERS * 8);
    for (int k = 0; k < plane; ++k) {
      BbdConsistPixel px;
      bbd_consist_pixel(&a, s, K9, src, M, i, k, &px);
      const size_t at = (size_t)i * plane + (size_t)k;
      seen[at] = (uint8_t)px.seen;
      agree[at] = (uint8_t)px.agree;
      if (err) memcpy(err + at, &px.err_bits, 4);
      if (filtered) filtered[at] = px.filtered;
      c[0] += px.valid; c[1] += px.seen; c[2] += px.agree; c[3] += px.err_sum; c[4] += px.kept;
    }
  }
  return 0;
}
