// Host port of bbd_geo.hip for the CPU test tier: the argument rules, what a sample is, its derivatives, the fixed
// points and the order of the float64 sums are bbd_geo_math.h, shared with the kernels; the launches are serial loops
// here, the 256 lanes of a work item an array, the wave sums bbd_geo_tree64 and the atomics plain integer additions.
// The C signatures of bbd_geo_fwd / bbd_geo_bwd minus `stream`.
#include <cstdint>
#include <cstring>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_geo_math.h"

extern "C" int hp_geo_fwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                          double* pair_sum, int64_t* pair_count, float* err, uint8_t* code, int64_t* scratch,
                          long scratch_words, int B, int H, int W, int V) {
  const int rc = bbd_geo_fwd_status(q_tgt, q_src, T, K, inv_K, pair_sum, pair_count, scratch, scratch_words, B, H, W, V);
  if (rc) return rc;
  const int plane = H * W;
  const long items = bbd_geo_items(H, W);
  for (int b = 0; b < B; ++b) {
    BbdGeoCamera cam;
    bbd_geo_camera(K, inv_K, b, &cam);
    for (long it = 0; it < items; ++it)
      for (int v = 0; v < V; ++v) {
        const size_t pair = (size_t)v * B + b;
        const float* src = q_src + pair * plane;
        int64_t sum = 0, count = 0;
        for (long k = it * BBD_GEO_RUN; k < (it + 1) * BBD_GEO_RUN && k < plane; ++k) {
          const int y = (int)(k / W), x = (int)(k - (long)y * W);
          float p[3];
          BbdGeoSample s;
          const int vis = bbd_geo_point(&cam, q_tgt[(size_t)b * plane + k], x, y, p) &&
                          bbd_geo_sample(&cam, p, T + pair * 12, src, H, W, &s);
          if (err) err[pair * plane + k] = vis ? s.e : 0.0f;
          if (code) code[pair * plane + k] = (uint8_t)(vis ? bbd_geo_code(&s) : 0);
          if (vis) {
            sum += bbd_geo_fixed(s.e, BBD_GEO_SUM_ONE);
            count += 1;
          }
        }
        int64_t* slot = scratch + (((size_t)b * items + it) * V + v) * 2;
        slot[0] = sum;
        slot[1] = count;
      }
  }
  for (int v = 0; v < V; ++v)
    for (int b = 0; b < B; ++b) {
      int64_t sum = 0, count = 0;
      for (long it = 0; it < items; ++it) {
        const int64_t* slot = scratch + (((size_t)b * items + it) * V + v) * 2;
        sum += slot[0];
        count += slot[1];
      }
      pair_sum[(size_t)v * B + b] = bbd_geo_pair_sum(sum);
      pair_count[(size_t)v * B + b] = count;
    }
  return 0;
}

extern "C" int hp_geo_bwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                          const double* g, float* grad_q_tgt, float* grad_q_src, float* grad_T, int64_t* scratch,
                          long scratch_words, int B, int H, int W, int V) {
  const int rc = bbd_geo_bwd_status(q_tgt, q_src, T, K, inv_K, g, grad_q_tgt, grad_q_src, grad_T, scratch, scratch_words,
                                    B, H, W, V);
  if (rc) return rc;
  const int plane = H * W;
  const long items = bbd_geo_items(H, W), n = (long)V * B * plane;
  int64_t* taps = scratch;
  double* slots = reinterpret_cast<double*>(scratch + n);
  memset(taps, 0, (size_t)n * 8);
  static thread_local double lanes[12][BBD_GEO_LANES];
  for (int b = 0; b < B; ++b) {
    BbdGeoCamera cam;
    bbd_geo_camera(K, inv_K, b, &cam);
    for (long it = 0; it < items; ++it) {
      double gq[BBD_GEO_RUN];
      for (int i = 0; i < BBD_GEO_RUN; ++i) gq[i] = 0.0;
      for (int v = 0; v < V; ++v) {
        const size_t pair = (size_t)v * B + b;
        const float* Tp = T + pair * 12;
        const float* src = q_src + pair * plane;
        int64_t* dst = taps + pair * plane;
        const double up = g[pair];
        memset(lanes, 0, sizeof(lanes));
        for (int pass = 0; pass < BBD_GEO_PASSES; ++pass)          // a lane adds its pixels in pass order
          for (int lane = 0; lane < BBD_GEO_LANES; ++lane) {
            const int i = pass * BBD_GEO_LANES + lane;
            const long k = it * BBD_GEO_RUN + i;
            if (k >= plane) continue;
            const int y = (int)(k / W), x = (int)(k - (long)y * W);
            const float q = q_tgt[(size_t)b * plane + k];
            float p[3];
            BbdGeoSample s;
            if (!(bbd_geo_point(&cam, q, x, y, p) && bbd_geo_sample(&cam, p, Tp, src, H, W, &s))) continue;
            BbdGeoGrad d;
            bbd_geo_sample_grad(&cam, p, q, Tp, &s, &d);
            int64_t* r0 = dst + (size_t)s.y0 * W + s.x0;
            r0[0] += bbd_geo_fixed(d.tap[0], BBD_GEO_TAP_ONE);
            r0[1] += bbd_geo_fixed(d.tap[1], BBD_GEO_TAP_ONE);
            r0[W] += bbd_geo_fixed(d.tap[2], BBD_GEO_TAP_ONE);
            r0[W + 1] += bbd_geo_fixed(d.tap[3], BBD_GEO_TAP_ONE);
            gq[i] += up * (double)d.gq;
            double acc[12];
            for (int e = 0; e < 12; ++e) acc[e] = lanes[e][lane];
            bbd_geo_pose_add(p, &d, acc);
            for (int e = 0; e < 12; ++e) lanes[e][lane] = acc[e];
          }
        for (int e = 0; e < 12; ++e) {
          double t = bbd_geo_tree64(lanes[e]);
          for (int wv = 1; wv < BBD_GEO_LANES / 64; ++wv) t += bbd_geo_tree64(lanes[e] + 64 * wv);
          slots[(((size_t)b * items + it) * V + v) * 12 + e] = t;
        }
      }
      for (int i = 0; i < BBD_GEO_RUN; ++i) {
        const long k = it * BBD_GEO_RUN + i;
        if (k < plane) grad_q_tgt[(size_t)b * plane + k] = (float)gq[i];
      }
    }
  }
  for (long i = 0; i < n; ++i) grad_q_src[i] = bbd_geo_tap_value(taps[i], g[i / plane]);
  for (long pair = 0; pair < (long)V * B; ++pair) {
    const int v = (int)(pair / B), b = (int)(pair - (long)v * B);
    for (int e = 0; e < 12; ++e) {
      double t = 0.0;
      for (long it = 0; it < items; ++it) t += slots[(((size_t)b * items + it) * V + v) * 12 + e];
      grad_T[pair * 12 + e] = (float)(g[pair] * t);
    }
  }
  return 0;
}
