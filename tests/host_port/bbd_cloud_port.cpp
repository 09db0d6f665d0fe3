// Host port of bbd_cloud.hip for the CPU test tier: the argument rules, the candidate grid, the depth / keep rule and
// the vertex are bbd_cloud_math.h, shared with the kernels; what the three launches compute - per image, the kept
// candidates in raster order from the start of the region, and their number - is a serial loop here.  Same C
// signatures as the bbd_point_cloud* entries minus `stream`.
#include <cstdint>
#include <cstring>

#include "../../include/bbd_hip.h"
#include "../../baseboostdepth_amd/csrc/bbd_cloud_math.h"

extern "C" int hp_point_cloud_scratch_ints(int n, int max_h, int max_w, int stride) {
  if (n < 1 || max_h < 1 || max_w < 1 || stride < 1) return BBD_E_BADARG;
  if ((long)max_h * (long)max_w > BBD_CLOUD_MAX_PIXELS) return BBD_E_TOOMANY;
  const long ints = (long)n * bbd_cloud_chunk_stride(max_h, max_w, stride);
  return ints > 0x7fffffffL ? BBD_E_TOOMANY : (int)ints;
}

extern "C" int hp_point_cloud(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                              const float* inv_K, const uint8_t* rgb, const uint8_t* lut, void* vertices,
                              int32_t* counts, int32_t* scratch, int scratch_ints, int n, int h, int w, int max_h,
                              int max_w, int stride, double min_depth, double max_depth, double clamp_lo,
                              double clamp_hi, double scale_factor, int flags) {
  const int rc = bbd_cloud_args_status(pred, gt, desc, inv_K, rgb, lut, vertices, counts, scratch, n, h, w, max_h,
                                       max_w, stride, flags);
  if (rc) return rc;
  if ((long)scratch_ints < (long)n * bbd_cloud_chunk_stride(max_h, max_w, stride)) return BBD_E_BADARG;
  BbdCloudParams a;
  a.pred = pred; a.gt = gt; a.desc = desc; a.rows = rows; a.inv_K = inv_K; a.rgb = rgb; a.lut = lut;
  a.h = h; a.w = w; a.max_h = max_h; a.max_w = max_w; a.stride = stride; a.flags = flags;
  a.lo = (float)min_depth; a.hi = (float)max_depth; a.clamp_lo = (float)clamp_lo; a.clamp_hi = (float)clamp_hi;
  a.scale_factor = (float)scale_factor;
  for (int i = 0; i < n; ++i) {
    const BbdCloudImg m = bbd_cloud_img(desc, i, stride, max_h, max_w);
    uint8_t* out = static_cast<uint8_t*>(vertices) + m.out * BBD_CLOUD_VERTEX;
    int kept = 0;
    for (int c = 0; c < m.cap; ++c) {
      int pixel;
      float d;
      if (!bbd_cloud_depth(&a, &m, i, c, &pixel, &d)) continue;
      uint32_t v[4];
      bbd_cloud_vertex(&a, &m, i, pixel, d, v);
      memcpy(out + (size_t)kept * BBD_CLOUD_VERTEX, v, BBD_CLOUD_VERTEX);
      ++kept;
    }
    counts[i] = kept;
  }
  return 0;
}
