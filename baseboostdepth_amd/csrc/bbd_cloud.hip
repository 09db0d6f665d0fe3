// bbd_cloud.hip - coloured point clouds of a ragged batch of predictions (or of their ground truth), compacted on the
// device into 16-byte vertices that a binary PLY file takes as they are (pointcloud.py).
//
// What a vertex is - the depth of a candidate pixel, whether it is kept, its back-projection and its colour - is
// bbd_cloud_math.h, shared with the host port.  What is here is the compaction: the kept candidates of image i go,
// in raster order and without gaps, to the start of the image's region.
//
//   count  cloud_count_kernel  (chunks, image): a chunk is BBD_CLOUD_CHUNK = 256 consecutive candidates, one per lane of
//                              four waves; kept lanes are counted with the 64-bit __ballot mask and a population count,
//                              the four wave counts are added, the chunk's total goes to the chunk table
//   scan   cloud_scan_kernel   one workgroup per image: exclusive prefix sum of the image's chunk totals, in place
//                              (a lane owns a contiguous run of the table, runs are combined with a shuffle scan in the
//                              wave and a serial sum over the 16 waves); counts[i] = the total
//   write  cloud_write_kernel  (chunks, image): the same lanes evaluate the same candidates again; a kept lane's slot is
//                              chunk prefix + kept lanes of the waves before it + population count of the ballot bits
//                              below its own; the vertex is ONE 16-byte store
//
// Integer sums only: nothing depends on launch geometry (every kernel strides over its work with the grid it was given)
// or on scheduling, and there are no atomics.  The depth is evaluated twice rather than kept between the passes: it
// costs four reads of a prediction that sits in cache, keeping it would cost 4 B written and read per candidate.
// No allocation, no host synchronisation; the chunk table is the caller's scratch and needs no initialisation.
// The ballots, the scan and the slot of a kept lane are bbd_compact.h, which bbd_map.hip shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_cloud_math.h"
#include "bbd_compact.h"
#include "bbd_device_util.h"

namespace {

constexpr int CT = BBD_CLOUD_CHUNK;   // threads of the count and write kernels: one candidate each
constexpr int CW = CT / 64;
constexpr int ST = 1024;              // threads of the scan kernel
constexpr int SW = ST / 64;
constexpr long MAX_GRID_X = 4096;     // chunks beyond this are reached by striding

struct CloudCall {
  BbdCloudParams p;
  int32_t* chunks;       // [n, chunk_stride]
  int32_t* counts;       // [n]
  uint4* vertices;
  int chunk_stride;
};

__global__ __launch_bounds__(CT) void cloud_count_kernel(CloudCall a) {
  __shared__ int wave_kept[CW];
  const int img = blockIdx.y, tid = threadIdx.x;
  const BbdCloudImg m = bbd_cloud_img(a.p.desc, img, a.p.stride, a.p.max_h, a.p.max_w);
  const int n_chunks = (m.cap + CT - 1) / CT;                      // <= chunk_stride: cap <= the largest grid
  int32_t* table = a.chunks + (size_t)img * a.chunk_stride;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {      // uniform over the workgroup
    const int c = chunk * CT + tid;
    int pixel;
    float d;
    const bool keep = c < m.cap && bbd_cloud_depth(&a.p, &m, img, c, &pixel, &d);
    compact_ballot(keep, wave_kept);
    __syncthreads();
    if (tid == 0) table[chunk] = compact_total<CW>(wave_kept);
    __syncthreads();
  }
}

__global__ __launch_bounds__(ST) void cloud_scan_kernel(CloudCall a) {
  __shared__ int wave_total[SW];
  const int img = blockIdx.x;
  const BbdCloudImg m = bbd_cloud_img(a.p.desc, img, a.p.stride, a.p.max_h, a.p.max_w);
  compact_scan<ST>(a.chunks + (size_t)img * a.chunk_stride, (m.cap + CT - 1) / CT, wave_total, a.counts + img);
}

__global__ __launch_bounds__(CT) void cloud_write_kernel(CloudCall a) {
  __shared__ int wave_kept[CW];
  const int img = blockIdx.y, tid = threadIdx.x;
  const BbdCloudImg m = bbd_cloud_img(a.p.desc, img, a.p.stride, a.p.max_h, a.p.max_w);
  const int n_chunks = (m.cap + CT - 1) / CT;
  const int32_t* table = a.chunks + (size_t)img * a.chunk_stride;
  uint4* out = a.vertices + m.out;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int c = chunk * CT + tid;
    int pixel = 0;
    float d = 0.0f;
    const bool keep = c < m.cap && bbd_cloud_depth(&a.p, &m, img, c, &pixel, &d);
    const unsigned long long mask = compact_ballot(keep, wave_kept);
    __syncthreads();
    if (keep) {
      const int slot = compact_slot(table[chunk], mask, wave_kept);  // < counts[i] <= cap
      uint32_t v[4];
      bbd_cloud_vertex(&a.p, &m, img, pixel, d, v);
      out[slot] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int bbd_point_cloud_scratch_ints(int n, int max_h, int max_w, int stride) {
  if (n < 1 || max_h < 1 || max_w < 1 || stride < 1) return BBD_E_BADARG;
  if ((long)max_h * (long)max_w > BBD_CLOUD_MAX_PIXELS) return BBD_E_TOOMANY;
  const long ints = (long)n * bbd_cloud_chunk_stride(max_h, max_w, stride);
  return ints > 0x7fffffffL ? BBD_E_TOOMANY : (int)ints;
}

extern "C" int bbd_point_cloud(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                               const float* inv_K, const uint8_t* rgb, const uint8_t* lut, void* vertices,
                               int32_t* counts, int32_t* scratch, int scratch_ints, int n, int h, int w, int max_h,
                               int max_w, int stride, double min_depth, double max_depth, double clamp_lo,
                               double clamp_hi, double scale_factor, int flags, void* stream) {
  const int rc = bbd_cloud_args_status(pred, gt, desc, inv_K, rgb, lut, vertices, counts, scratch, n, h, w, max_h,
                                       max_w, stride, flags);
  if (rc) return rc;
  const long chunk_stride = bbd_cloud_chunk_stride(max_h, max_w, stride);
  if ((long)scratch_ints < (long)n * chunk_stride) return BBD_E_BADARG;
  CloudCall a;
  a.p.pred = pred; a.p.gt = gt; a.p.desc = desc; a.p.rows = rows; a.p.inv_K = inv_K; a.p.rgb = rgb; a.p.lut = lut;
  a.p.h = h; a.p.w = w; a.p.max_h = max_h; a.p.max_w = max_w; a.p.stride = stride; a.p.flags = flags;
  a.p.lo = (float)min_depth; a.p.hi = (float)max_depth; a.p.clamp_lo = (float)clamp_lo; a.p.clamp_hi = (float)clamp_hi;
  a.p.scale_factor = (float)scale_factor;
  a.chunks = scratch; a.counts = counts; a.vertices = static_cast<uint4*>(vertices); a.chunk_stride = (int)chunk_stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(chunk_stride < MAX_GRID_X ? chunk_stride : MAX_GRID_X), (unsigned)n);
  hipLaunchKernelGGL(cloud_count_kernel, grid, dim3(CT), 0, st, a);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)n), dim3(ST), 0, st, a);
  hipLaunchKernelGGL(cloud_write_kernel, grid, dim3(CT), 0, st, a);
  return launch_status();
}
