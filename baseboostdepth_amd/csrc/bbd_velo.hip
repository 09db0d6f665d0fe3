// bbd_velo.hip - ground-truth depth maps from Velodyne scans on the device (kitti_utils.py:46-98, the
// generate_depth_map behind export_gt_depth.py), a ragged batch of frames per call.
//
// The reference projects a scan with numpy, scatters the depths into the image ("last point wins"), then walks a
// Counter over sub2ind keys in Python and gives the pixel of each duplicated key's first point the minimum depth of
// that key - about 0.05 s per frame on the host.  Here the same result is four order-independent reductions:
//
//   point sweep  (chunk, frame) grid: every point is projected in fp64 (bbd_velo_math.h) and, when it lands in the
//                image, updates with integer vector atomics in global scratch
//                  last[pixel]  = max point index + 1            -> the value the scatter leaves
//                  first[key]   = max ~point index               -> the smallest point index of the key
//                  count[key]  += 1
//                  least[key]   = max ~order key of the depth    -> the minimum depth; the order key is the monotone
//                                                                   integer image of the float32 (q2 may be negative)
//   pixel sweep  (tile, frame) grid: every pixel re-projects the one point that wrote it last, and, where its key was
//                hit more than once and the key's first point is its own, takes the key's minimum instead; negative
//                depths become 0.  Every pixel of the frame is written, so `out` needs no clearing.
//
// sub2ind multiplies the row by w - 1 (kitti_utils.py:39-43): pixels (r, w-1) and (r+1, 0) share a key, and the
// reference's result depends on it.  bbd_velo_key reproduces the collision on purpose; the pixel sweep's "is the first
// point mine" test is what keeps the pixel that merely shares a key on its last-written value.
//
// All four reductions are integer max / add: the result depends on the order of the points in the input only, never on
// launch geometry or on the order atomics land in.  One memset and two launches; the stream orders them; nothing spins
// on another workgroup and nothing synchronises with the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_velo_math.h"
#include "bbd_device_util.h"

namespace {

constexpr int VT = 256;        // threads per workgroup
constexpr int VTILES = 256;    // pixel-sweep workgroups per frame (one per CU of an MI355X)

struct VeloArgs {
  const float4* points;    // [total points] x, y, z, (reflectance: ignored, the reference overwrites it with 1)
  const int32_t* desc;     // [n, BBD_VELO_DESC]
  const double* proj;      // [n, 12]
  uint32_t* scratch;       // 4 tables of h*w words per frame, zero on entry of the point sweep
  float* out;
  long scratch_ints;
  int vel_depth;
};

struct Frame {
  size_t off;
  int h, w, n_points;
  uint32_t npx;
  const float4* pts;
  const double* P;
  uint32_t *last, *first, *count, *least;
  bool ok;
};

__device__ __forceinline__ Frame load_frame(const VeloArgs& a, int f) {
  const int32_t* d = a.desc + (size_t)f * BBD_VELO_DESC;
  Frame fr;
  fr.off = bbd_join64(d[0], d[1]);
  fr.h = d[2];
  fr.w = d[3];
  fr.n_points = d[4];
  const long poff = d[5], soff = d[6];
  const long npx = (long)fr.h * (long)fr.w;
  // a row that does not fit the scratch it was given is skipped, not trusted
  fr.ok = fr.h >= 1 && fr.w >= 1 && npx < (1L << 31) && fr.n_points >= 0 && poff >= 0 && soff >= 0 &&
          4 * (soff + npx) <= a.scratch_ints;
  fr.npx = fr.ok ? (uint32_t)npx : 0u;
  fr.pts = a.points + poff;
  fr.P = a.proj + (size_t)f * 12;
  fr.last = a.scratch + 4 * (size_t)soff;
  fr.first = fr.last + fr.npx;
  fr.count = fr.first + fr.npx;
  fr.least = fr.count + fr.npx;
  return fr;
}

__device__ __forceinline__ int project(const Frame& fr, uint32_t i, int vel_depth, bbd_velo_hit_t* hit) {
  const float4 p = fr.pts[i];
  return bbd_velo_project(fr.P, p.x, p.y, p.z, fr.h, fr.w, vel_depth, hit);
}

__global__ __launch_bounds__(VT) void velo_point_kernel(VeloArgs a) {
  const Frame fr = load_frame(a, blockIdx.y);
  const uint32_t i = blockIdx.x * (uint32_t)VT + threadIdx.x;
  if (!fr.ok || i >= (uint32_t)fr.n_points) return;
  bbd_velo_hit_t hit;
  if (!project(fr, i, a.vel_depth, &hit)) return;
  atomicMax(fr.last + hit.pixel, i + 1u);
  atomicMax(fr.first + hit.key, ~i);
  atomicAdd(fr.count + hit.key, 1u);
  atomicMax(fr.least + hit.key, ~bbd_viz_order_key(hit.depth));
}

__global__ __launch_bounds__(VT) void velo_pixel_kernel(VeloArgs a) {
  const Frame fr = load_frame(a, blockIdx.y);
  if (!fr.ok) return;
  float* out = a.out + fr.off;
  for (uint32_t p = blockIdx.x * (uint32_t)VT + threadIdx.x; p < fr.npx; p += (uint32_t)VTILES * VT) {
    bbd_velo_hit_t hit;
    float d = 0.0f;
    const uint32_t l = fr.last[p];
    if (l && project(fr, l - 1u, a.vel_depth, &hit)) d = hit.depth;            // depth[v, u] = z, last point wins
    const int r = (int)(p / (uint32_t)fr.w), c = (int)(p - (uint32_t)r * (uint32_t)fr.w);
    const int32_t key = bbd_velo_key(r, c, fr.w);
    if (fr.count[key] > 1u && project(fr, ~fr.first[key], a.vel_depth, &hit) && hit.pixel == (int32_t)p)
      d = bbd_viz_key_value(~fr.least[key]);                                     // minimum over ALL points of the key
    out[p] = bbd_velo_finish(d);
  }
}

}  // namespace

extern "C" int bbd_velo_depth_scratch_ints(int total_pixels, int n_frames) {
  if (total_pixels < 0 || n_frames < 0 || total_pixels > 0x7fffffff / 4) return BBD_E_TOOMANY;
  return 4 * total_pixels;
}

extern "C" int bbd_velo_depth(const float* points, const int32_t* desc, const double* proj, int32_t* scratch,
                              int scratch_ints, float* out, int n_frames, int max_points, int flags, void* stream) {
  if (!desc || !proj || !scratch || !out || n_frames <= 0 || n_frames > 65535 || max_points < 0 || scratch_ints < 0 ||
      (!points && max_points > 0) || (flags & ~BBD_VELO_VEL_DEPTH))
    return BBD_E_BADARG;
  VeloArgs a;
  a.points = reinterpret_cast<const float4*>(points); a.desc = desc; a.proj = proj;
  a.scratch = reinterpret_cast<uint32_t*>(scratch); a.out = out; a.scratch_ints = scratch_ints;
  a.vel_depth = (flags & BBD_VELO_VEL_DEPTH) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = scratch_ints ? hipMemsetAsync(scratch, 0, (size_t)scratch_ints * sizeof(int32_t), st) : hipSuccess;
  if (e != hipSuccess) return (int)e;
  if (max_points > 0)
    hipLaunchKernelGGL(velo_point_kernel, dim3((unsigned)((max_points + VT - 1) / VT), (unsigned)n_frames), dim3(VT), 0, st, a);
  hipLaunchKernelGGL(velo_pixel_kernel, dim3(VTILES, (unsigned)n_frames), dim3(VT), 0, st, a);
  return launch_status();
}
