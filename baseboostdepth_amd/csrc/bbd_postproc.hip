// bbd_postproc.hip - flip post-processing of predicted disparities on the device (Monodepth2's
// batch_post_process_disparity, evaluate_depth.py --post_process).
//
// The networks run on a batch and its left-right flipped copy; this kernel blends the two predictions of every image:
// near the left border the flipped prediction wins, near the right border the plain one, in between their mean.  The
// flipped half is read mirrored (disp[n+i][y][w-1-x]), so it is never flipped back in memory.
//
// One thread owns a column x of the row tile it is given: the two float64 mask values of the column are computed once,
// then the thread walks rows (image x row, the two flattened) with a grid stride.  Per pixel: two 4-byte reads, one
// 4-byte write; a wave's mirrored read is the same 256 contiguous bytes walked backwards.  No LDS, no atomics, nothing
// allocated: identical calls give identical bytes.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/bbd_hip.h"
#include "bbd_device_util.h"
#include "bbd_postproc_math.h"

namespace {

constexpr int PT = 128;              // threads per workgroup: 640 and 1024 columns are whole multiples
constexpr unsigned PMAX_GX = 64;     // column tiles per row before a thread takes more than one column
constexpr unsigned PMAX_BLOCKS = 4096;

__global__ __launch_bounds__(PT) void post_process_kernel(const float* __restrict__ disp, float* __restrict__ out,
                                                          size_t rows, int w, double step) {
  const float* flipped = disp + rows * (size_t)w;
  for (unsigned ux = blockIdx.x * PT + threadIdx.x; ux < (unsigned)w; ux += gridDim.x * PT) {   // unsigned: no overflow
    const int x = (int)ux, xm = w - 1 - x;
    const double a = bbd_postproc_mask(x, w, step), b = bbd_postproc_mask(xm, w, step);
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y) {
      const size_t base = r * (size_t)w;
      out[base + (size_t)x] = bbd_postproc_blend(disp[base + (size_t)x], flipped[base + (size_t)xm], a, b);
    }
  }
}

}  // namespace

extern "C" int bbd_post_process_disp(const float* disp, float* out, int n, int h, int w, void* stream) {
  if (!disp || !out || n < 1 || h < 1 || w < 1) return BBD_E_BADARG;
  const size_t rows = (size_t)n * (size_t)h;
  unsigned gx = ((unsigned)w + PT - 1) / PT;
  gx = gx < PMAX_GX ? gx : PMAX_GX;
  const size_t want_y = PMAX_BLOCKS / gx;
  const unsigned gy = (unsigned)(rows < want_y ? rows : want_y);
  hipLaunchKernelGGL(post_process_kernel, dim3(gx, gy), dim3(PT), 0, static_cast<hipStream_t>(stream), disp, out, rows,
                     w, bbd_postproc_step(w));
  return launch_status();
}
