// bbd_uncert.hip - depth uncertainty from the flip pass, and the sparsification scores that judge an uncertainty map
// (Poggi et al., CVPR 2020: AUSE / AURG), on the device.
//
// bbd_post_process_uncert is bbd_post_process_disp's launch with one more plane: the blend and |d - flip(d')|.
//
// bbd_sparsification scores a ragged batch while it is in HBM.  Four orderings per image (the map under test and the
// three oracles) are four segments of one stable least-significant-digit radix sort; a segment's length is known on the
// device only, so every launch is sized by the capacity the scratch states and workgroups without work leave.
//
//   setup    one workgroup: window areas -> first slot and first chunk of every image (64-bit scan); do they fit?
//   count    a chunk = 1024 window pixels of one image, one per lane: ballot of the valid ones, the chunk's total
//   prefix   one workgroup per image: chunk totals -> exclusive prefixes (bbd_compact.h), N
//   terms    the chunks again: a valid lane computes its terms and stores them, with the four keys, at its slot
//   4 x      histogram  digit counts of a chunk of 1024 sorted slots (integer LDS atomics: exact)
//            offsets    one workgroup per segment: counts -> first rank of every (digit, chunk), digit-major
//            scatter    a lane's rank = that + equal digits in the waves before it + equal digits below it in its wave
//                       (match by 8 ballots): order within a chunk is kept, nothing is decided by an atomic
//   buckets  a wave per (segment, bucket): the terms gathered through the sorted slots and added in the order
//            bbd_uncert_math.h writes down
//   finish   a wave per image: suffix sums and curves (a lane per curve), trapezoids, AUSE / AURG (a lane per metric)
//
// No allocation, no host synchronisation, no atomics on floats: identical calls give identical bytes.  Not tuned: the
// sort moves 8 bytes per valid pixel, ordering and pass each way, and every pass is three launches.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_compact.h"
#include "bbd_device_util.h"
#include "bbd_postproc_math.h"
#include "bbd_uncert_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- the flip pass
constexpr int PT = 128;              // as bbd_postproc.hip
constexpr unsigned PMAX_GX = 64;
constexpr unsigned PMAX_BLOCKS = 4096;

__global__ __launch_bounds__(PT) void post_process_uncert_kernel(const float* __restrict__ disp, float* __restrict__ out,
                                                                 float* __restrict__ uncert, size_t rows, int w,
                                                                 double step) {
  const float* flipped = disp + rows * (size_t)w;
  for (unsigned ux = blockIdx.x * PT + threadIdx.x; ux < (unsigned)w; ux += gridDim.x * PT) {
    const int x = (int)ux, xm = w - 1 - x;
    const double a = bbd_postproc_mask(x, w, step), b = bbd_postproc_mask(xm, w, step);
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y) {
      const size_t base = r * (size_t)w;
      const float ld = disp[base + (size_t)x], rd = flipped[base + (size_t)xm];
      out[base + (size_t)x] = bbd_postproc_blend(ld, rd, a, b);
      uncert[base + (size_t)x] = bbd_uncert_flip(ld, rd);
    }
  }
}

// ---------------------------------------------------------------------------------------------- sparsification
constexpr int UT = BBD_UNCERT_CHUNK;   // threads of a chunk's workgroup: one pixel / slot per lane
constexpr int UW = UT / 64;
constexpr int ST = 256;                // threads of a per-image / per-segment workgroup: one digit per lane
constexpr int BT = 256;                // threads of a bucket workgroup
constexpr int BW = BT / 64;            // its waves: a bucket each

struct UArgs {
  const float* pred;
  const float* uncert;
  const float* gt;
  const int32_t* desc;
  const float* rows;
  double* out;
  char* scratch;
  BbdUncertLayout L;
  int n, h, w, K;
  float min_depth, max_depth, scale_factor;
  int flags;
};

template <typename T>
__device__ __forceinline__ T* at(const UArgs& a, size_t offset) { return reinterpret_cast<T*>(a.scratch + offset); }

__device__ __forceinline__ bool unfit(const UArgs& a) { return *at<int32_t>(a, 0) != 0; }

// keys / slots of buffer `buf`, ordering `o`
__device__ __forceinline__ uint32_t* plane(const UArgs& a, size_t base, int buf, int o) {
  return at<uint32_t>(a, base) + (size_t)(buf * 4 + o) * (size_t)a.L.P;
}

// The image chunk `gc` belongs to: the last i with chunk_off[i] <= gc (gc < chunk_off[n]).
__device__ __forceinline__ int image_of(const int32_t* chunk_off, int n, int gc) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= gc) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(UT) void setup_kernel(UArgs a) {
  __shared__ long long wave_px[UW], wave_ch[UW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int run = (a.n + UT - 1) / UT, j0 = min(tid * run, a.n), j1 = min(j0 + run, a.n);
  long long px = 0, ch = 0;
  for (int j = j0; j < j1; ++j) {
    const long area = bbd_uncert_window(a.desc, j).area;
    px += area;
    ch += (area + UT - 1) / UT;
  }
  long long ipx = px, ich = ch;
  for (int o = 1; o < 64; o <<= 1) {
    const long long tp = __shfl_up(ipx, o, 64), tc = __shfl_up(ich, o, 64);
    if (lane >= o) { ipx += tp; ich += tc; }
  }
  if (lane == 63) { wave_px[wave] = ipx; wave_ch[wave] = ich; }
  __syncthreads();
  long long bpx = 0, bch = 0;
  for (int wv = 0; wv < wave; ++wv) { bpx += wave_px[wv]; bch += wave_ch[wv]; }
  long long ppx = bpx + ipx - px, pch = bch + ich - ch;
  int64_t* pix_off = at<int64_t>(a, a.L.pix_off);
  int32_t* chunk_off = at<int32_t>(a, a.L.chunk_off);
  const long long cap = 0x7fffffffLL;
  for (int j = j0; j < j1; ++j) {
    const long area = bbd_uncert_window(a.desc, j).area;
    pix_off[j] = ppx;
    chunk_off[j] = (int32_t)(pch < cap ? pch : cap);
    ppx += area;
    pch += (area + UT - 1) / UT;
  }
  if (tid == UT - 1) {                                     // its prefix + its run = the totals
    pix_off[a.n] = ppx;
    chunk_off[a.n] = (int32_t)(pch < cap ? pch : cap);
    *at<int32_t>(a, 0) = (ppx > (long long)a.L.P || pch > (long long)a.L.C) ? 1 : 0;
  }
}

// Chunk blockIdx.x: its image, its window and whether this lane's pixel is one the metrics score.
struct ChunkPixel {
  int img, y, x;
  float g;
  bool keep;
};

__device__ __forceinline__ ChunkPixel chunk_pixel(const UArgs& a, const int32_t* chunk_off, int gc, BbdUncertWindow* win) {
  ChunkPixel c;
  c.img = image_of(chunk_off, a.n, gc);
  *win = bbd_uncert_window(a.desc, c.img);
  const long j = (long)(gc - chunk_off[c.img]) * UT + threadIdx.x;
  c.keep = false; c.y = 0; c.x = 0; c.g = 0.0f;
  if (j < win->area) {
    c.y = win->r0 + (int)(j / win->ww);
    c.x = win->c0 + (int)(j % win->ww);
    c.g = a.gt[win->off + (size_t)c.y * win->GW + c.x];
    c.keep = bbd_uncert_valid(c.g, a.min_depth, a.max_depth);
  }
  return c;
}

__global__ __launch_bounds__(UT) void count_kernel(UArgs a) {
  __shared__ int wave_kept[UW];
  const int32_t* chunk_off = at<int32_t>(a, a.L.chunk_off);
  const int gc = blockIdx.x;
  if (unfit(a) || gc >= chunk_off[a.n]) return;
  BbdUncertWindow win;
  const ChunkPixel c = chunk_pixel(a, chunk_off, gc, &win);
  compact_ballot(c.keep, wave_kept);
  __syncthreads();
  if (threadIdx.x == 0) at<int32_t>(a, a.L.chunk_total)[gc] = compact_total<UW>(wave_kept);
}

__global__ __launch_bounds__(ST) void prefix_kernel(UArgs a) {
  __shared__ int wave_total[ST / 64];
  if (unfit(a)) return;
  const int32_t* chunk_off = at<int32_t>(a, a.L.chunk_off);
  const int i = blockIdx.x, first = chunk_off[i];
  compact_scan<ST>(at<int32_t>(a, a.L.chunk_total) + first, chunk_off[i + 1] - first, wave_total,
                   at<int32_t>(a, a.L.count) + i);
}

__global__ __launch_bounds__(UT) void terms_kernel(UArgs a) {
  __shared__ int wave_kept[UW];
  const int32_t* chunk_off = at<int32_t>(a, a.L.chunk_off);
  const int gc = blockIdx.x;
  if (unfit(a) || gc >= chunk_off[a.n]) return;
  BbdUncertWindow win;
  const ChunkPixel c = chunk_pixel(a, chunk_off, gc, &win);
  const unsigned long long mask = compact_ballot(c.keep, wave_kept);
  __syncthreads();
  if (!c.keep) return;
  const int slot = compact_slot(at<int32_t>(a, a.L.chunk_total)[gc], mask, wave_kept);
  const size_t plane_hw = (size_t)a.h * a.w;
  const BbdUncertTerms t = bbd_uncert_terms(a.pred + (size_t)c.img * plane_hw, a.uncert + (size_t)c.img * plane_hw, a.h,
                                            a.w, c.g, c.y, c.x, win.GH, win.GW, a.min_depth, a.max_depth, a.scale_factor,
                                            a.rows[(size_t)c.img * BBD_EVAL_OUT + 7], a.flags);
  const size_t p = (size_t)at<int64_t>(a, a.L.pix_off)[c.img] + (size_t)slot;
  at<float>(a, a.L.e_abs)[p] = t.e_abs;
  at<float>(a, a.L.e_sq)[p] = t.e_sq;
  at<float>(a, a.L.th)[p] = t.th;
  const float key[4] = {t.u, t.e_abs, t.e_sq, t.th};
  for (int o = 0; o < 4; ++o) {
    plane(a, a.L.keys, 0, o)[p] = bbd_uncert_sort_key(key[o]);
    plane(a, a.L.order, 0, o)[p] = (uint32_t)slot;
  }
}

// Sorted-slot chunk blockIdx.x of ordering blockIdx.y: false when the chunk lies past the image's N.
struct SortChunk {
  int img;
  long first, N;           // first rank of the chunk in its segment, length of the segment
  size_t base;             // first slot of the image
};

__device__ __forceinline__ bool sort_chunk(const UArgs& a, SortChunk* s) {
  const int32_t* chunk_off = at<int32_t>(a, a.L.chunk_off);
  const int gc = blockIdx.x;
  if (unfit(a) || gc >= chunk_off[a.n]) return false;
  s->img = image_of(chunk_off, a.n, gc);
  s->N = at<int32_t>(a, a.L.count)[s->img];
  s->first = (long)(gc - chunk_off[s->img]) * UT;
  s->base = (size_t)at<int64_t>(a, a.L.pix_off)[s->img];
  return s->first < s->N;
}

__global__ __launch_bounds__(UT) void histogram_kernel(UArgs a, int shift, int src) {
  __shared__ uint32_t h[256];
  SortChunk s;
  if (!sort_chunk(a, &s)) return;
  const int tid = threadIdx.x, o = blockIdx.y;
  if (tid < 256) h[tid] = 0u;
  __syncthreads();
  const long r = s.first + tid;
  if (r < s.N) atomicAdd(&h[(plane(a, a.L.keys, src, o)[s.base + (size_t)r] >> shift) & 255u], 1u);
  __syncthreads();
  if (tid < 256) at<uint32_t>(a, a.L.hist)[((size_t)o * a.L.C + blockIdx.x) * 256 + tid] = h[tid];
}

__global__ __launch_bounds__(ST) void offsets_kernel(UArgs a) {
  __shared__ uint32_t total[256];
  if (unfit(a)) return;
  const int i = blockIdx.x, o = blockIdx.y, d = threadIdx.x;
  const long N = at<int32_t>(a, a.L.count)[i];
  const int chunks = (int)((N + UT - 1) / UT);
  uint32_t* h = at<uint32_t>(a, a.L.hist) + ((size_t)o * a.L.C + at<int32_t>(a, a.L.chunk_off)[i]) * 256;
  uint32_t run = 0u;
  for (int c = 0; c < chunks; ++c) {
    const uint32_t t = h[(size_t)c * 256 + d];
    h[(size_t)c * 256 + d] = run;
    run += t;
  }
  total[d] = run;
  __syncthreads();
  uint32_t before = 0u;
  for (int e = 0; e < d; ++e) before += total[e];
  for (int c = 0; c < chunks; ++c) h[(size_t)c * 256 + d] += before;
}

__global__ __launch_bounds__(UT) void scatter_kernel(UArgs a, int shift, int src) {
  __shared__ uint32_t wave_digit[UW][256];
  SortChunk s;
  if (!sort_chunk(a, &s)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, o = blockIdx.y;
  for (int j = tid; j < UW * 256; j += UT) (&wave_digit[0][0])[j] = 0u;
  __syncthreads();
  const long r = s.first + tid;
  const bool live = r < s.N;
  uint32_t key = 0u, slot = 0u;
  if (live) {
    key = plane(a, a.L.keys, src, o)[s.base + (size_t)r];
    slot = plane(a, a.L.order, src, o)[s.base + (size_t)r];
  }
  const uint32_t d = (key >> shift) & 255u;
  unsigned long long same = __ballot(live);                 // the live lanes of the wave with this lane's digit
  for (int b = 0; b < 8; ++b) {
    const unsigned long long set = __ballot((d >> b) & 1u);
    same &= ((d >> b) & 1u) ? set : ~set;
  }
  const int below = __popcll(same & ((1ull << lane) - 1ull));
  if (live && below == 0) wave_digit[wave][d] = (uint32_t)__popcll(same);
  __syncthreads();
  if (!live) return;
  uint32_t rank = at<uint32_t>(a, a.L.hist)[((size_t)o * a.L.C + blockIdx.x) * 256 + d] + (uint32_t)below;
  for (int wv = 0; wv < wave; ++wv) rank += wave_digit[wv][d];
  plane(a, a.L.keys, src ^ 1, o)[s.base + rank] = key;
  plane(a, a.L.order, src ^ 1, o)[s.base + rank] = slot;
}

__global__ __launch_bounds__(BT) void buckets_kernel(UArgs a) {
  __shared__ double part[BW][3][BBD_UNCERT_LANES];
  if (unfit(a)) return;
  const int i = blockIdx.x, o = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long N = at<int32_t>(a, a.L.count)[i];
  if (N < 1) return;
  const size_t base = (size_t)at<int64_t>(a, a.L.pix_off)[i];
  const int b = blockIdx.z * BW + wave;                            // a wave per bucket
  if (b < a.K) {
    double s[3];
    bbd_uncert_lane_sums(at<float>(a, a.L.e_abs) + base, at<float>(a, a.L.e_sq) + base, at<float>(a, a.L.th) + base,
                         plane(a, a.L.order, 0, o) + base,         // four passes: the result is back in buffer 0
                         bbd_uncert_rank(b, N, a.K), bbd_uncert_rank(b + 1, N, a.K), lane, s);
    for (int t = 0; t < 3; ++t) part[wave][t][lane] = s[t];
  }
  __syncthreads();
  // ordering 0 (the map under test) feeds the three sparse curves, ordering 1 + t the oracle curve of metric t
  if (b < a.K && lane < 3 && (o == 0 || lane == o - 1))
    at<double>(a, a.L.bsum)[(size_t)i * BBD_UNCERT_BSUMS + (size_t)((o == 0 ? 0 : 3) + lane) * BBD_SPARS_MAX_INTERVALS + b] =
        bbd_uncert_tree(part[wave][lane]);
}

__global__ __launch_bounds__(64) void finish_kernel(UArgs a) {
  const int i = blockIdx.x, lane = threadIdx.x, width = BBD_SPARS_SUMMARY + 6 * (a.K + 1);
  const bool fits = !unfit(a);
  const long N = fits ? (long)at<int32_t>(a, a.L.count)[i] : 0;
  double* row = a.out + (size_t)i * width;
  if (N < 1) {
    for (int j = lane; j < width; j += 64) row[j] = bbd_uncert_empty(j, fits);
    return;
  }
  if (lane < 6)                                                    // a lane per curve, then a lane per metric
    bbd_uncert_curve(at<double>(a, a.L.bsum) + (size_t)i * BBD_UNCERT_BSUMS + (size_t)lane * BBD_SPARS_MAX_INTERVALS, N,
                     a.K, lane % 3, row + BBD_SPARS_SUMMARY + (size_t)lane * (a.K + 1));
  __syncthreads();
  if (lane < 3) bbd_uncert_scores(row + BBD_SPARS_SUMMARY, a.K, lane, row);
  if (lane == 3) { row[6] = (double)N; row[7] = 0.0; }
}

}  // namespace

extern "C" int bbd_post_process_uncert(const float* disp, float* out, float* uncert, int n, int h, int w, void* stream) {
  if (!disp || !out || !uncert || n < 1 || h < 1 || w < 1) return BBD_E_BADARG;
  const size_t rows = (size_t)n * (size_t)h;
  unsigned gx = ((unsigned)w + PT - 1) / PT;
  gx = gx < PMAX_GX ? gx : PMAX_GX;
  const size_t want_y = PMAX_BLOCKS / gx;
  const unsigned gy = (unsigned)(rows < want_y ? rows : want_y);
  hipLaunchKernelGGL(post_process_uncert_kernel, dim3(gx, gy), dim3(PT), 0, static_cast<hipStream_t>(stream), disp, out,
                     uncert, rows, w, bbd_postproc_step(w));
  return launch_status();
}

extern "C" int bbd_sparsification(const float* pred, const float* uncert, const float* gt, const int32_t* desc,
                                  const float* rows, double* out, void* scratch, long scratch_bytes, int n, int h, int w,
                                  int intervals, double min_depth, double max_depth, double scale_factor, int flags,
                                  void* stream) {
  UArgs a;
  const int rc = bbd_uncert_status(pred, uncert, gt, desc, rows, out, scratch, scratch_bytes, n, h, w, intervals, flags,
                                   &a.L);
  if (rc) return rc;
  a.pred = pred; a.uncert = uncert; a.gt = gt; a.desc = desc; a.rows = rows; a.out = out;
  a.scratch = static_cast<char*>(scratch);
  a.n = n; a.h = h; a.w = w; a.K = intervals;
  a.min_depth = (float)min_depth; a.max_depth = (float)max_depth; a.scale_factor = (float)scale_factor;
  a.flags = flags;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 chunks((unsigned)a.L.C), segments_of_chunks((unsigned)a.L.C, 4), segments((unsigned)n, 4);
  hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(UT), 0, st, a);
  hipLaunchKernelGGL(count_kernel, chunks, dim3(UT), 0, st, a);
  hipLaunchKernelGGL(prefix_kernel, dim3((unsigned)n), dim3(ST), 0, st, a);
  hipLaunchKernelGGL(terms_kernel, chunks, dim3(UT), 0, st, a);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(histogram_kernel, segments_of_chunks, dim3(UT), 0, st, a, 8 * pass, pass & 1);
    hipLaunchKernelGGL(offsets_kernel, segments, dim3(ST), 0, st, a);
    hipLaunchKernelGGL(scatter_kernel, segments_of_chunks, dim3(UT), 0, st, a, 8 * pass, pass & 1);
  }
  hipLaunchKernelGGL(buckets_kernel, dim3((unsigned)n, 4, (unsigned)((intervals + BW - 1) / BW)), dim3(BT), 0, st, a);
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)n), dim3(64), 0, st, a);
  return launch_status();
}
