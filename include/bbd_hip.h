/*
 * bbd_hip.h - C ABI of the MI355X-native photometric-reprojection hot path.
 *
 * The upstream reference (kieran514/baseboostdepth) has no FFI / plugin interface: its
 * seam is Python (`Trainer.process_batch`, trainer.py:286-308).  This header is the drop-in
 * boundary the build adds underneath that seam: every entry point replaces a group of
 * eager PyTorch calls in the reference and cites them.  Rules for every function:
 *
 *   - plain pointers and sizes only (no torch types); all pointers are DEVICE pointers
 *     unless the parameter is documented "host";
 *   - no allocation, no synchronisation: work is enqueued on `stream` (a hipStream_t passed
 *     as void*; NULL = the null stream) and the call returns immediately;
 *   - return value 0 = enqueued, >0 = hipError_t from the launch, <0 = BBD_E_* argument error;
 *   - tensors are fp32, contiguous, NCHW like the reference's batch dict.
 *
 * Python binding: baseboostdepth_amd/_lib.py (ctypes).  It is READ FROM THIS HEADER at import (baseboostdepth_amd/_abi.py):
 * argument and result types of every prototype, and every `#define BBD_<NAME> <integer>`, which Python sees as
 * `_lib.<NAME>`.  A new entry point therefore needs its prototype here, its definition in a csrc .hip file, a host port under
 * tests/host_port/ (`hp_<name>`: the same parameters minus `stream`) and the Python function that calls it - nothing else.
 * What the reader accepts, and so what this header keeps to:
 *   - results `int` or `long`; parameters `int`, `long`, `unsigned` or `double` by value, everything else a pointer;
 *   - `void* stream` is the LAST parameter of every function that enqueues work; a function without it is a host-side
 *     helper and becomes `lib.<name minus bbd_>` (one without parameters: a constant of the build, bound as its value);
 *   - a BBD_* define is ONE integer literal: decimal, hex or a parenthesised negative - no expressions, no suffixes.
 * Anything else makes the import raise, naming the function and parameter or the macro.  See INTEGRATION.md for the stub a
 * reference maintainer would add.
 */
#ifndef BBD_HIP_H
#define BBD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on EVERY incompatible change of a prototype or of a scratch-size contract; the Python binding refuses a
 * library whose number differs (a stale build selected through BBD_HIP_LIB, or a C caller compiled against an older
 * header, would otherwise mis-marshal pointers into a kernel).  1 = round 1; 2 = bbd_bn_act_bwd gained `beta`, BN
 * scratch sizing changed (round 2, was not bumped then); 3 = round 3 (backward tiling / scratch contract); 4 = the
 * depth-wise token weight gradient's scratch contract (one partial row per workgroup) and `add_input` of
 * bbd_dwconv_tokens_fwd became a bit field (round 3, with the bbd_token_ln_* / bbd_colsum additions); 5 = round 4 (the
 * work-item table of the fused launches, per-row `invert` of the pose matrices, the multi-scale smoothness launches);
 * 6 = round 5: bbd_bn_act_grouped_fwd gained `untracked_groups` (the padding group of the batched pose pass);
 * 7 = round 6: bbd_bn_act_grouped_dev_fwd / _bwd (group table resident on the device: launches whose arguments do not
 * depend on the batch signature); 8 = bbd_disp_viz / bbd_disp_viz_scratch_ints (single-image prediction);
 * 9 = bbd_velo_depth / bbd_velo_depth_scratch_ints (ground-truth depth maps from Velodyne scans);
 * 10 = bbd_syns_* / bbd_chamfer_nn (SYNS-Patches evaluation: edge and point-cloud metrics);
 * 11 = bbd_pose_ate (KITTI odometry evaluation: chained poses, local ground truth, trajectory error);
 * 12 = bbd_post_process_disp (depth evaluation: flip post-processing of the predicted disparities);
 * 14 = bbd_pose_trajectory (KITTI odometry: full-trajectory t_rel, r_rel and aligned ATE);
 * 15 = bbd_point_cloud (coloured point clouds); 16 = bbd_map_* (voxel-fused scene map);
 * 17 = bbd_view_* (points and polylines rasterised into a z-buffered canvas);
 * 18 = bbd_ground_scale (metric scale of a prediction from the camera's height above the ground);
 * 19 = bbd_disp_head_fwd / _bwd (the disparity head with its sigmoid inside);
 * 20 = bbd_depth_consistency (depth-pose geometric consistency: a score and a filter for the scene map);
 * 21 = bbd_stem_* (the encoder stem: BatchNorm + ReLU + max-pool in one pass each way);
 * 22 = bbd_upcat_pad_act_* / bbd_bias_elu_pad_* (the depth decoder's bias + ELU inside its pad / up-sample passes);
 * 23 = bbd_post_process_uncert / bbd_sparsification (depth uncertainty from the flip pass and its AUSE / AURG scores);
 * 24 = bbd_conv3x3_wgrad (the decoder's 3x3 weight gradients from the NCHW tensors);
 * 25 = bbd_geo_fwd / bbd_geo_bwd (the geometry-consistency loss for training, forward and backward);
 * 26 = bbd_up2conv3x3_fwd / _bwd (the decoder's finest up-sample + pad + 3x3 convolution in sub-pixel form);
 * 27 = bbd_sgm_hints (semi-global stereo matching: proxy disparities for --depth_hints);
 * 28 = bbd_depth_metrics_affine (depth evaluation under a per-image least-squares scale and shift);
 * 29 = bbd_stem_conv7s2_fwd / _wgrad (the encoder stems' 7x7 stride-2 convolution and its weight gradient);
 * 30 = bbd_conv1x1s2_fwd / _bwd_data / _wgrad (the ResNet shortcuts' 1x1 stride-2 convolution, three directions). */
#define BBD_ABI_VERSION 30

/* Source frames live in separate tensors, one per frame id (inputs[("color", f, 0)],
 * trainer.py:428).  A "slot" indexes a host array of their base pointers. */
#define BBD_MAX_FRAME_SLOTS 16   /* f = -7..7 and 's' */
#define BBD_MAX_CAND 20          /* reference maximum is 18 (trainer.py:1025-1042) */

#define BBD_KIND_WARP 0          /* reprojection or error-induced candidate */
#define BBD_KIND_IDENT 1         /* identity candidate (+ noise) */
#define BBD_FLAG_NO_POSE_GRAD 0x100 /* warp row whose pose is a constant (stereo_T, T_error) */
/* Optional pairing hint of a WARP candidate, bits 16-23 of `kind`: 1 + the index (arg-min id) of another warp
 * candidate of the same sample that samples the SAME source image (the error-induced warp of a frame and its true-pose
 * warp, trainer.py:439-442).  The backward takes two candidates per pass and prefers the hinted partner (their gathers
 * share cache lines); 0 = no hint (the next candidate in id order is taken).  A speed hint: min-loss maps, arg-min ids,
 * depth and warped images are bit-for-bit the same with any hint (the running minimum is order-free); the backward adds
 * a pixel's per-candidate depth gradients in visiting order, so disparity gradients are deterministic for a given table
 * and equal across tables up to fp32 summation order (a pixel collects gradient from every candidate that won one of
 * its 3x3 neighbours). */
#define BBD_PAIR_SHIFT 16

#define BBD_E_BADARG (-1)
#define BBD_E_TOOMANY (-2)

/* One arg-min candidate of one target sample; candidates are stored [B][BBD_MAX_CAND] in
 * the reference's arg-min id order (trainer.py:549-555, 983-1100).
 *   WARP : slot/row select the source image frames[slot] + row*3*H*W; `pose` is the row of
 *          the pose table; kind may be OR-ed with BBD_FLAG_NO_POSE_GRAD.
 *   IDENT: `row` is the row of the identity-loss tensor [NI,H,W]. */
typedef struct bbd_cand {
  int32_t kind;
  int32_t slot;
  int32_t row;
  int32_t pose;
} bbd_cand_t;

/* Row of the pose table (40 floats) of one (warp job, sample):  K[:3,:] row-major (12),
 * T row-major (16), inv_K[:3,:3] row-major (9), 3 pad.  bbd_pose_expand turns it into the
 * projection table with the reference's CPU rounding order; replaces the per-warp matmul chain
 * of layers.py:163-165 and :182-185. */
#define BBD_POSE_STRIDE 40

/* Row of the projection table (24 floats) the fused kernels read: P = (K@T)[:3,:] row-major (12),
 * inv_K[:3,:3] row-major (9), 3 pad.  Produced from the pose table by bbd_pose_expand. */
#define BBD_PROJ_STRIDE 24

/* Geometry of the launch tiling, so callers can size scratch buffers. */
int bbd_abi_version(void);
int bbd_tile_w(void);
int bbd_tile_h(void);
int bbd_num_tiles(int H, int W);
/* tiles of the fused FORWARD launch: sizes partial [S, B, bbd_num_tiles_fwd(H,W)]; bbd_num_tiles = the 64x16 tiling
 * of the identity / SSIM-map kernels */
int bbd_num_tiles_fwd(int H, int W);
/* tiles of the BACKWARD launch: sizes grad_proj [S, NP, bbd_num_tiles_bwd(H,W), 12] */
int bbd_num_tiles_bwd(int H, int W);

/* Pose composition of a step in one launch each way (replaces the per-frame Python loops of
 * trainer.py:359-388 (incremental chain), :376-377 / :403-405 (T_error) and :415-418 (partial swap)).
 *   steps  [R,4,4]   every pose-network result of the step (transformation_from_parameters output), row-major
 *   table  int32 [NO][BBD_COMPOSE_STRIDE]: {n, i0..i6, direct, flags, 0, 0} per composed matrix:
 *            out = steps[i0] @ steps[i1] @ ... @ steps[i(n-1)]   (n = 0: identity; products rounded like torch.matmul
 *            on the reference's CPU path); flags & BBD_COMPOSE_REPLACE: the 4th column is then taken from
 *            steps[direct]; flags & BBD_COMPOSE_ERROR: out[:3,3] /= pose_error and the row carries no gradient
 *   out    [NO,4,4]
 * Backward: refs_off int32 [R+1], refs int32 [.][2] = for each step row the (output row, chain position | -1 = direct)
 * pairs that read it; grad_steps [R,4,4] is written whole (zeros for unreferenced rows).  Deterministic. */
#define BBD_COMPOSE_STRIDE 12
#define BBD_COMPOSE_ERROR 1
#define BBD_COMPOSE_REPLACE 2
int bbd_pose_compose_fwd(const float* steps, const int32_t* table, float* out, int NO, double pose_error, void* stream);
int bbd_pose_compose_bwd(const float* steps, const int32_t* table, const int32_t* refs_off, const int32_t* refs,
                         const float* grad_out, float* grad_steps, int R, void* stream);

/* Pose table [NP,40] -> projection table [NP,24]: P = (K@T)[:3,:] formed with the rounding order of
 * the reference's CPU torch.matmul (layers.py:182), inv_K[:3,:3] copied. */
int bbd_pose_expand(const float* pose, float* proj, int NP, void* stream);

/* Identity photometric loss  0.85*mean_c SSIM(src, tgt) + 0.15*mean_c |tgt - src|
 * for NI (target sample, source image) pairs.  Replaces trainer.py:501-508
 * (compute_reprojection_loss on un-warped sources; layers.py:219-249).
 *   frames  host array[BBD_MAX_FRAME_SLOTS] of device pointers to [n_f,3,H,W] tensors
 *   target  [B,3,H,W]
 *   items   device int32 [NI][4] = {target sample, slot, row, 0}
 *   ident   out [NI,H,W]                                                            */
int bbd_identity_loss_fwd(const void* const* frames, const float* target,
                          const int32_t* items, int NI, float* ident,
                          int H, int W, int no_ssim, void* stream);
/* Grouped form of the same (what the trainer calls): the items of group g are items[group_off[g] .. group_off[g+1]) and
 * share ONE target sample (items[first].target): the target tile and its window statistics are set up once per group
 * and tile instead of once per item, the next item's source travels while the current one's SSIM runs.
 *   group_off  device int32 [G+1]        Same results, bit for bit. */
int bbd_identity_loss_grouped_fwd(const void* const* frames, const float* target, const int32_t* items,
                                  const int32_t* group_off, int G, float* ident, int H, int W, int no_ssim,
                                  void* stream);

/* Fused forward:  back-project -> project -> bilinear border sample -> SSIM+L1 ->
 * per-pixel min/arg-min over the sample's candidate list, for S scales x B samples.
 * Replaces trainer.py:421-442 (warping_block), :477-486, :525-557 and x_min_opt :983-1100,
 * i.e. layers.BackprojectDepth/Project3D/SSIM + F.grid_sample + cat + torch.min.
 *   depth      [S,B,H,W]   full-resolution depth per scale (outputs[("depth",0,s)])
 *   proj       [NP,24]     projection table from bbd_pose_expand (see BBD_PROJ_STRIDE)
 *   ident      [NI,H,W]    identity losses from bbd_identity_loss_fwd
 *   noise      [B,H,W]     identity noise per sample (trainer.py:518-523), may be NULL
 *   cand/ncand [B][BBD_MAX_CAND] / [B]
 *   min_loss   out [S,B,H,W]   value of the winning candidate (to_optimise)
 *   argmin     out [S,B,H,W]   u8 id of the winning candidate (ident, trainer.py:546)
 *   partial    out [S,B,ntiles] per-tile sums of min_loss (deterministic 2-stage mean)
 *   warped     out [S,NP,3,H,W] or NULL: materialise outputs[("color"/"color_D",f,s)]      */
int bbd_warp_ssim_min_fwd(const void* const* frames, const float* target, const float* depth,
                          const float* proj, const float* ident, const float* noise,
                          const bbd_cand_t* cand, const int32_t* ncand,
                          float* min_loss, uint8_t* argmin, float* partial, float* warped,
                          int S, int B, int NP, int H, int W, int no_ssim, void* stream);

/* Fused backward of the above w.r.t. depth and P = (K@T)[:3,:] of every pose-table row.
 * Replaces the autograd of min.dim, avg_pool2d, reflection_pad2d, grid_sampler_2d and bmm
 * (SURVEY.md Appendix A4-A6).  Gradient flows only to the arg-min candidate of each pixel.
 *   gscale       [S]           d loss / d min_loss[s,...] (one scalar per scale, device)
 *   grad_depth   out [S,B,H,W]
 *   grad_proj    out [S,NP,ntiles,12]  per-tile partial sums of dL/dP (caller reduces over
 *                               tiles and applies dL/dT = K[:3,:]^T dL/dP; rows never visited
 *                               are written as zeros)                                        */
int bbd_warp_ssim_min_bwd(const void* const* frames, const float* target, const float* depth,
                          const float* proj, const bbd_cand_t* cand, const int32_t* ncand,
                          const uint8_t* argmin, const float* gscale,
                          float* grad_depth, float* grad_proj,
                          int S, int B, int NP, int H, int W, int no_ssim, void* stream);

/* Disparity-mode forms of the two launches: instead of depth planes they take the decoder's
 * disparity maps themselves - disp = host array of S device pointers ([B,1,h_s,w_s] each), disp_hw = host array
 * {h_0,w_0,h_1,w_1,...} - and evaluate F.interpolate(bilinear, align_corners=False) + layers.disp_to_depth
 * (trainer.py:455-461, layers.py:13-22) per staged pixel, bit-identical to bbd_disp_to_depth_fwd.  No depth
 * buffer is read; depth_out (optional, [S,B,H,W]) receives outputs[("depth",0,s)] as a by-product.
 * The backward takes `depth` = the forward's depth_out (or NULL: it then re-evaluates the up-sampling per staged
 * pixel, +5 % instructions) and hands back grad_up [S,B,H,W] = d loss / d (up-sampled disparity); for a scale at full
 * resolution that IS the disparity gradient, the reduced scales go through bbd_disp_upsample_adjoint
 * (ONE launch for all of them; n <= 4 entries: grad_up[i] -> grad_disp[i] [B,h_i,w_i]; deterministic).
 * work_items (device [S*B*ntiles][2] int32 from bbd_fused_work_items, or NULL = grid order decoded in the kernel): which
 * (sample, scale, tile) each workgroup takes.  A speed choice: results do not depend on it.                 */
int bbd_warp_ssim_min_disp_fwd(const void* const* frames, const float* target, const void* const* disp,
                               const int32_t* disp_hw, double min_depth, double max_depth, const float* proj,
                               const float* ident, const float* noise, const bbd_cand_t* cand, const int32_t* ncand,
                               const int32_t* work_items, float* min_loss, uint8_t* argmin, float* partial, float* warped,
                               float* depth_out, int S, int B, int NP, int H, int W, int no_ssim, void* stream);
int bbd_warp_ssim_min_disp_bwd(const void* const* frames, const float* target, const void* const* disp,
                               const int32_t* disp_hw, double min_depth, double max_depth, const float* depth,
                               const float* proj, const bbd_cand_t* cand, const int32_t* ncand,
                               const int32_t* work_items, const uint8_t* argmin, const float* gscale, float* grad_up,
                               float* grad_proj, int S, int B, int NP, int H, int W, int no_ssim, void* stream);
/* Work order of the fused launches (host function, fills a HOST buffer the caller uploads once per batch signature):
 * out [S*B*ntiles][2] for the forward (backward = 0, ntiles = bbd_num_tiles_fwd) or the backward (1, bbd_num_tiles_bwd)
 * launch.  Slab order: every XCD walks one slab of consecutive tiles - for every sample in `sample_order` (host [B], a
 * permutation of 0..B-1, or NULL = 0..B-1; list the samples with the most candidates first so that a batch mixing 8-,
 * 14- and 18-candidate samples, mono_dataset.py:87-109, ends on its cheap workgroups), for every scale, the slab's
 * tiles - so the scales of a sample share one XCD's L2 and every XCD gets the same work.                    */
int bbd_fused_work_items(int B, int S, int H, int W, int backward, const int32_t* sample_order, int32_t* out);
int bbd_disp_upsample_adjoint(const void* const* grad_up, const int32_t* disp_hw, void* const* grad_disp, int n, int B,
                              int H, int W, void* stream);

/* disp -> full-resolution depth:  bilinear upsample (align_corners=False) then
 * depth = 1 / (1/max + (1/min - 1/max) * disp).  Replaces trainer.py:455-461 and
 * layers.disp_to_depth (layers.py:13-22).  disp [B,h,w] -> depth [B,H,W].           */
int bbd_disp_to_depth_fwd(const float* disp, float* depth, int B, int h, int w, int H, int W,
                          double min_depth, double max_depth, void* stream);
/* grad_disp [B,h,w] is OVERWRITTEN with the adjoint (gather form, deterministic).  `depth` is the
 * forward's output [B,H,W] (d depth/d disp_up = -span*depth^2) or NULL to recompute it from disp. */
int bbd_disp_to_depth_bwd(const float* disp, const float* depth, const float* grad_depth, float* grad_disp,
                          int B, int h, int w, int H, int W,
                          double min_depth, double max_depth, void* stream);

/* Pose matrix from the pose head's output: layers.transformation_from_parameters
 * (layers.py:25-100: rot_from_axisangle, get_translation_matrix, T@R or R^T@T(-t)).
 *   axisangle, translation [n,3] -> M [n,4,4];  bwd: grad_M [n,4,4] -> grads [n,3] each.
 *   invert_rows (device [n] int32, or NULL): per-row `invert` flag that replaces the scalar one, so that the poses of
 *   BOTH signs of a step (trainer.py:360,384,402: invert for negative frame ids) are one launch each way.         */
int bbd_pose_matrix_fwd(const float* axisangle, const float* translation, float* M, int n, int invert,
                        const int32_t* invert_rows, void* stream);
int bbd_pose_matrix_bwd(const float* axisangle, const float* translation, const float* grad_M,
                        float* grad_axisangle, float* grad_translation, int n, int invert,
                        const int32_t* invert_rows, void* stream);

/* Edge-aware smoothness of the mean-normalised disparity: layers.get_smooth_loss
 * (layers.py:203-216) applied to disp / (mean_{H,W}(disp) + 1e-7) as in trainer.py:560-563.
 *   disp [B,h,w], img [B,3,h,w]
 *   fwd : mean_disp out [B, bbd_smooth_chunks()] partial sums of disp (mean = sum / (h*w));
 *         sums out [B, bbd_smooth_chunks(), 2] partial sums of the x- and
 *         y-terms; smooth = sum(x-terms)/(B*h*(w-1)) + sum(y-terms)/(B*(h-1)*w)
 *   bwd : gscale [1] device scalar dL/d(smooth); dots scratch [B, bbd_smooth_chunks()];
 *         grad_disp out [B,h,w] (overwritten).  Deterministic (fixed reduction order).        */
int bbd_smooth_chunks(void);
int bbd_smooth_loss_fwd(const float* disp, const float* img, float* mean_disp, float* sums,
                        int B, int h, int w, void* stream);
int bbd_smooth_loss_bwd(const float* disp, const float* img, const float* mean_disp,
                        const float* gscale, float* grad_disp, float* dots,
                        int B, int h, int w, void* stream);
/* The same for ALL scales of a step (trainer.py:527-564 loops over opt.scales) in one launch pair each way: disp / img /
 * grad_disp = host arrays of S (<= 4) device pointers, hw = host {h_0,w_0,h_1,w_1,...}; mean_disp [S,B,chunks],
 * sums [S,B,chunks,2], dots [S,B,chunks], gscale [S] (device).  Same kernels, same reduction order as the single-scale
 * form (which is the S = 1 case).                                                                              */
int bbd_smooth_loss_multi_fwd(const void* const* disp, const void* const* img, const int32_t* hw, float* mean_disp,
                              float* sums, int S, int B, void* stream);
int bbd_smooth_loss_multi_bwd(const void* const* disp, const void* const* img, const int32_t* hw,
                              const float* mean_disp, const float* gscale, void* const* grad_disp, float* dots,
                              int S, int B, void* stream);

/* Stand-alone kernels behind the reference's layer classes (the training step uses the fused entry
 * points above and never materialises these tensors; callers written against the reference's
 * `layers` module - including its own trainer - get differentiable modules through these).
 *   bbd_backproject_fwd : layers.BackprojectDepth.forward (layers.py:160-167)
 *                         depth [n,H,W], inv_K [n,4,4] -> points [n,4,H*W]
 *   bbd_project3d_fwd   : layers.Project3D.forward (layers.py:181-195)
 *                         points [n,4,H*W], K [n,4,4], T [n,4,4] -> grid [n,H,W,2] in [-1,1]
 *   bbd_ssim_fwd        : layers.SSIM.forward (layers.py:235-249)  x,y [n,3,H,W] -> [n,3,H,W] */
int bbd_backproject_fwd(const float* depth, const float* inv_K, float* points, int n, int H, int W,
                        void* stream);
int bbd_project3d_fwd(const float* points, const float* K, const float* T, float* grid,
                      int n, int H, int W, double eps, void* stream);
int bbd_ssim_fwd(const float* x, const float* y, float* out, int n, int H, int W, void* stream);

/* Their backward passes (the reference's layers are plain autograd nn.Modules, layers.py:136-249, and its
 * trainer back-propagates through them, trainer.py:434-442, 477-486).  Closed forms of SURVEY Appendix A.
 *   bbd_backproject_bwd : grad_points [n,4,H*W] -> grad_depth [n,H,W]          (inv_K carries no gradient)
 *   bbd_project3d_bwd   : grad_grid [n,H,W,2] -> grad_points [n,4,H*W] and gp_partial
 *                         [n, bbd_project3d_bwd_blocks(), 12]: per-workgroup partial sums of dL/dP,
 *                         P = (K@T)[:3,:]; the caller sums them (fixed order => deterministic) and
 *                         forms dL/dT = K[:3,:]^T dP, dL/dK[:3,:] = dP T^T
 *   bbd_ssim_bwd        : grad_out [n,3,H,W] -> grad_x [n,3,H,W]; the SSIM expression is symmetric in
 *                         its two arguments, so d/dy is the same call with x and y exchanged          */
int bbd_backproject_bwd(const float* grad_points, const float* inv_K, float* grad_depth, int n, int H, int W,
                        void* stream);
int bbd_project3d_bwd_blocks(void);
int bbd_project3d_bwd(const float* points, const float* K, const float* T, const float* grad_grid,
                      float* grad_points, float* gp_partial, int n, int H, int W, double eps, void* stream);
int bbd_ssim_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, int n, int H, int W,
                 void* stream);

/* Validation metrics on the device: one workgroup per image.
 *   flags 0                       : Trainer.compute_depth_losses, KITTI branch (trainer.py:594-617):
 *                                   pred = depth [n,h,w]; F.interpolate(bilinear, align_corners=False)
 *                                   to the ground-truth size, clamp to [clamp_lo, clamp_hi], mask
 *                                   (min_depth < gt < max_depth inside the window), torch.median
 *                                   scaling (lower median), clamp, layers.compute_depth_errors.
 *   BBD_EVAL_PRED_IS_DISP         : evaluate_depth.py:244-297: pred = disparity, cv2.resize (linear)
 *                                   then 1/disp, times scale_factor (opt.pred_depth_scale_factor).
 *   BBD_EVAL_MEDIAN_MIDPOINT      : np.median (mean of the two middle values) instead of torch.median.
 *   BBD_EVAL_NO_MEDIAN_SCALING    : opt.disable_median_scaling (stereo evaluation).
 * gt is a ragged buffer; desc[i] = {offset_lo, offset_hi (elements), GH, GW, r0, r1, c0, c1} with
 * [r0,r1) x [c0,c1) the crop window (Garg crop, trainer.py:603-606; whole image = 0,GH,0,GW).
 * out[i] = {abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, median_gt, median_pred, count, 0}. */
#define BBD_EVAL_DESC 8
#define BBD_EVAL_OUT 12
#define BBD_EVAL_PRED_IS_DISP 1
#define BBD_EVAL_MEDIAN_MIDPOINT 2
#define BBD_EVAL_NO_MEDIAN_SCALING 4
int bbd_depth_metrics(const float* pred, const float* gt, const int32_t* desc, float* out, int n, int h,
                      int w, double min_depth, double max_depth, double clamp_lo, double clamp_hi,
                      double scale_factor, int flags, void* stream);

/* Colour-mapped disparity of single-image prediction (test_simple.py:135-148), n images per call, never leaving
 * the device.  For image i, with desc[i] = {offset_lo, offset_hi (pixels), H0, W0} (original sizes, ragged):
 *   d    = F.interpolate(disp[i], (H0, W0), bilinear, align_corners=False)      (not materialised)
 *   s    = min_disp + (max_disp - min_disp) * d                                 layers.disp_to_depth, fp32
 *   vmin = min(s);  vmax = np.percentile(s, percentile)                         numpy "linear" method on float32:
 *          both bracketing order statistics are selected exactly (radix select on the float bit patterns, integer
 *          histograms) and interpolated in numpy's float32 arithmetic (bbd_viz_math.h)
 *   out_u8[3*offset + 3*(y*W0+x) + c] = trunc(magma[idx][c] * 255),  idx = trunc((s - vmin) / (vmax - vmin) * 256),
 *          256 and everything above vmax -> 255, vmax == vmin -> 0       matplotlib Normalize + ScalarMappable.to_rgba
 * lut is that table, uint8 [256,3] (baseboostdepth_amd/magma_lut.hex).  out_float (may be NULL) receives s at
 * out_float + offset.  stats[i] = {vmin, vmax, lower, upper order statistic}.  Offsets that are multiples of 4
 * pixels get packed 12-byte stores.  scratch holds bbd_disp_viz_scratch_ints(n) int32 and is zeroed on `stream` by
 * the call; four launches, no host synchronisation; results do not depend on launch geometry or atomic order.
 * percentile in (0, 100]; min_disp = 1 / max_depth, max_disp = 1 / min_depth as Python doubles. */
#define BBD_VIZ_DESC 4
int bbd_disp_viz_scratch_ints(int n);
int bbd_disp_viz(const float* disp, const int32_t* desc, const uint8_t* lut, uint8_t* out_u8, float* out_float,
                 float* stats, int32_t* scratch, int n, int h, int w, double min_disp, double max_disp,
                 double percentile, void* stream);

/* Training-log panel (csrc/bbd_panel.hip): a grid of rows x cols tiles of H x W pixels each, rendered on the device
 * from what a training step leaves behind, into ONE uint8 RGB image out [rows*H, cols*W, 3].
 *   desc[t] = {kind, cell = row * cols + col, src lo, src hi, aux lo, aux hi, p0, p1}      device int32 [n_tiles, 8]
 *     (addresses as two 32-bit words, low word first)
 *   BBD_PANEL_COLOR   src = fp32 [3,H,W] in [0,1]:  u8 = (int)(min(max(x,0),1) * 255.0f + 0.5f)  (round to nearest, so
 *                     that a frame decoded as k / 255.0f gives its file's bytes back)
 *   BBD_PANEL_WARP    src = source image fp32 [3,H,W], aux = depth fp32 [H,W], p0 = row of the pose table `pose`
 *                     [NP, BBD_POSE_STRIDE] (K | T | inv_K, as bbd_pose_expand takes it): the warp of the fused forward
 *                     - same functions of bbd_math.h in the same order, so the float that is quantised (like COLOR) is
 *                     the bit pattern bbd_warp_ssim_min_*fwd writes to `warped`.  p0 outside [0, NP), H < 2 or W < 2:
 *                     the tile is black.
 *   BBD_PANEL_SCALAR  src = fp32 [H,W], p0 = 0 plasma | 1 magma:  lut[256 * p0 + bbd_viz_lut_index(v, min, max)] with
 *                     min / max the plane's extrema without its NaNs (exact: integer maxima of order keys);
 *                     max == min and NaN take entry 0.  stats[t] = {min, max} (NaN, NaN for a plane of NaNs).
 *   BBD_PANEL_ARGMIN  src = uint8 [H,W] arg-min ids, p0 = n_T, p1 = n_E (true-pose / error-induced candidates of the
 *                     sample):  id < n_T -> palette[id];  n_T <= id < n_T + n_E -> palette[id - n_T] >> 1 per channel;
 *                     anything else (an identity candidate won: the pixel is auto-masked) -> black.
 *   lut = uint8 [BBD_PANEL_LUT_ROWS, 3]: plasma (256), magma (256), the categorical palette (20).
 * Every byte of `out` is written: cells no tile names are 0; of several tiles naming one cell the last wins; a tile
 * whose cell is outside the grid or whose kind is unknown draws nothing.  stats [n_tiles, 2] is written for SCALAR
 * tiles only.  scratch holds bbd_train_panel_scratch_ints(n_tiles) int32 and needs no initialisation.  Two launches
 * (per-tile partial extrema; the render), no atomics, no allocation, no host synchronisation: identical calls give
 * identical bytes.  A NULL pointer, a count or size below 1, H*W >= 2^31, rows*H or cols*W >= 2^31, rows*cols or
 * n_tiles > 65535 return BBD_E_BADARG and launch nothing. */
#define BBD_PANEL_DESC 8
#define BBD_PANEL_COLOR 0
#define BBD_PANEL_WARP 1
#define BBD_PANEL_SCALAR 2
#define BBD_PANEL_ARGMIN 3
#define BBD_PANEL_LUT_ROWS 532
int bbd_train_panel_scratch_ints(int n_tiles);
int bbd_train_panel(const int32_t* desc, const float* pose, const uint8_t* lut, uint8_t* out, float* stats,
                    int32_t* scratch, int n_tiles, int NP, int H, int W, int rows, int cols, void* stream);
/* counts[b][id] = number of pixels of argmin [B, n_px] (uint8) equal to id, id < BBD_MAX_CAND; larger ids are not
 * counted.  counts int32 [B, BBD_MAX_CAND] is zeroed on `stream` by the call; one launch, integer atomics (exact).
 * B <= 65535. */
int bbd_argmin_hist(const uint8_t* argmin, int32_t* counts, int B, int n_px, void* stream);

/* Checkpoint comparison sheets (csrc/bbd_compare.hip, validation.py): the two pictures that are not a disparity.  Both
 * take a ragged batch of n ground-truth maps described by BBD_EVAL_DESC rows (offset lo, hi in elements of `gt`, GH, GW,
 * crop window r0, r1, c0, c1 - the table of bbd_depth_metrics) and write picture i as uint8 RGB [GH, GW, 3] at
 * out_u8 + 3 * offset_i: the maps' packing is the pictures' packing.  A picture that starts on a 4-byte boundary gets
 * 12-byte packed stores, any other byte stores.  lut is magma, uint8 [256,3] (baseboostdepth_amd/magma_lut.hex).
 *
 * bbd_gt_viz - the colour-mapped ground truth (validation.py:250-254), for every pixel g of map i:
 *   v    = 1.0f / g                         IEEE float32 division: a zero (no LiDAR return) gives +inf
 *   v    = v > max_inv ? 0.0f : v           the reference's value of max_inv is 80
 *   vmin, vmax = minimum / maximum of v over the whole map, NaNs skipped (exact: integer maxima of order keys)
 *   rgb  = lut[bbd_viz_lut_index(v, vmin, vmax)]          vmax == vmin and NaN take entry 0
 * stats[i] = {vmin, vmax} (NaN, NaN for a map of NaNs or without pixels).  The crop window is not used.  scratch holds
 * bbd_gt_viz_scratch_ints(n) int32 and needs no initialisation.  Two launches (partial extrema; the colouring), no
 * atomics, no allocation, no host synchronisation: identical calls give identical bytes.
 *
 * bbd_error_map - where a model is wrong.  pred [n,h,w] is the scaled disparity bbd_depth_metrics was given with
 * BBD_EVAL_PRED_IS_DISP, rows [n, BBD_EVAL_OUT] that call's output (ratio and count are read on the device).  A pixel
 * (y, x) of map i is VALID when it lies inside the row's crop window and min_depth < g < max_depth in float32 - the
 * pixels bbd_depth_metrics scores - and its error is that kernel's abs_rel summand:
 *   p = bbd_eval_resample(pred[i], ..., BBD_EVAL_PRED_IS_DISP, y, x)         cv2-style resize, 1 / x, * scale_factor
 *   p *= ratio  unless flags has BBD_EVAL_NO_MEDIAN_SCALING;  p = min(max(p, min_depth), max_depth)
 *   e = fabsf(g - p) / g
 * Every output pixel takes the MAXIMUM e over the valid pixels within Chebyshev distance `radius` (0 ..
 * BBD_ERROR_MAP_MAX_RADIUS; neighbours outside the map do not exist) - a gather, so nothing depends on order - and is
 * coloured lut[bbd_viz_lut_index(e_max, 0.0f, err_max)].  A pixel without a valid neighbour takes (r + g + b) / 6
 * (integer division) of pixel (y, x) of images + 3 * offset_i (uint8 HWC at the ground-truth size) in all three
 * channels, or black when images is NULL.  A row whose count is 0 is all background.  out_float (may be NULL) receives
 * at out_float + offset_i the error e of every valid pixel and the quiet NaN 0x7fc00000 elsewhere.  One launch, no
 * scratch, no atomics.  flags may hold BBD_EVAL_NO_MEDIAN_SCALING only.
 *
 * Both return BBD_E_BADARG and launch nothing for a NULL pointer (other than the optional ones), n outside
 * [1, 65535], h or w below 1, a radius outside its range or an unknown flag. */
#define BBD_ERROR_MAP_MAX_RADIUS 4
int bbd_gt_viz_scratch_ints(int n);
int bbd_gt_viz(const float* gt, const int32_t* desc, const uint8_t* lut, uint8_t* out_u8, float* stats, int32_t* scratch,
               int n, double max_inv, void* stream);
int bbd_error_map(const float* pred, const float* gt, const int32_t* desc, const float* rows, const uint8_t* images,
                  const uint8_t* lut, uint8_t* out_u8, float* out_float, int n, int h, int w, double min_depth,
                  double max_depth, double scale_factor, double err_max, int radius, int flags, void* stream);

/* Ground-truth depth maps from Velodyne scans (kitti_utils.py:46-98, generate_depth_map), a ragged batch of n_frames
 * frames per call, written straight into a packed float32 buffer such as evaluation.GroundTruthSet keeps.
 *   points  float32 [total points, 4]: x, y, z and a fourth column that is ignored (KITTI's reflectance, which the
 *           reference overwrites with 1) - the .bin files as they are on disk, frames back to back, 16-byte aligned
 *   desc[f] = {out offset lo, hi (elements of `out`), h, w, n_points, first point, first pixel of the frame's scratch, 0}
 *   proj[f] = P_rect_0c . R_cam2rect . velo2cam, float64 [3,4] row-major
 * For every point with x >= 0, in float64 (operation order: bbd_velo_math.h): q = P (x, y, z, 1),
 * u = rint(q0/q2) - 1, v = rint(q1/q2) - 1, depth = x with BBD_VELO_VEL_DEPTH, else q2; the point is valid when
 * 0 <= u < w and 0 <= v < h.  out[v, u] is the depth of the LAST valid point on the pixel; then, for every key
 * v * (w-1) + u - 1 hit by more than one valid point, the pixel of the key's FIRST point takes the MINIMUM depth of
 * the key.  The key is the reference's sub2ind and is not unique - (r, w-1) and (r+1, 0) share one - which is
 * reproduced on purpose.  Negative depths become 0; values are the float32 casts of the float64 ones.  Every pixel of
 * every frame is written.
 * scratch holds scratch_ints = bbd_velo_depth_scratch_ints(sum of h*w, n_frames) int32 and is zeroed on `stream` by
 * the call; a frame whose tables would not fit in scratch_ints is skipped.  One memset and two launches (a point
 * sweep over ceil(max_points / 256) x n_frames workgroups, max_points >= every n_points; a pixel sweep), integer
 * atomics only: the result depends on the order of the points, not on launch geometry or scheduling.  No host
 * synchronisation.  n_frames <= 65535. */
#define BBD_VELO_DESC 8
#define BBD_VELO_VEL_DEPTH 1
int bbd_velo_depth_scratch_ints(int total_pixels, int n_frames);
int bbd_velo_depth(const float* points, const int32_t* desc, const double* proj, int32_t* scratch, int scratch_ints,
                   float* out, int n_frames, int max_points, int flags, void* stream);

/* ---- SYNS-Patches evaluation (evaluate_depth.py:26-102, :244-297; trainer.py:576-594): edge accuracy and
 * completeness, `err`, point-cloud F-score and IoU, for a ragged batch of n images per call.  Images are described by
 * the BBD_EVAL_DESC table of bbd_depth_metrics (the crop window is not used: SYNS is scored on the whole image); the
 * ground-truth edge maps are bytes (non-zero = edge) in a buffer with the SAME element offsets as the depth maps.
 * Per-image work arrays (edge maps, distance maps, scratch) are strided: image i at base + i * px_stride elements,
 * px_stride a multiple of 4 and >= max_h * max_w, max_h / max_w >= every GH / GW of the batch (they size the launch;
 * an image that does not fit px_stride is skipped).  scratch holds bbd_syns_scratch_ints(n, px_stride) int32, 16-byte
 * aligned; every entry uses it from its start, so one buffer serves the calls of a batch one after another.  The
 * arithmetic, operation by operation, is in bbd_syns_math.h (and bbd_eval_math.h for the resampled prediction);
 * everything is compiled with -ffp-contract=off.  No result depends on launch geometry or atomic order: sums are
 * integer or fp64 in an order the kernels fix, minima are over integers or over float32 values.
 *
 * bbd_syns_pred_edges: d = the prediction at every ground-truth pixel (flags 0: depth, F.interpolate bilinear then
 *   clamp to [clamp_lo, clamp_hi]; BBD_EVAL_PRED_IS_DISP: disparity, cv2-style linear resize, then 1 / x, unclamped),
 *     L   = (d > 0) * float32(log(double(max(d, 2^-23))))
 *     B   = GaussianBlur 3x3 sigma 1 of L in float32, BORDER_REFLECT_101: horizontal then vertical pass, each
 *           k1 * (a + c) + k0 * b with k = float32(exp(-x^2/2) / sum)
 *     mag = sqrt(dx^2 + dy^2), dx / dy the 5x5 Sobel of B in float64 (smoothing 1 4 6 4 1, derivative -1 -2 0 2 1)
 *     edge[i * px_stride + p] = mag > mean(mag)  (one byte, 0 / 1);  stats[i] = {mean(mag), number of edge pixels}.
 * bbd_syns_edt: out = SQUARED exact Euclidean distance of every pixel to the nearest non-zero byte of `map` (what
 *   scipy.ndimage.distance_transform_edt(1 - map) ** 2 gives), int32; BBD_SYNS_EDT_NONE (2^30) where the map has no
 *   non-zero byte.  Sizes with max_w > 8192, max_h >= 32768 or max_h^2 + max_w^2 >= 2^30 return BBD_E_TOOMANY.
 * bbd_syns_edge_metrics: with valid = min_depth < gt < max_depth, tgt = valid & gt_edge, D_t / D_p the distances to
 *   tgt / pred_edge (square roots in fp64), near = pred_edge & (D_t < th):
 *     out[i] = {edge_Acc = mean(D_t[near]), edge_comp = mean(D_p[tgt]), err = mean |p - gt| over valid,
 *               count(near), count(tgt), count(valid), count(pred_edge), 0}            (BBD_SYNS_OUT doubles)
 *   edge_Acc = edge_comp = th when near is empty, NaN when tgt is empty (scipy's input then has no background pixel).
 *   p = the prediction resampled as in bbd_depth_metrics (times scale_factor in disparity mode), times rows[i][7]
 *   (the median-scaling ratio of the bbd_depth_metrics row, read on the device) unless BBD_EVAL_NO_MEDIAN_SCALING,
 *   clamped to [min_depth, max_depth].
 * bbd_chamfer_nn: nn_a[i] = min_j |a_i - b_j|^2, nn_b[j] = min_i |a_i - b_j|^2 for a [na,3], b [nb,3] float32,
 *   d = (dx*dx + dy*dy) + dz*dz from the differences: defined to the bit; +inf where the other set is empty.
 * bbd_syns_pointcloud: pred_org = clamp(rows[i][7] * prediction, min_depth, max_depth), gt_org = gt; flat pixel k of
 *   every valid pixel becomes depth * ((iK[j][0] * u + iK[j][1] * v) + iK[j][2]), (u, v) = (k / GH, k % GH) - the
 *   reference's own pairing (torch.meshgrid(arange(w), arange(h)) in ij order against a row-major depth map) - or
 *   (k % GW, k / GW) with BBD_SYNS_RAYS_PIXEL; nearest neighbours both ways as bbd_chamfer_nn;
 *     P = count(sqrtf(nn_p) < th) / N, R likewise over nn_t, float32;  P, R < 1e-3: f = iou = P, else
 *     f = 2PR / (P + R), iou = PR / (P + R - PR);  out[i] = {f, iou, P, R, count_p, count_t, N, 0}. */
#define BBD_SYNS_OUT 8
#define BBD_SYNS_CLOUD_OUT 8
#define BBD_SYNS_RAYS_PIXEL 8
int bbd_syns_scratch_ints(int n, int px_stride);
int bbd_syns_pred_edges(const float* pred, const int32_t* desc, int32_t* scratch, int scratch_ints, uint8_t* edge,
                        double* stats, int n, int h, int w, int px_stride, int max_h, int max_w, double clamp_lo,
                        double clamp_hi, int flags, void* stream);
int bbd_syns_edt(const uint8_t* map, const int32_t* desc, int32_t* out, int n, int px_stride, int max_h, int max_w,
                 void* stream);
int bbd_syns_edge_metrics(const float* pred, const float* gt, const uint8_t* gt_edge, const uint8_t* pred_edge,
                          const int32_t* desc, const float* rows, int32_t* scratch, int scratch_ints, double* out,
                          int n, int h, int w, int px_stride, int max_h, int max_w, double min_depth,
                          double max_depth, double clamp_lo, double clamp_hi, double scale_factor, double th,
                          int flags, void* stream);
int bbd_chamfer_nn(const float* a, const float* b, int na, int nb, float* nn_a, float* nn_b, void* stream);
int bbd_syns_pointcloud(const float* pred, const float* gt, const int32_t* desc, const float* rows,
                        const float* inv_K, int32_t* scratch, int scratch_ints, float* out, int n, int h, int w,
                        int px_stride, int max_h, int max_w, double min_depth, double max_depth, double clamp_lo,
                        double clamp_hi, double th, int flags, void* stream);

/* ---- Coloured point clouds (csrc/bbd_cloud.hip, pointcloud.py): the cloud of a prediction, or of its
 * ground truth, for a ragged batch of n images per call, compacted on the device into vertices of BBD_CLOUD_VERTEX =
 * 16 bytes - x, y, z float32 little-endian, then red, green, blue, alpha - the vertex record of a binary PLY file.
 *   pred    float32 [n,h,w], depth or (BBD_EVAL_PRED_IS_DISP) disparity, resampled at every exported pixel by
 *           bbd_eval_resample exactly as bbd_depth_metrics does it (clamp_lo / clamp_hi, scale_factor as there)
 *   gt      float32 ragged buffer at the desc offsets; may be NULL unless a flag below reads it
 *   desc[i] = {offset_lo, offset_hi, GH, GW, r0, r1, c0, c1, out_lo, out_hi}            (BBD_CLOUD_DESC int32)
 *           the BBD_EVAL_DESC row of the image, then the position, in vertices, of the image's region in `vertices`.
 *           [r0,r1) x [c0,c1) is the window of pixels to export (whole image = 0,GH,0,GW; it is cut to the image)
 *   rows    float32 [n, BBD_EVAL_OUT] of bbd_depth_metrics, read on the device: rows[i][7] is the median-scaling ratio;
 *           NULL = ratio 1
 *   inv_K   float32 [n,3,3] row-major
 *   rgb     uint8 RGB images of GH x GW at rgb + 3 * offset, or NULL
 *   lut     uint8 [256,3], magma (baseboostdepth_amd/magma_lut.hex); may be NULL where rgb is given
 * The CANDIDATES of image i are the pixels (y, x) of the window with (y - r0) % stride == 0 and (x - c0) % stride == 0,
 * in raster order; their number is the capacity of the region, which the caller provides.  For a candidate:
 *   d = rows[i][7] * bbd_eval_resample(...)  (the order bbd_syns_pointcloud forms pred_org in), or, with
 *       BBD_CLOUD_FROM_GT, d = gt at the pixel
 *   kept when d is finite and min_depth <= d <= max_depth: a zero disparity gives inf and is dropped, NaN is dropped
 *       BBD_CLOUD_CLAMP    d is clamped to [min_depth, max_depth] instead (NaN is still dropped)
 *       BBD_CLOUD_MASK_GT  additionally min_depth < gt < max_depth at the pixel: the pixels the F-score scores
 *   xyz = bbd_syns_backproject(inv_K[i], k = y * GW + x, GH, GW, pixel_rays, d): the pixel's own ray (k % GW, k / GW),
 *       or with BBD_CLOUD_RAYS_REFERENCE the reference's pairing (k / GH, k % GH)
 *   rgb = the pixel's three bytes, or lut[idx] from inverse depth in float32: t = (1/d - 1/max_depth) /
 *       (1/min_depth - 1/max_depth), idx = min(max((int)(t * 256), 0), 255); alpha = 255
 * (operation by operation: csrc/bbd_cloud_math.h, -ffp-contract=off).  The kept vertices of image i are written from
 * the start of its region, contiguously, in the raster order of their pixels, each with one aligned 16-byte store;
 * counts[i] (int32) is their number.  Bytes of a region past 16 * counts[i] and bytes outside all regions are not
 * written.  `vertices` is 16-byte aligned.
 * max_h / max_w >= every GH / GW of the batch: they size the launches and the scratch, bbd_point_cloud_scratch_ints(n,
 * max_h, max_w, stride) int32 that need no initialisation; an image larger than that exports nothing (counts[i] = 0).
 * Three launches - kept candidates per chunk of 256 (64-bit ballot, population count), a prefix sum of every image's
 * chunk totals, the write pass - no atomics, no allocation, no host synchronisation; integer sums only, so nothing
 * depends on launch geometry and identical calls give identical bytes.
 * A NULL required pointer, n, h, w, max_h, max_w or stride below 1, an unknown flag bit, a flag that reads gt with gt
 * NULL, vertices not 16-byte aligned or scratch_ints too small return BBD_E_BADARG; n > 65535, max_h * max_w >
 * 2^31 - 257 or a scratch size beyond int32 return BBD_E_TOOMANY.  Nothing is launched then. */
#define BBD_CLOUD_DESC 10
#define BBD_CLOUD_VERTEX 16
#define BBD_CLOUD_FROM_GT 16
#define BBD_CLOUD_CLAMP 32
#define BBD_CLOUD_MASK_GT 64
#define BBD_CLOUD_RAYS_REFERENCE 128
int bbd_point_cloud_scratch_ints(int n, int max_h, int max_w, int stride);
int bbd_point_cloud(const float* pred, const float* gt, const int32_t* desc, const float* rows, const float* inv_K,
                    const uint8_t* rgb, const uint8_t* lut, void* vertices, int32_t* counts, int32_t* scratch,
                    int scratch_ints, int n, int h, int w, int max_h, int max_w, int stride, double min_depth,
                    double max_depth, double clamp_lo, double clamp_hi, double scale_factor, int flags, void* stream);

/* ---- Metric scale from the ground plane (csrc/bbd_ground.hip, ops.ground_scale): the factor that brings
 * a prediction of unknown scale to metres, from the known height of the camera above the road, for n images per call.
 *   pred    float32 [n,h,w], depth or (BBD_EVAL_PRED_IS_DISP) disparity: d = pred or 1.0f / pred; a pixel is valid
 *           when d > 0 and finite
 *   inv_K   float32 [n,3,3] row-major, for pixels of the h x w map itself
 *   rows    float32 [n, BBD_EVAL_OUT], written: [0] median distance of the ground pixels' planes from the camera, in the
 *           prediction's units, [1] their number, [2] the number of candidates, [7] camera_height / median - the slot
 *           bbd_point_cloud reads as its ratio - all others 0.  Where the count is below max(min_count, 1), [0] and [7]
 *           are the quiet NaN 0x7fc00000; the counts are written all the same
 *   mask    uint8 [n,h,w] or NULL: 1 at ground pixels, 0 elsewhere, the border included
 *   scratch float32 [bbd_ground_scale_scratch_floats(n, h, w)] = n * h * w, no initialisation needed
 * P = bbd_syns_backproject(inv_K[i], y * w + x, h, w, pixel rays, d).  A CANDIDATE is an interior pixel (1 <= x <= w-2,
 * 1 <= y <= h-2) whose nine pixels are all valid; maps with h < 3 or w < 3 have none.  Its normal N is the sum, in ring
 * order, of the cross products v_k x v_(k+1) of the differences v_k = P_k - P_c to its eight neighbours (x+1,y),
 * (x+1,y+1), (x,y+1), (x-1,y+1), (x-1,y), (x-1,y-1), (x,y-1), (x+1,y-1): +y for flat ground under a camera with x right,
 * y down, z forward.  With len = sqrtf((N.x*N.x + N.y*N.y) + N.z*N.z), cosv = N.y / len and
 * ht = ((N.x*P.x + N.y*P.y) + N.z*P.z) / len, the pixel is GROUND when len > 0 and finite, cosv > (float)cos_threshold,
 * P.y > 0 and ht > 0 and finite.  The median is the element of rank (count - 1) / 2 of the ascending ht values (the
 * lower median, exact).  All float32, one IEEE operation where written (csrc/bbd_ground_math.h, -ffp-contract=off).
 * Two launches - a tiled pass that stages the depths of a tile and a one-pixel halo in LDS and writes one float per pixel
 * to the scratch map, then one workgroup per image that takes the median by an 11+11+10-bit radix select on the bit
 * patterns and writes the row - no allocation, no host synchronisation, integer counts only: identical calls give
 * identical bytes.
 * A NULL pred, inv_K, rows or scratch, n, h or w below 1, camera_height not above 0, cos_threshold outside (0, 1],
 * min_count below 0 or a flag other than BBD_EVAL_PRED_IS_DISP return BBD_E_BADARG; n > 65535 or h * w > INT_MAX
 * return BBD_E_TOOMANY.  Nothing is launched then; the size helper returns the same codes for such sizes. */
long bbd_ground_scale_scratch_floats(int n, int h, int w);
int bbd_ground_scale(const float* pred, const float* inv_K, float* rows, uint8_t* mask, float* scratch, int n, int h,
                     int w, double camera_height, double cos_threshold, int min_count, int flags, void* stream);

/* ---- Scene map (csrc/bbd_map.hip, pointcloud.SceneMap): the points of many frames, each placed in the
 * world by its camera-to-world pose, fused on a voxel grid into one coloured cloud.  A streaming accumulator: the state
 * is the caller's, an open-addressing hash table of T slots, T a power of two up to 2^30:
 *   keys      uint64 [T]     voxel key of the slot, empty = all ones
 *   pos       uint64 [T,3]   sums of the points' fixed-point offsets inside the voxel (16 fractional bits), x y z
 *   col       uint32 [T,4]   sum of red, green, blue bytes, number of points; 16-byte aligned
 *   counters  int64 [BBD_MAP_COUNTERS] = {candidates, kept, out-of-range drops, table-full drops}, running totals
 * bbd_map_state_bytes(T) = T * BBD_MAP_SLOT_BYTES + 8 * BBD_MAP_COUNTERS, the bytes of the four buffers together.
 *
 * bbd_map_clear: every key empty, sums and counters zero.  One launch.
 *
 * bbd_map_accumulate adds n frames.  One launch, a lane per candidate.
 *   disp    float32 [n,h,w]: the network's scaled disparity (depth = 1 / disp), or, with BBD_MAP_INPUT_IS_DEPTH, depth
 *   rgb     float32 [n,3,h,w] in [0,1]
 *   poses   float64 [n,16] row-major 4x4, camera to world
 *   inv_K   float32 [3,3] row-major
 *   scale   DEVICE pointer to one double that multiplies depth and camera-frame point (bbd_pose_trajectory's
 *           summary + 6), or NULL = 1
 *   [r0,r1) x [c0,c1) is the window of pixels (it is cut to the image); the CANDIDATES are its pixels (y, x) with
 *   (y - r0) % stride == 0 and (x - c0) % stride == 0.  For a candidate, k = y * w + x:
 *     d = 1.0f / disp (or disp), float32;  x = bbd_syns_backproject(inv_K, k, h, w, pixel rays, d), float32
 *     dm = scale * (double)d: the candidate is REJECTED unless dm is finite and min_depth <= dm <= max_depth (the limits
 *       are in world units; a zero or NaN disparity and a NaN scale are rejected here)
 *     X = R (scale * (double)x) + t in float64, three-term sums left to right
 *     per axis u = X / voxel, v = floor(u), q = (uint32)((u - v) * 65536.0); a non-finite X or |v| >= 2^20 on any axis:
 *       the point is dropped and counted OUT OF RANGE
 *     key = ((v_x + 2^20) << 42) | ((v_y + 2^20) << 21) | (v_z + 2^20)
 *     colour byte = min(max((int)(c * 255.0f + 0.5f), 0), 255) per channel
 *   (operation by operation: csrc/bbd_map_math.h, -ffp-contract=off).  The point's slot is found by linear probing from
 *   mix(key) & (T - 1) - mix = splitmix64's finaliser: z ^= z >> 30, z *= 0xbf58476d1ce4e5b9, z ^= z >> 27,
 *   z *= 0x94d049bb133111eb, z ^= z >> 31 - with a 64-bit compare-and-swap on keys; at most T slots are visited, a point
 *   that finds none is dropped and counted TABLE FULL.  On the slot q_x q_y q_z are added to pos and r, g, b, 1 to col
 *   with integer atomic adds: the sums do not depend on the order of arrival, the slot a key occupies does.
 *   Neighbouring candidates of a wave that fall into one voxel are summed in registers first and added once; with
 *   BBD_MAP_NO_MERGE every point adds for itself.  The state's bytes are the same either way (profiles/map/README.md).
 *   counters: candidates += n * candidates per frame, kept += points added, and the two drop counts.
 *   A voxel takes fewer than 2^24 points (the colour sums are 32 bits).
 *
 * bbd_map_finish compacts the occupied slots with count >= min_points, in slot order, into
 *   out_keys  int64 [T]: the voxel keys (below 2^63), so that the caller can order the voxels; keys are unique
 *   vertices  [T] records of BBD_CLOUD_VERTEX bytes, 16-byte aligned: per axis
 *             (float)((v + ((double)sum_q / count + 0.5) / 65536.0) * voxel), per channel (sum + count / 2) / count in
 *             integers, alpha 255
 *   out_counts int32 [T]; m int32 [1]: the number of records M.  Records past M are not written.
 *   scratch   int32 [bbd_map_finish_scratch_ints(T)], no initialisation
 * Three launches, the compaction of bbd_point_cloud (csrc/bbd_compact.h).  The state is only read: accumulation may go
 * on afterwards.  `voxel` is the one the points were accumulated with.
 *
 * No allocation, no host synchronisation.  A NULL required pointer, T, n, h, w, stride or min_points below 1, T not a
 * power of two, voxel not positive and finite, min_depth > max_depth (or a NaN limit), col or vertices not 16-byte
 * aligned, scratch_ints too small or an unknown flag bit return BBD_E_BADARG; T > 2^30 or n * h * w > INT_MAX return
 * BBD_E_TOOMANY.  Nothing is launched then.  The size helpers return the same codes. */
#define BBD_MAP_INPUT_IS_DEPTH 1
#define BBD_MAP_NO_MERGE 2
#define BBD_MAP_COUNTERS 4
#define BBD_MAP_SLOT_BYTES 48
#define BBD_MAP_MAX_T 1073741824 /* 2^30: the largest table */
long bbd_map_state_bytes(int T);
int bbd_map_finish_scratch_ints(int T);
int bbd_map_clear(uint64_t* keys, uint64_t* pos, uint32_t* col, int64_t* counters, int T, void* stream);
int bbd_map_accumulate(uint64_t* keys, uint64_t* pos, uint32_t* col, int64_t* counters, int T, const float* disp,
                       const float* rgb, const double* poses, const float* inv_K, const double* scale, int n, int h,
                       int w, int r0, int r1, int c0, int c1, int stride, double min_depth, double max_depth,
                       double voxel, int flags, void* stream);
int bbd_map_finish(const uint64_t* keys, const uint64_t* pos, const uint32_t* col, int T, int min_points, double voxel,
                   int64_t* out_keys, void* vertices, int32_t* out_counts, int32_t* m, int32_t* scratch,
                   int scratch_ints, void* stream);

/* ---- Depth-pose geometric consistency (csrc/bbd_consist.hip, ops.depth_consistency): does the depth of
 * a frame agree with the depth of its neighbours under the predicted motion?  A pixel of reference frame i is
 * back-projected with its depth, moved into source frame j with inv(P_j) . P_i and projected; the depth z it has there is
 * compared with the depth d_b frame j predicts at that place: err = |z - d_b| / (z + d_b), in [0, 1].  One call, two
 * launches (the pairs' transforms, then a lane per reference pixel), no scratch: every buffer is the caller's and its
 * size is written here.
 *   disp        float32 [n,h,w]: the network's scaled disparity (depth = 1 / disp), or, with
 *               BBD_CONSIST_INPUT_IS_DEPTH, depth.  A value is VALID when its depth is above 0 and finite
 *   poses       float64 [n,16] row-major 4x4, camera to world (the rows of bbd_pose_trajectory's aligned trajectory)
 *   scale       DEVICE pointer to one double that multiplies depth and camera-frame point, or NULL = 1: the same meaning
 *               as in bbd_map_accumulate
 *   K, inv_K    float32 [3,3] row-major, of the h x w map
 *   sources     int32 [n,V] on the device, 1 <= V <= BBD_CONSIST_MAX_VIEWS: row i lists the frames that frame i is
 *               checked against, -1 = none.  The table lives on the device and cannot be checked on the host: an entry
 *               outside [-1, n) is treated as -1
 *   transforms  OUT float64 [n,V,12]: rows 0..2 of inv(P_src) . P_ref of every listed pair - the general inverse of the
 *               odometry evaluation (Gauss-Jordan, partial pivoting), then the 4x4 product, each entry
 *               ((a0 b0 + a1 b1) + a2 b2) + a3 b3; twelve zeros where there is no source.  Written by the first launch,
 *               read by the second
 *   seen        OUT uint8 [n,h,w]: the number of sources in which the pixel is visible
 *   agree       OUT uint8 [n,h,w]: the number of sources in which it is visible and err < threshold (strict: threshold
 *               0 keeps nothing)
 *   err         OUT float32 [n,h,w] or NULL: the smallest err over the visible sources; none: the quiet NaN 0x7fc00000
 *   filtered    OUT float32 [n,h,w] or NULL: disp where the pixel is VALID and agree >= min_views, else 0 - also under
 *               the depth flag.  bbd_map_accumulate turns a disparity of 0 into an infinite depth and rejects it, so the
 *               map takes `filtered` in the place of `disp` as it is
 *   counters    OUT int64 [n,BBD_CONSIST_COUNTERS], cleared by the call: per frame {VALID pixels, visible samples,
 *               agreeing samples, sum over visible samples of (int64)((double)err * 16777216.0 + 0.5), pixels kept}.
 *               Integer sums: identical calls give identical bytes, whatever the launch geometry
 * For pixel k = y * w + x of frame i (operation by operation: csrc/bbd_consist_math.h, -ffp-contract=off):
 *   d = 1.0f / disp (or disp), float32;  p = bbd_syns_backproject(inv_K, k, h, w, pixel rays, d), float32 - the point the
 *   scene map fuses;  q = scale * (double)p;  per source X = M q + t in float64, three-term sums left to right, z = X_2;
 *   c = K X likewise, u = c_0 / c_2, t = c_1 / c_2.  The sample is VISIBLE when z > 0 and finite, 0 <= u <= w - 1,
 *   0 <= t <= h - 1 and the four taps at x0 = min(floor(u), w - 2), y0 = min(floor(t), h - 2) are VALID (maps with h < 2
 *   or w < 2 have no visible samples).  The INVERSE depth of the source is sampled bilinearly in float64,
 *   s = top + fy (bot - top) with top = s00 + fx (s01 - s00) - it is affine in the pixel on a plane, depth is not -
 *   d_b = scale / s (above 0 and finite, else not visible), err = (float)(fabs(z - d_b) / (z + d_b)).
 * No transcendental function appears, so a correctly rounding host gives the device's bits.
 *
 * No allocation, no host synchronisation.  A NULL required pointer (all but scale, err and filtered), n, h, w or V below
 * 1, V above BBD_CONSIST_MAX_VIEWS, min_views below 0, a negative or NaN threshold or an unknown flag bit return
 * BBD_E_BADARG; n * h * w > INT_MAX returns BBD_E_TOOMANY.  Nothing is launched then. */
#define BBD_CONSIST_INPUT_IS_DEPTH 1
#define BBD_CONSIST_MAX_VIEWS 8
#define BBD_CONSIST_COUNTERS 5
int bbd_depth_consistency(const float* disp, const double* poses, const double* scale, const float* K,
                          const float* inv_K, const int32_t* sources, double* transforms, uint8_t* seen, uint8_t* agree,
                          float* err, float* filtered, int64_t* counters, int n, int h, int w, int V, double threshold,
                          int min_views, int flags, void* stream);

/* ---- Geometry-consistency loss for training (csrc/bbd_geo.hip, ops.geometry_consistency; Bian et al.,
 * NeurIPS 2019): the err of bbd_depth_consistency as a differentiable loss between a target frame and V source frames of
 * the SAME batch, with gradients to both inverse-depth maps and to the pose.  Everything float32 on the device:
 *   q_tgt       [B,H,W]    inverse depth of the target frames (the scaled disparity min_disp + (max_disp - min_disp) disp)
 *   q_src       [V,B,H,W]  the same of each source frame, 1 <= V <= BBD_GEO_MAX_VIEWS
 *   T           [V,B,12]   rows 0..2 of the target-to-source 4x4 matrix, row-major
 *   K, inv_K    [B,16]     4x4 row-major as the batch dictionary holds them; the 3x3 parts are read
 * Per target pixel (x, y) and source (operation by operation: csrc/bbd_geo_math.h, -ffp-contract=off, float32, one IEEE
 * operation where written, no transcendental function): p = inv_K [x, y, 1] / q_tgt;  X = R p + t, z = X_2;  c = K X,
 * u = c_0 / c_2, t = c_1 / c_2.  The sample is VISIBLE when q_tgt > 0 and finite, z finite and above 0.001,
 * 0 <= u <= W - 1, 0 <= t <= H - 1, the four taps at x0 = min(floor(u), W - 2), y0 = min(floor(t), H - 2) above 0 and finite
 * (H < 2 or W < 2: nothing is visible), the bilinear sample s of the source's inverse depth at least 2^-10 and a = z s
 * finite.  e = |a - 1| / (a + 1).
 *   bbd_geo_fwd
 *   pair_sum    OUT float64 [V,B]: the sum of e over the pair's visible samples - the integer sum of
 *               floor(e 2^36 + 0.5), times 2^-36: order-free
 *   pair_count  OUT int64 [V,B]: its visible samples
 *   err         OUT float32 [V,B,H,W] or NULL: e, 0 where not visible
 *   code        OUT uint8 [V,B,H,W] or NULL: bit 0 = visible, bit 1 = a > 1
 *   scratch     8-byte words, at least B * items * V * 2 with items = ceil(H * W / BBD_GEO_RUN); need not be cleared
 *   bbd_geo_bwd
 *   g           float64 [V,B] ON THE DEVICE: the upstream gradient of pair_sum
 *   grad_q_tgt  OUT float32 [B,H,W]: summed over a pixel's sources in the pixel's lane, in source order
 *   grad_q_src  OUT float32 [V,B,H,W]: a scatter, added as 64-bit integers of fixed point 2^30 (vector atomics, order-free)
 *               and converted once.  |de/ds| <= 1 / (2 s) <= 2^9 by the rule s >= 2^-10, a map has at most 2^23 pixels: the
 *               sums cannot leave the 64-bit range
 *   grad_T      OUT float32 [V,B,12]: float64 partial sums per work item in a fixed layout, added in a fixed order
 *   scratch     8-byte words, at least V * B * H * W + B * items * V * 12; cleared by the call
 * Identical calls give identical bytes in every output, and the host port gives the device's bytes.
 *
 * No allocation, no host synchronisation.  A NULL required pointer (all but err and code), B, H, W or V below 1, V above
 * BBD_GEO_MAX_VIEWS or scratch_words below the formula return BBD_E_BADARG; H * W > 2^23 or V * B * H * W > INT_MAX return
 * BBD_E_TOOMANY.  Nothing is launched or written then. */
#define BBD_GEO_MAX_VIEWS 8
#define BBD_GEO_RUN 2048
int bbd_geo_fwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                double* pair_sum, int64_t* pair_count, float* err, uint8_t* code, int64_t* scratch, long scratch_words,
                int B, int H, int W, int V, void* stream);
int bbd_geo_bwd(const float* q_tgt, const float* q_src, const float* T, const float* K, const float* inv_K,
                const double* g, float* grad_q_tgt, float* grad_q_src, float* grad_T, int64_t* scratch,
                long scratch_words, int B, int H, int W, int V, void* stream);

/* ---- Semi-global stereo matching (csrc/bbd_sgm.hip, ops.stereo_hints, --depth_hints; Hirschmueller, PAMI
 * 2008; Watson et al., ICCV 2019): a proxy disparity in 1/16 pixel for every pixel of a rectified pair.
 *   left, right  float32 [B,3,H,W] in [0,1]: the frame and its stereo partner
 *   side         int32 [B]: 0 = the partner lies to the right, matches at x - d; otherwise the roles are mirrored (the
 *                frame is the right camera's, or the sample was flipped), matches at x + d.  A mirrored image is matched
 *                through an index reflection of its loads and of its store: it gives the mirror image of what the
 *                mirrored inputs give with side 0
 *   disp16       OUT int16 [B,H,W]: 16 times the disparity, BBD_SGM_INVALID where the pixel failed a check
 *   valid_count  OUT int64 [B]: the pixels that passed every check (before the fill): integer sums per workgroup and one
 *                integer atomic add each, order-free
 *   scratch      caller-owned, 8-byte aligned, at least bbd_sgm_scratch_bytes(B, H, W, D, paths) bytes
 *                (include/bbd_sgm.h): grey bytes, census words, the cost volume as uint8, the path sums S as uint16 and
 *                one selection word a pixel.  Need not be cleared
 *   D            disparities 0 .. D - 1: 64, 128, 192 or 256;  paths  4 or 8
 *   p1, p2       the penalties of the path recurrence, 1 <= p1 < p2 <= BBD_SGM_MAX_P2 (the bound that keeps 8 paths of
 *                62 + p2 inside uint16); BBD_SGM_P1 / BBD_SGM_P2 are the defaults of the Python layer
 *   uniqueness   OpenCV's uniquenessRatio in percent, 0 .. 99, 0 = no test;  fill  0 or 1: invalid pixels take the
 *                nearest valid value of their row (smaller x first, in matching coordinates)
 * The rules - grey, the 9 x 7 census, the Hamming cost, the recurrence, winner takes all with ties to the lowest d, the
 * left-right check, the sub-pixel division - are csrc/bbd_sgm_math.h, shared with the host port.  Integer arithmetic:
 * identical calls give identical bytes, and the host port gives the device's bytes.  No allocation, no host
 * synchronisation.  A NULL pointer, a shape, D, paths, penalty, uniqueness or fill outside the above, a scratch that is
 * misaligned or too small return BBD_E_BADARG; more than BBD_SGM_MAX_BATCH images or 2^26 pixels return BBD_E_TOOMANY.
 * Nothing is launched or written then. */
#define BBD_SGM_MAX_P2 8129
#define BBD_SGM_P1 10
#define BBD_SGM_P2 120
#define BBD_SGM_UNIQUENESS 5
#define BBD_SGM_INVALID (-16)
int bbd_sgm_hints(const float* left, const float* right, const int32_t* side, int16_t* disp16, int64_t* valid_count,
                  void* scratch, long scratch_bytes, int B, int H, int W, int D, int paths, int p1, int p2, int uniqueness,
                  int fill, void* stream);

/* ---- Views (csrc/bbd_view.hip, pointcloud.Canvas): points and polylines rasterised into a z-buffered
 * canvas, resolved to RGB bytes.  The canvas is the caller's:
 *   cells     uint64 [H,W]   one key per pixel, empty = all ones
 *   counters  int64 [BBD_VIEW_COUNTERS] = {offered, drawn, clipped, rejected} points, running totals
 * A key is rank << 32 | colour, colour = r << 24 | g << 16 | b << 8 | 0xff.  The rank of a point at view depth d > 0 is
 * 0x80000000 | (bits((float)d) >> 1); the rank of an overlay primitive is 0x7fffffff - layer, 0 <= layer < 2^16.  Every
 * write is an unsigned 64-bit atomic minimum, so the finished canvas does not depend on the order of lanes, launches or
 * calls: the nearer point wins, every overlay beats every point, a higher layer beats a lower one, an exact tie goes to
 * the smaller colour word.
 *
 * A world position (x, y, z) is projected by `view`, a DEVICE float64 row-major 4x4, in float64:
 *   p_r = ((V[4r] x + V[4r+1] y) + V[4r+2] z) + V[4r+3];  u = p_0 / p_3, v = p_1 / p_3, d = p_2
 * (an orthographic view has the last row 0 0 0 1; a perspective view repeats row 3 in row 2).  It is REJECTED when any
 * of u, v, d, p_3 is not finite (p_3 = 0 is: the quotients are not finite), else BEHIND when p_3 <= 0 or d <= 0.
 * Operation by operation: csrc/bbd_view_math.h, -ffp-contract=off.
 *
 * bbd_view_clear: every cell empty, the counters zero.  One launch.
 *
 * bbd_view_points draws the first min(*count, n_max) records of `vertices` (BBD_CLOUD_VERTEX bytes each: x y z float32,
 *   then r g b a; 16-byte aligned), all n_max with count = NULL.  `count` is a DEVICE int32 read by the kernel; records
 *   past it are never read.  A point that is not rejected or behind covers the size x size pixels centred on pixel
 *   (floor(u), floor(v)), size in {1, 3, 5, 7}, cut to the canvas; it is CLIPPED when it is behind or the square misses
 *   the canvas, else DRAWN.  counters: offered += records visited, and one of drawn, clipped, rejected per record.
 *   One launch, a lane per record; nothing is launched for n_max = 0.
 *
 * bbd_view_lines draws the polyline through the P world positions xyz (float64 [P,3]) as an overlay of one colour
 *   (rgb = r | g << 8 | b << 16) and layer: P - 1 segments, one more back to the first vertex with closed = 1 and P > 2.
 *   P = 1 and a segment of no length draw a disc.  A segment with an end that is rejected or behind is skipped.  Pixel
 *   (i, j) is painted when the squared distance of (i + 0.5, j + 0.5) from the projected segment is <= (width / 2)^2.
 *   One launch, a wave per segment; a segment costs its bounding box cut to the canvas.  The counters are the points':
 *   they are left as they are.
 *
 * bbd_view_resolve writes out uint8 [H,W,3]: the colour of every cell, background_rgb (r | g << 8 | b << 16) where it
 *   is empty.  One launch; the cells are only read.
 *
 * No allocation, no host synchronisation.  A NULL pointer (other than count), H or W below 1, n_max below 0, P below 1,
 * vertices not 16-byte aligned, a size other than 1, 3, 5, 7, a width that is not positive and finite, a layer outside
 * [0, 65535], a colour outside [0, 0xffffff] or closed other than 0 or 1 return BBD_E_BADARG; H * W > 2^28 returns
 * BBD_E_TOOMANY.  Nothing is launched then. */
#define BBD_VIEW_COUNTERS 4
#define BBD_VIEW_MAX_CELLS 268435456 /* 2^28: the largest canvas, H * W */
#define BBD_VIEW_MAX_LAYER 65535
int bbd_view_clear(uint64_t* cells, int64_t* counters, int H, int W, void* stream);
int bbd_view_points(uint64_t* cells, int64_t* counters, int H, int W, const void* vertices, const int32_t* count,
                    int n_max, const double* view, int size, void* stream);
int bbd_view_lines(uint64_t* cells, int64_t* counters, int H, int W, const double* xyz, int P, const double* view,
                   int rgb, double width, int layer, int closed, void* stream);
int bbd_view_resolve(const uint64_t* cells, int H, int W, int background_rgb, uint8_t* out, void* stream);

/* Flip post-processing of predicted disparities (Monodepth2's batch_post_process_disparity; evaluate_depth.py
 * --post_process), n images per call.
 *   disp  float32 [2n,h,w]: rows 0..n-1 are the predictions for n images, rows n..2n-1 the predictions for the same
 *         images flipped left-right, STILL flipped (they are read mirrored, never flipped back in memory)
 *   out   float32 [n,h,w]; must not overlap disp
 * With ld = disp[i][y][x], rd = disp[n+i][y][w-1-x], m = (ld + rd) * 0.5f in float32, l = np.linspace(0, 1, w) and
 * lm(x) = 1 - clip(20 * (l[x] - 0.05), 0, 1), a = lm(x), b = lm(w-1-x) in float64:
 *   out[i][y][x] = (float)((b * ld + a * rd) + ((1 - a) - b) * m)
 * - the float64 blend of the reference rounded once to float32 (operation order: csrc/bbd_postproc_math.h).  One
 * launch, no LDS, no atomics, no host synchronisation; identical calls give identical bytes.  A NULL pointer or n, h
 * or w below 1 returns BBD_E_BADARG and launches nothing. */
int bbd_post_process_disp(const float* disp, float* out, int n, int h, int w, void* stream);

/* ---- Depth uncertainty from the flip pass and its sparsification scores (csrc/bbd_uncert.hip, ops.post_process_uncert,
 * ops.sparsification; Poggi et al., CVPR 2020).  Arithmetic and the order of every addition:
 * csrc/bbd_uncert_math.h.
 *
 * bbd_post_process_uncert - bbd_post_process_disp with one more plane, in ONE launch: `out` has the bytes that call
 * writes, and uncert [n,h,w] = fabsf(disp[i][y][x] - disp[n+i][y][w-1-x]), one float32 subtraction ("Post").  A NULL
 * pointer or n, h or w below 1 returns BBD_E_BADARG and launches nothing.
 *
 * bbd_sparsification - how good is an uncertainty map?  pred and uncert are float32 [n,h,w]: the scaled disparity
 * bbd_depth_metrics was given with BBD_EVAL_PRED_IS_DISP and its uncertainty; gt, desc and rows are what bbd_error_map
 * takes (rows [n, BBD_EVAL_OUT]: rows[i][7], the median-scaling ratio, is read on the device).  The pixels of image i are
 * the N pixels bbd_depth_metrics scores (inside the crop window cut to the map, min_depth < g < max_depth in float32),
 * in the order of y * GW + x.  Per pixel, in float32:
 *   p = bbd_eval_resample(pred[i], ..., BBD_EVAL_PRED_IS_DISP, y, x) [* ratio unless BBD_EVAL_NO_MEDIAN_SCALING], clamped
 *   df = g - p;  e_abs = fabsf(df) / g;  e_sq = df * df;  th = max(g / p, p / g);  a1 = th < 1.25f
 *   u = the cv2-style linear resize of uncert[i] at (y, x): the taps and weights of the disparity, no reciprocal
 * Four orderings of the N pixels - by u, e_abs, e_sq, th - each by the monotone order key of the float (every NaN first
 * made 0x7fc00000, -0 made +0: a NaN ranks above +inf) DESCENDING, pixel order ascending among equal keys.  With
 * K = intervals and r_k = floor(k * N / K), S_k is what remains after the first r_k pixels of an ordering, and
 *   abs_rel_k = sum(e_abs) / |S_k|   rmse_k = sqrt(sum(e_sq) / |S_k|)   a1_k = #a1 / |S_k|       k < K, in float64
 * point K is 0, 0, 1; trapz(c) = (sum over k < K of (c_k + c_(k+1)) / 2) / K.  `sparse` is a metric's curve under the u
 * ordering, `oracle` under its own.  out is float64 [n, BBD_SPARS_SUMMARY + 6 * (K + 1)]:
 *   {AUSE abs_rel, AUSE rmse, AUSE a1, AURG abs_rel, AURG rmse, AURG a1, N, 0}, then curves [2: sparse, oracle][3][K + 1]
 *   AUSE = trapz(sparse) - trapz(oracle), AURG = sparse_0 - trapz(sparse); both signs flipped for a1 (higher is better)
 * An image with N = 0 gets quiet NaNs with N = 0; a NaN prediction propagates as in bbd_depth_metrics.  The sums are
 * float64 in an order that depends on N and K alone, the sort is a stable segmented radix sort: no atomics on floats or
 * on positions, no allocation, no host synchronisation - identical calls give identical bytes.
 *
 * scratch is the caller's, 8-byte aligned, needs no initialisation, and scratch_bytes states its capacity - the call
 * cannot read the windows on the host:
 *   scratch_bytes = BBD_SPARS_SCRATCH_CALL + n * BBD_SPARS_SCRATCH_IMAGE + P * BBD_SPARS_SCRATCH_PIXEL
 * with P at least the sum over the n desc rows of the area of the crop window cut to the map,
 * max(0, min(r1, GH) - max(r0, 0)) * max(0, min(c1, GW) - max(c0, 0)).  A scratch_bytes that is not of this form for a
 * whole P >= 0 is refused.  Launches are sized by P; should the windows on the device exceed P, nothing is sorted and
 * every row is NaN, N included.
 *
 * Returns BBD_E_BADARG and launches nothing for a NULL pointer, n outside [1, 65535], h or w below 1, intervals outside
 * [1, BBD_SPARS_MAX_INTERVALS], a flag other than BBD_EVAL_NO_MEDIAN_SCALING, a scratch that is misaligned or too small
 * (not of the form above) or P beyond 2^31 - 2049. */
#define BBD_SPARS_MAX_INTERVALS 100
#define BBD_SPARS_SUMMARY 8
#define BBD_SPARS_SCRATCH_PIXEL 81
#define BBD_SPARS_SCRATCH_IMAGE 8916
#define BBD_SPARS_SCRATCH_CALL 128
int bbd_post_process_uncert(const float* disp, float* out, float* uncert, int n, int h, int w, void* stream);
int bbd_sparsification(const float* pred, const float* uncert, const float* gt, const int32_t* desc, const float* rows,
                       double* out, void* scratch, long scratch_bytes, int n, int h, int w, int intervals,
                       double min_depth, double max_depth, double scale_factor, int flags, void* stream);

/* ---- Affine-invariant depth evaluation (csrc/bbd_align.hip, evaluation.depth_metrics_affine): the protocol
 * of the relative-depth models (MiDaS, DPT, Depth Anything), whose prediction is a disparity up to an unknown scale AND
 * shift.  Arithmetic and the order of every addition: csrc/bbd_align_math.h.
 *
 * pred is float32 [n,h,w], a disparity-like map in any affine gauge; gt and desc are the ragged ground truth and the
 * BBD_EVAL_DESC table of bbd_depth_metrics.  The pixels of image i are the N pixels bbd_depth_metrics scores (inside the
 * crop window cut to the map, min_depth < g < max_depth in float32).  Per pixel
 *   x = the cv2-style linear resize of pred[i] at (y, x), float32: no reciprocal, no scale factor;  t = 1.0 / (double)g
 * and, in float64, the centred two-sweep least squares of t on x:
 *   mx = sum x / N, mt = sum t / N;  scale = sum (x - mx)(t - mt) / sum (x - mx)^2;  shift = mt - scale * mx
 *   a = scale * x + shift;  a = a < 1 / max_depth ? 1 / max_depth : a      the disparity cap: a pixel the fit sends to
 *                                                                          zero or below is scored at max_depth
 *   p = (float)(1.0 / a), clamped to [min_depth, max_depth] in float32
 * then the seven summands of bbd_depth_metrics (float32 operations, float64 sums) and, with d = logf(p) - logf(g),
 *   silog = 100 sqrt(max(sum d^2 / N - (sum d / N)^2, 0))      irmse = 1000 sqrt(sum (1/p - 1/g)^2 / N)   (1/km for metres)
 * out is float64 [n, BBD_ALIGN_OUT]:
 *   {abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, scale, shift, silog, count N, irmse}
 * An image with N < 2 or max x == min x is degenerate: quiet NaNs, the count kept (0 where nothing is scored).  A
 * non-finite x among the scored pixels is not caught: it makes the fit, and with it every column but the count, NaN.
 * One 1024-thread workgroup per image, three sweeps, no scratch, no atomics, no host synchronisation; every float64 sum
 * is taken in an order that depends on the window alone - identical calls give identical bytes.
 *
 * flags must be 0.  Returns BBD_E_BADARG and launches nothing for a NULL pointer, n <= 0, h or w below 1, a flag, or
 * unless 0 <= min_depth < max_depth. */
#define BBD_ALIGN_OUT 12
int bbd_depth_metrics_affine(const float* pred, const float* gt, const int32_t* desc, double* out, int n, int h, int w,
                             double min_depth, double max_depth, int flags, void* stream);

/* ---- KITTI odometry evaluation (evaluate_pose.py:18-41, :101-116, :125-159): everything after the pose
 * network, for all windows of a sequence in one call - three small launches, no host synchronisation, no atomics
 * (identical calls give identical bytes).  Arithmetic and its order: csrc/bbd_odom_math.h.
 *   poses    float32 [1+S, N, 16]: section 0 = the direct pose of window i (frames i, i+S); section 1+k = the single-step
 *            pose of frames (i+k, i+k+1), k = 0..S-1
 *   gt       float64 [M, 12]: the rows of the KITTI poses file (3x4, row-major); (0 0 0 1) is appended here
 *   chained  float32 [N, 16] out: step_{S-1} @ ... @ step_0, rounded like torch.matmul on the CPU
 *   gt_local float64 [M-S, 16] out: inv(inv(G[j]) . G[j+S]) with a general (Gauss-Jordan, partial pivoting) inverse
 *   ates     float64 [2, N-S] out: row 0 direct, row 1 chained; track i takes min(L, N-i) poses; 0/0 stays NaN
 *   summary  float64 [2, 4] out: mean, population std, count, 0 per row; NaN when count == 0 or a track is NaN
 * S < 1, L < 1, N < 0 or N > M - S return BBD_E_BADARG.  An output without elements may be NULL. */
int bbd_pose_ate(const float* poses, const double* gt, float* chained, double* gt_local, double* ates, double* summary,
                 int N, int M, int S, int L, void* stream);

/* ---- KITTI odometry, the whole trajectory: the trajectory chained from the network's single steps, its
 * alignment to ground truth, the ATE of the aligned trajectory and the devkit's sub-sequence errors (calcSequenceErrors)
 * in one call - four small launches on `stream`, no allocation, no host synchronisation, no atomics (identical calls
 * give identical bytes).  Arithmetic and its order: csrc/bbd_traj_math.h.  F = J + 1 frames.
 *   steps      float32 [J, 16]: steps[j] = the network's pose matrix of the frame pair (j, j+1), in the convention of
 *              bbd_pose_ate's gt_local with skip 1: it plays the role of inv(inv(G_j) . G_{j+1})
 *   gt         float64 [M, 12], M >= F: the rows of the KITTI poses file; rows past F are not read
 *   lengths    HOST float64 [n_len], 1 <= n_len <= BBD_TRAJ_MAX_LEN, positive, finite and strictly increasing: the
 *              sub-sequence lengths in the unit of gt (the devkit: 100 .. 800 m); read before the call returns
 *   traj       float64 [F, 16] out: C_0 = I, C_{j+1} = C_j . inv(steps[j]) (general inverse, left to right)
 *   gt_traj    float64 [F, 16] out: inv(G_0) . G_j
 *   aligned    float64 [F, 16] out: [R R_j | c R p_j + t] over (0 0 0 1)
 *   transform  float64 [16] out: [R | t] over (0 0 0 1); the scale c is summary[6]
 *   dist       float64 [F] out: the ground truth's path length up to frame j, non-decreasing
 *   pairs      float64 [ceil(F / step), n_len, 4] out: for first = 0, step, 2 step .. and every length (last, t_err, r_err,
 *              0), errors per unit of length and in radians per unit of length; no frame far enough: (-1, NaN, NaN, 0)
 *   per_length float64 [n_len, 3] out: mean t_err, mean r_err, count of the length's valid pairs
 *   summary    float64 [8] out: t_rel, r_rel (means over all valid pairs), their count, ate_rmse, ate_mean, ate_max, c, F
 *   mode       BBD_TRAJ_SIM3 (Umeyama), _SE3 (the same with c = 1), _SCALE (R = I, t = 0, c = sum g.p / sum p.p) or _NONE
 * A mean without a pair is NaN; a prediction that never moves makes c = 0/0 = NaN under SIM3 and SCALE, and every
 * number that depends on c with it.  Every NaN is 0x7ff8000000000000.  A NULL pointer, J < 1, M < J + 1, n_len outside
 * [1, 8], step < 1, bad lengths or an unknown mode return BBD_E_BADARG, M > INT_MAX / 16 BBD_E_TOOMANY; nothing is
 * launched then and no output is touched. */
#define BBD_TRAJ_MAX_LEN 8
#define BBD_TRAJ_SIM3 0
#define BBD_TRAJ_SE3 1
#define BBD_TRAJ_SCALE 2
#define BBD_TRAJ_NONE 3
int bbd_pose_trajectory(const float* steps, const double* gt, const double* lengths, double* traj, double* gt_traj,
                        double* aligned, double* transform, double* dist, double* pairs, double* per_length,
                        double* summary, int J, int M, int n_len, int step, int mode, void* stream);

/* ---- Loader image pipeline: replaces the per-item Pillow/torchvision work of
 * datasets/mono_dataset.py:186-205 (Resize(LANCZOS) chain, ColorJitter, ToTensor) and the stacking of
 * Trainer.custom_collate (trainer.py:867-886).  Images are uint8 HWC (as PIL decodes them) inside one
 * device buffer; every job addresses its source and destination by offset, so results land directly
 * in the rows of the collated batch tensors.  Bit-exact against Pillow (bbd_image_math.h).
 *
 * Resample job (int32[BBD_RESAMPLE_JOB]): src byte offset lo,hi | dst byte offset lo,hi | in_h, in_w,
 * out_size, ksize | coef_off, bounds_off (int32 elements into coef / bounds), flags, pad.
 *   bbd_resample_h_u8: [in_h,in_w,C] -> [in_h,out_size,C]   (flags & BBD_RESAMPLE_FLIP mirrors the source
 *                      columns = PIL transpose(FLIP_LEFT_RIGHT) before the resize, kitti_dataset.py:58-59)
 *   bbd_resample_v_u8: [in_h,in_w,C] -> [out_size,in_w,C]
 * coef[out][ksize] are Pillow's 22-bit fixed-point filter taps, bounds[out] = (first source index, count);
 * the host builds them (baseboostdepth_amd/imageops.py:resample_table, Resample.c precompute_coeffs). */
#define BBD_RESAMPLE_JOB 12
#define BBD_RESAMPLE_FLIP 1
int bbd_resample_h_u8(const uint8_t* src, uint8_t* dst, const int32_t* jobs, int n_jobs, int max_in_h,
                      const int32_t* coef, const int32_t* bounds, int channels, void* stream);
int bbd_resample_v_u8(const uint8_t* src, uint8_t* dst, const int32_t* jobs, int n_jobs, int max_out_h,
                      int max_row_bytes, const int32_t* coef, const int32_t* bounds, int channels, void* stream);

/* torchvision ColorJitter (functional_pil, order and factors drawn by the host per image) followed by
 * ToTensor, for n_jobs uint8 [H,W,3] images -> fp32 [3,H,W] at dst + offset (floats).
 * Jitter job (int32[BBD_JITTER_JOB]): src byte offset lo,hi | dst float offset lo,hi | op[4] in
 * application order (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none) | param[4]: float bits of
 * the factor, or for hue the uint8 offset int(hue_factor*255) & 255.  lsum_scratch: uint32[n_jobs]. */
#define BBD_JITTER_JOB 12
int bbd_color_jitter_u8(const uint8_t* src, float* dst, const int32_t* jobs, int n_jobs, int H, int W,
                        uint32_t* lsum_scratch, void* stream);

/* ToTensor only. Convert job (int32[BBD_CONVERT_JOB]): src byte offset lo,hi | dst float offset lo,hi. */
#define BBD_CONVERT_JOB 4
int bbd_u8_to_float_chw(const uint8_t* src, float* dst, const int32_t* jobs, int n_jobs, int H, int W,
                        void* stream);

/* ---- Encoder glue: training-mode BatchNorm2d (+ residual) (+ ReLU) of the torchvision-layout ResNet
 * blocks (networks/resnet_encoder.py:12-91; `bn(conv(x))`, `relu(bn(conv(x)))`, `relu(bn(conv(x)) + identity)`),
 * same definition as F.batch_norm(training=True): biased variance to normalise, unbiased for running_var.
 * x, y, residual, grads are [N,C,HW] fp32 (NCHW contiguous); scratch holds bbd_bn_scratch_doubles(N,C,HW)
 * doubles; running_mean/var may both be NULL (no tracking); relu != 0 applies max(0, .).
 *   fwd: writes y, save_mean[C], save_invstd[C]; updates running stats with `momentum` and increments
 *        *num_batches_tracked (int64 device scalar, may be NULL)
 *   bwd: the ReLU mask (relu != 0) is y > 0; a forward WITHOUT a residual may pass y = NULL and `beta`: the mask is
 *        then re-derived from x with the forward's own expression (identical bits), which saves one read of the
 *        activation in each of the two backward launches; grad_residual may be NULL */
int bbd_bn_scratch_doubles(int N, int C, int HW);
/* Grouped form: the N samples are G consecutive call groups, rows [group_rows[g], group_rows[g+1]) (HOST array of
 * G+1 ints, group_rows[0] = 0, group_rows[G] = N, G <= BBD_BN_MAX_GROUPS), each normalised with its OWN batch
 * statistics - bit for bit what G separate calls of the layer on the G sub-batches compute, in one pass.  This is how
 * the pose network's per-frame calls (trainer.py:348-418: up to 26 calls per step on <= 12 samples each) run as one
 * batched pass.  save_mean / save_invstd are [G,C]; the running statistics receive G momentum updates in group order
 * and num_batches_tracked += G; grad_gamma / grad_beta are summed over the groups.  scratch:
 * bbd_bn_grouped_scratch_doubles(largest group, G, C, HW) doubles.
 * untracked_groups (ABI 6; 0 <= . < G): the LAST that many groups are normalised like the others but take no part in the
 * running statistics or num_batches_tracked - padding rows.  Boosted batches change the batched pose pass's row count
 * almost every step (mono_dataset.py:87-109), and every new row count is a new convolution problem for MIOpen (tens of
 * seconds of solver compilation at first sight); the trainer rounds the pass up to a row count with shipped find results (else a multiple of 32) with one
 * trailing group of zero rows whose outputs nobody reads (their gradients are exact zeros). */
#define BBD_BN_MAX_GROUPS 32
int bbd_bn_grouped_scratch_doubles(int max_group_rows, int G, int C, int HW);
int bbd_bn_act_grouped_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                           float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                           long long* num_batches_tracked, double* scratch, const int32_t* group_rows, int G,
                           int untracked_groups, int N, int C, int HW, double eps, double momentum, int relu, void* stream);
int bbd_bn_act_grouped_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual,
                           float* grad_gamma, float* grad_beta, double* scratch, const int32_t* group_rows, int G, int N,
                           int C, int HW, int relu, void* stream);
/* The same two launches with the group table RESIDENT ON THE DEVICE (ABI 7): group_table = device int32
 * [BBD_BN_MAX_GROUPS + 2] = { rows[0] = 0, rows[1], ..., rows[G] = N, (unused up to index BBD_BN_MAX_GROUPS),
 * [BBD_BN_MAX_GROUPS + 1] = number of TRACKED groups }.  Groups may be EMPTY (rows[g+1] == rows[g]: nothing is read or
 * written for them); the groups from the tracked count on are the padding of bbd_bn_act_grouped_fwd's `untracked_groups`.
 * max_group_rows (host) bounds every group's row count (it sizes the grid and the scratch:
 * bbd_bn_grouped_scratch_doubles(max_group_rows, G, C, HW)); a group holds its own statistics exactly as in the
 * host-table form - bit for bit the same numbers.  Why: the boosted recipe redraws every sample's frame set per item
 * (mono_dataset.py:87-109), so the pose pass's call groups change every step; with the table on the device NOTHING in the
 * launch arguments depends on the batch signature, and one captured step graph serves every ordering that shares the
 * padded row count (the table is a section of the step's one table upload). */
int bbd_bn_act_grouped_dev_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                               float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                               long long* num_batches_tracked, double* scratch, const int32_t* group_table, int G,
                               int max_group_rows, int N, int C, int HW, double eps, double momentum, int relu,
                               void* stream);
int bbd_bn_act_grouped_dev_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual,
                               float* grad_gamma, float* grad_beta, double* scratch, const int32_t* group_table, int G,
                               int max_group_rows, int N, int C, int HW, int relu, void* stream);
int bbd_bn_act_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                   float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                   long long* num_batches_tracked, double* scratch, int N, int C, int HW, double eps,
                   double momentum, int relu, void* stream);
int bbd_bn_act_bwd(const float* x, const float* y, const float* grad_y, const float* gamma, const float* beta,
                   const float* save_mean, const float* save_invstd, float* grad_x, float* grad_residual,
                   float* grad_gamma, float* grad_beta, double* scratch, int N, int C, int HW, int relu,
                   void* stream);

/* ReflectionPad2d(1) in front of every decoder convolution (layers.py:118-133) and the stem's
 * MaxPool2d(kernel 3, stride 2, padding 1) (networks/resnet_encoder.py:28), forward and gather-form
 * (atomic-free, deterministic) backward; `planes` = N*C, tensors NCHW fp32.
 *   pad : in [planes,H,W] -> out [planes,H+2,W+2]
 *   pool: in [planes,H,W] -> out [planes,OH,OW], OH = (H-1)/2+1; `code` u8 [planes,OH,OW] = position
 *         0..8 of the maximum inside its window (ATen's tie / NaN rule), consumed by the backward */
int bbd_reflect_pad1_fwd(const float* in, float* out, int planes, int H, int W, void* stream);
int bbd_reflect_pad1_bwd(const float* grad_out, float* grad_in, int planes, int H, int W, void* stream);
int bbd_maxpool3s2_fwd(const float* in, float* out, uint8_t* code, int planes, int H, int W, void* stream);
int bbd_maxpool3s2_bwd(const float* grad_out, const uint8_t* code, float* grad_in, int planes, int H, int W,
                       void* stream);

/* Encoder stem (ABI 21): conv1 -> BatchNorm2d + ReLU -> MaxPool2d(3, 2, 1) (networks/resnet_encoder.py:80-84) with the
 * pool inside the BatchNorm launches - what bbd_bn_act_grouped_fwd(relu = 1, no residual) followed by bbd_maxpool3s2_fwd
 * computes, and the backward of that pair, bit for bit.
 *   fwd: bn_stats, then ONE pass that reads x [N,C,H,W] and writes pooled / code [N,C,OH,OW] (OH = (H-1)/2+1, OW = W/2)
 *        and, when y is not NULL, y [N,C,H,W]; statistics, running statistics and call groups as in
 *        bbd_bn_act_grouped_fwd (save_mean / save_invstd [G,C]).
 *   bwd: the two BatchNorm launches with g = [grad_y, if given] + the pooled gradients whose code points at the pixel;
 *        neither the pool's full-size gradient nor its sum with grad_y is written.  grad_y or grad_pooled may be NULL,
 *        not both; the ReLU mask is re-derived from x (`beta`).
 * Only activations that take the two-launch form are accepted: largest group * H * W > BBD_STEM_MIN_ELEMS and
 * W % 4 == 0 (any H >= 1); everything else is BBD_E_BADARG and stays with the separate entry points.  x, y and the
 * full-size gradients are 16-byte aligned, pooled / grad_pooled 8, code 2.  scratch: bbd_bn_grouped_scratch_doubles(largest
 * group, G, C, H * W).  The _dev_ forms read the device-resident table of bbd_bn_act_grouped_dev_*. */
#define BBD_STEM_MIN_ELEMS 8192
int bbd_stem_fwd(const float* x, const float* gamma, const float* beta, float* y, float* pooled, uint8_t* code,
                 float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                 long long* num_batches_tracked, double* scratch, const int32_t* group_rows, int G, int untracked_groups,
                 int N, int C, int H, int W, double eps, double momentum, void* stream);
int bbd_stem_bwd(const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code, const float* gamma,
                 const float* beta, const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma,
                 float* grad_beta, double* scratch, const int32_t* group_rows, int G, int N, int C, int H, int W,
                 void* stream);
int bbd_stem_dev_fwd(const float* x, const float* gamma, const float* beta, float* y, float* pooled, uint8_t* code,
                     float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                     long long* num_batches_tracked, double* scratch, const int32_t* group_table, int G,
                     int max_group_rows, int N, int C, int H, int W, double eps, double momentum, void* stream);
int bbd_stem_dev_bwd(const float* x, const float* grad_y, const float* grad_pooled, const uint8_t* code, const float* gamma,
                     const float* beta, const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma,
                     float* grad_beta, double* scratch, const int32_t* group_table, int G, int max_group_rows, int N, int C,
                     int H, int W, void* stream);

/* Disparity head of the depth decoder: layers.Conv3x3(C, 1) = ReflectionPad2d(1) + Conv2d(C, 1, 3) + bias
 * (layers.py:118-133, networks/depth_decoder.py:38-39), forward and backward without a padded copy.
 * x [N,C,H,W], weight [C,3,3] (= conv.weight[0]), bias [1] or NULL, y / grad_y [N,1,H,W];
 * grad_x or grad_weight(+grad_bias) may be NULL; scratch holds bbd_dispconv_scratch_doubles(C) doubles. */
int bbd_dispconv_scratch_doubles(int C);
int bbd_dispconv_fwd(const float* x, const float* weight, const float* bias, float* y, int N, int C, int H, int W,
                     void* stream);
int bbd_dispconv_bwd(const float* x, const float* weight, const float* grad_y, float* grad_x, float* grad_weight,
                     float* grad_bias, double* scratch, int N, int C, int H, int W, void* stream);

/* The same layer with the decoder's sigmoid inside (networks/depth_decoder.py:58): disp = sigmoid(dispconv(x)) in one
 * launch, nothing but disp [N,1,H,W] written.  The backward takes grad_disp [N,1,H,W] and forms
 * grad_disp * (1 - disp) * disp (ATen's sigmoid_backward) on the fly inside both gradient kernels; arguments otherwise
 * as bbd_dispconv_bwd, scratch of the same size. */
int bbd_disp_head_fwd(const float* x, const float* weight, const float* bias, float* disp, int N, int C, int H, int W,
                      void* stream);
int bbd_disp_head_bwd(const float* x, const float* weight, const float* disp, const float* grad_disp, float* grad_x,
                      float* grad_weight, float* grad_bias, double* scratch, int N, int C, int H, int W, void* stream);

/* Input of the batched pose pass in the pooled form of the step: out [R, 2, chw] row r = the image pair
 * (pool[idx_a[r]], pool[idx_b[r]]) of the frame pool [F, chw] (chw = 3*H*W floats, multiple of 4), every texel (v - sub) * mul.
 * Replaces the reference's per-call `torch.cat([frame_a, frame_b], 1)` (trainer.py:352-358, 394-400) over masked sub-batches
 * plus the pose encoder's input normalisation `(x - 0.45) / 0.225` (networks/resnet_encoder.py:83; PyTorch-ROCm divides by a
 * Python scalar as a multiplication by its float reciprocal: pass mul = (float)1 / (float)0.225): same bits, one pass.
 * idx_a / idx_b: device int32 [R] (sections of the step's static table buffer).  sub = 0, mul = 1: a plain gather. */
int bbd_gather_pairs(const float* pool, const int32_t* idx_a, const int32_t* idx_b, float* out, int R, long chw, double sub,
                     double mul, void* stream);

/* Measurement aid (bench.py, SURVEY 8d "on-box measured stream-copy ceiling"): dst[i] = src[i] as a float4 grid-stride
 * copy of n_floats floats (multiple of 4, both pointers 16-byte aligned) with `unroll` (1, 2, 4, 8) independent 16-byte
 * loads per thread in flight; 2 * 4 * n_floats bytes of HBM traffic. */
int bbd_stream_copy(const float* src, float* dst, long n_floats, int unroll, void* stream);

/* Device self-test: the kernels replace hipcc's IEEE division sequence by a cheaper one that is
 * exact for moderate exponents (bbd_math.h).  Runs blocks*256*iters random operand tuples through
 * both and adds the number of bit mismatches to *mismatches (device int32, caller zeroes it). */
int bbd_selftest_div(int blocks, int iters, unsigned seed, int32_t* mismatches, void* stream);

/* Decoder glue (reference networks/depth_decoder.py:44-50, layers.py:103-133), fp32 NCHW:
 *   bbd_upcat_pad1_fwd : out [N, C1+C2, 2h+2, 2w+2] = ReflectionPad2d(1)(cat(nearest_x2(x [N,C1,h,w]), skip [N,C2,2h,2w]))
 *                        in one pass (skip may be NULL with C2 = 0); _bwd: grad_out -> grad_x, grad_skip (gather form,
 *                        no atomics, deterministic).  N*(C1+C2) <= 65535.
 *   bbd_bias_elu_fwd   : y <- ELU(y + bias[c]) in place on a convolution's output [N,C,HW] (HW % 4 == 0)
 *   bbd_bias_elu_bwd   : grad_x = grad_y * ELU'(from the saved output y), grad_bias[c] = sum grad_x (fp64 partial sums,
 *                        fixed order); scratch = bbd_bias_elu_scratch_doubles(N,C,HW) doubles.                       */
int bbd_upcat_pad1_fwd(const float* x, const float* skip, float* out, int N, int C1, int C2, int h, int w, void* stream);
int bbd_upcat_pad1_bwd(const float* grad_out, float* grad_x, float* grad_skip, int N, int C1, int C2, int h, int w,
                       void* stream);
int bbd_bias_elu_scratch_doubles(int N, int C, int HW);
int bbd_bias_elu_fwd(float* y, const float* bias, int N, int C, int HW, void* stream);
int bbd_bias_elu_bwd(const float* y, const float* grad_y, float* grad_x, float* grad_bias, double* scratch, int N, int C,
                     int HW, void* stream);

/* The same glue with the ConvBlock's bias + ELU inside (DepthDecoder levels 4..1), fp32 NCHW.  Values are
 * those of the entry points above applied one after the other, bit for bit; the bias gradients add the same numbers in
 * another (fixed) order.
 *   bbd_upcat_pad_act_fwd : out [N, C1+C2, 2h+2, 2w+2] = ReflectionPad2d(1)(cat(nearest_x2(ELU(z + bias)), skip)) from the
 *                           bias-free convolution output z [N,C1,h,w], which is left as it is (skip may be NULL, C2 = 0)
 *   bbd_upcat_pad_act_bwd : grad_z = g * ELU'(y) with y recomputed from z + bias and g the gradient bbd_upcat_pad1_bwd
 *                           hands to x; grad_skip as there; grad_bias [C1] = sum grad_z
 *   bbd_bias_elu_pad_fwd  : y [N,C,H,W] <- ELU(y + bias[c]) in place and yp [N,C,H+2,W+2] = ReflectionPad2d(1)(y)
 *   bbd_bias_elu_pad_bwd  : grad_z = (the gradient bbd_reflect_pad1_bwd makes of grad_yp + grad_y) * ELU'(y) from the
 *                           saved output y; grad_yp or grad_y may be NULL, not both; grad_bias [C] = sum grad_z
 * Both backwards are one pass plus a one-wave-per-channel sum of per-workgroup float64 partials (no atomics): scratch
 * holds at least channels * N * ceil(rows / BBD_GLUE_ROWS) doubles, rows = h resp. H, channels = C1 resp. C, and
 * scratch_doubles says how many it has.  No allocation, no host synchronisation, every element of every output is
 * written.  N * (C1 + C2) resp. N * C above 65535, H or W below 2, h or w below 1, a padded plane of 2^31 elements or more, a missing pointer or
 * a scratch that is too small return BBD_E_BADARG and launch nothing.  Rows of whole float4s in 16-byte aligned tensors move 16 bytes per
 * lane, everything else one float. */
#define BBD_GLUE_ROWS 4
int bbd_upcat_pad_act_fwd(const float* z, const float* bias, const float* skip, float* out, int N, int C1, int C2, int h, int w,
                          void* stream);
int bbd_upcat_pad_act_bwd(const float* grad_out, const float* z, const float* bias, float* grad_z, float* grad_skip,
                          float* grad_bias, double* scratch, int scratch_doubles, int N, int C1, int C2, int h, int w,
                          void* stream);
int bbd_bias_elu_pad_fwd(float* y, const float* bias, float* yp, int N, int C, int H, int W, void* stream);
int bbd_bias_elu_pad_bwd(const float* grad_yp, const float* grad_y, const float* y, float* grad_z, float* grad_bias,
                         double* scratch, int scratch_doubles, int N, int C, int H, int W, void* stream);

/* Weight gradient of a ConvBlock's 3x3, stride-1 convolution of an input that already carries its border (DepthDecoder
 * `upconv` layers), straight from the NCHW tensors: no transposed copies, no atomics, nothing zeroed first.
 *   xp [N, C, H+2, W+2], grad_z [N, K, H, W], grad_w [K, C, 3, 3] (written, not accumulated), all contiguous fp32:
 *   grad_w[k][c][r][s] = sum over (n, y, x) of grad_z[n][k][y][x] * xp[n][c][y + r][x + s].
 * Numerics: v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain.  Every fp32 accumulator takes at most BBD_WGRAD_RUN
 * products and is then widened; the widened values are added as doubles in a fixed order (per workgroup, then over the
 * workgroups by a second launch), so |grad_w - exact| <= (BBD_WGRAD_RUN + 1) * 2^-24 * sum |grad_z| |xp| element by
 * element, and two calls on the same inputs give the same bits.
 * The call's two host-side queries are declared in include/bbd_wgrad.h.  bbd_conv3x3_wgrad_supported: 1 where the call
 * takes the shape - C and K multiples of 16 in 16..1024, N, H, W >= 1, every tensor and the scratch below 2^31
 * elements - else 0, and the call returns BBD_E_BADARG and launches nothing.  scratch holds
 * bbd_conv3x3_wgrad_scratch_doubles(N, C, K, H, W) doubles (0: not supported); no element of it is read before the call
 * has written it. */
#define BBD_WGRAD_RUN 128
int bbd_conv3x3_wgrad(const float* xp, const float* grad_z, float* grad_w, double* scratch, int N, int C, int K, int H,
                      int W, void* stream);

/* Nearest x2 up-sampling, ReflectionPad2d(1) and a 3x3 convolution of ELU(z + bias) without the up-sampled copy
 * (DepthDecoder upconv(0,1), the level without a skip connection).  All tensors contiguous fp32 NCHW:
 *   bbd_up2conv3x3_fwd : out [N, K, 2h, 2w] = conv3x3(ReflectionPad2d(1)(nearest_x2(ELU(z + bias))), w), no bias added;
 *                        z [N, C, h, w_] is the bias-free output of the convolution before and is left as it is, bias [C],
 *                        w [K, C, 3, 3].  Output pixel (2i + a, 2j + b) reads kernel row r at source row
 *                        i + floor((a + r - 1) / 2), clamped to the map (the reflection border of the up-sampled map is a
 *                        clamp on the source); taps on one source pixel add their weights, so each parity is a 2x2
 *                        convolution: 4/9 of the products.
 *   bbd_up2conv3x3_bwd : grad_z [N, C, h, w_] = the adjoint of that applied to grad_out [N, K, 2h, 2w], times ELU'
 *                        recomputed from z + bias; grad_bias [C] = sum grad_z from float64 per-workgroup partials that a
 *                        second launch adds in a fixed order (scratch holds bbd_up2conv3x3_scratch_doubles(N, C, K, h, w_)
 *                        doubles and scratch_doubles says how many it has; none is read before the call wrote it).
 * Numerics: v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain; no atomics, so two calls give equal bits, and every
 * element of every output is written.  Forward: the longest chain is 4 taps x 16 channels = 64 fused multiply-adds (64
 * roundings); each summed weight is added in double and rounded once (1); the input is ELU(z + bias): one rounding of
 * the sum and expm1f's 2 ulp (3).  With 4 more for second-order terms that is BBD_UP2CONV_ROUNDINGS = 72:
 *   |out - exact| <= BBD_UP2CONV_ROUNDINGS * 2^-24 * sum |w| |ELU(z + bias)|  element by element
 * (nine separate taps would take 144 + 8).  Backward: kernel rows are summed as weights, kernel columns as data (two or
 * three gradients added in fp32 before the product), at most 60 fused multiply-adds per element against the 576 products
 * of the composition.
 * The two host-side queries are declared in include/bbd_up2conv.h.  A shape bbd_up2conv3x3_supported refuses - anything
 * but C = K = 16, N, h or w_ below 1, an output of 2^31 elements or more - a NULL pointer or a scratch that is too small
 * return BBD_E_BADARG and launch nothing. */
#define BBD_UP2CONV_ROUNDINGS 72
int bbd_up2conv3x3_fwd(const float* z, const float* bias, const float* w, float* out, int N, int C, int K, int h, int w_,
                       void* stream);
int bbd_up2conv3x3_bwd(const float* grad_out, const float* z, const float* bias, const float* w, float* grad_z,
                       float* grad_bias, double* scratch, int scratch_doubles, int N, int C, int K, int h, int w_,
                       void* stream);

/* The encoder stems' conv1 - 7x7, stride 2, pad 3, C = 3 or 6 input channels, K = 64 output channels, no bias - and its
 * weight gradient, straight from the NCHW tensors.  All tensors contiguous fp32; Ho = (H + 1) / 2,
 * Wo = (W + 1) / 2:
 *   bbd_stem_conv7s2_fwd   : out [N, 64, Ho, Wo] = conv2d(x' [N, C, H, W], w [64, C, 7, 7], stride 2, pad 3), where
 *                            x' = x, or with normalize != 0 the encoder's (x - 0.45) / 0.225 evaluated as bbd_gather_pairs
 *                            evaluates it (subtract, multiply by the float reciprocal); the zero border pads x'.
 *   bbd_stem_conv7s2_wgrad : grad_w [64, C, 7, 7] (written, not accumulated) = sum over (n, oy, ox) of
 *                            grad_out[n][k][oy][ox] * x'[n][c][2 oy + r - 3][2 ox + s - 3], x' re-formed from x by the
 *                            same flag.  scratch holds bbd_stem_conv7s2_wgrad_scratch_doubles(...) doubles and
 *                            scratch_doubles says how many it has; none is read before the call wrote it.
 * Numerics: v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain; no atomics and nothing zeroed first, so two calls give
 * equal bits and every element of every output is written.  Forward: one chain per input channel over its 49 taps
 * (padding taps carry weight zero and add exactly nothing), the C chains added in fp32 - fewer roundings than one chain
 * over all C * 49 taps, so |out - exact| <= (P + 1) * 2^-24 * sum |w| |x'| with P = 148 (C = 3) or 296 (C = 6).  Weight gradient: every fp32 accumulator takes at most BBD_WGRAD_RUN products and is
 * then added to a double; doubles are added in a fixed order (per lane, then over the workgroups by a second launch):
 * |grad_w - exact| <= (BBD_WGRAD_RUN + 1) * 2^-24 * sum |grad_out| |x'|.
 * x must be finite: the zero taps that pad the reduction and, in the weight gradient, the pixels past the last row or
 * column of out multiply an exact zero by a staged value of x, so an Inf or NaN in x can reach elements that conv2d would
 * leave finite.
 * The two host-side queries are declared in include/bbd_stemconv.h.  A shape bbd_stem_conv7s2_supported refuses -
 * K != 64, C not 3 or 6, N, H or W below 1, a tensor of 2^31 elements or more - a NULL pointer or a scratch that is too
 * small return BBD_E_BADARG and launch nothing. */
int bbd_stem_conv7s2_fwd(const float* x, const float* w, float* out, int N, int C, int K, int H, int W, int normalize,
                         void* stream);
int bbd_stem_conv7s2_wgrad(const float* x, const float* grad_out, float* grad_w, double* scratch, int scratch_doubles,
                           int N, int C, int K, int H, int W, int normalize, void* stream);

/* The ResNet shortcut convolution - 1x1, stride 2, no padding, no bias, groups 1 (layer{2,3,4}.0.downsample.0 of both
 * encoders) - in its three directions, straight from the NCHW tensors.  All tensors contiguous fp32;
 * Ho = (H + 1) / 2, Wo = (W + 1) / 2; any N, H, W >= 1, C and K multiples of 16:
 *   bbd_conv1x1s2_fwd      : y [N, K, Ho, Wo] = conv2d(x [N, C, H, W], w [K, C, 1, 1], stride 2); one launch; reads the
 *                            even rows of x only.
 *   bbd_conv1x1s2_bwd_data : grad_x [N, C, H, W] from grad_y and w; one launch.  accumulate == 0: every element of grad_x
 *                            is written exactly once, the zeros of odd rows and odd columns included.  accumulate != 0:
 *                            grad_x holds a tensor already; the gradient is added to its even positions (2 oy, 2 ox) and
 *                            no other element is read or written.
 *   bbd_conv1x1s2_wgrad    : grad_w [K, C, 1, 1] (written, not accumulated) = sum over (n, oy, ox) of
 *                            grad_y[n][k][oy][ox] * x[n][c][2 oy][2 ox]; two launches.  scratch holds
 *                            bbd_conv1x1s2_wgrad_scratch_doubles(...) doubles (K * C times a count that depends on K and C
 *                            only, not on N) and scratch_doubles says how many it has; none is read before the call wrote
 *                            it.
 * Numerics: v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain; no atomics and nothing zeroed first, so two calls give
 * equal bits.  Forward: one chain over the C input channels, |y - exact| <= (C + 1) * 2^-24 * sum |w| |x|.  Data
 * gradient: one chain over the K output channels, |grad_x - exact| <= (K + 1) * 2^-24 * sum |w| |grad_y|; accumulate mode
 * adds that value to the element in fp32, one more rounding: (K + 2) * 2^-24 * (sum |w| |grad_y| + |grad_x before|).
 * Weight gradient: every fp32 accumulator takes at most BBD_WGRAD_RUN products and is then added to a double; doubles are
 * added in a fixed order (per lane, then over the records by the second launch):
 * |grad_w - exact| <= (BBD_WGRAD_RUN + 1) * 2^-24 * sum |grad_y| |x|.
 * The two host-side queries are declared in include/bbd_conv1x1.h.  A shape bbd_conv1x1s2_supported refuses - C or K not
 * a multiple of 16, N, H or W below 1, a tensor of 2^31 elements or more - a NULL pointer or a scratch that is too small
 * return BBD_E_BADARG and launch nothing. */
int bbd_conv1x1s2_fwd(const float* x, const float* w, float* y, int N, int C, int K, int H, int W, void* stream);
int bbd_conv1x1s2_bwd_data(const float* grad_y, const float* w, float* grad_x, int N, int C, int K, int H, int W,
                           int accumulate, void* stream);
int bbd_conv1x1s2_wgrad(const float* x, const float* grad_y, float* grad_w, double* scratch, int scratch_doubles, int N,
                        int C, int K, int H, int W, void* stream);

/* ---- MonoViT encoder (BASELINE configs[4]): depth-wise convolution on token-layout activations ----------
 * The position encodings of the reference's MPViT (networksvit/mpvit.py:240-330: ConvPosEnc, ConvRelPosEnc)
 * are depth-wise k x k convolutions (k in {3,5,7}, stride 1, zero padding k/2) over the token matrix viewed
 * as an image.  Tokens are [B, H*W, C] row-major (= NHWC); x / y / grad_y may be channel slices of wider
 * rows: `*_row` is the number of floats between consecutive tokens and the pointer addresses the slice's
 * first channel, C is the number of channels of the slice.  weight [C,k,k] (nn.Conv2d's [C,1,k,k]), bias [C]
 * or NULL.
 *   fwd   : y = bias + conv(x) (+ x when add_input & 1; added to y's previous contents when add_input & 2).
 *           flip = 1 mirrors the taps: with x := grad_y, bias NULL this is the data gradient (bit 0 carries the
 *           residual's gradient, bit 1 lets it land in a slice that already holds another contribution).
 *   wgrad : grad_weight [C,k,k], grad_bias [C] (or NULL); partial = scratch of
 *           bbd_dwconv_tokens_wgrad_scratch_floats(B,H,W,C,k) floats.  Deterministic (one partial row per
 *           workgroup, a fixed-order column sum in fp64).  accumulate != 0: added to grad_weight / grad_bias
 *           (a parameter shared by several layers - MPViT's MHCAEncoder shares its position encodings - whose
 *           launches follow each other on one stream).                                                   */
long bbd_dwconv_tokens_wgrad_scratch_floats(int B, int H, int W, int C, int k);
int bbd_dwconv_tokens_fwd(const float* x, int x_row, const float* weight, const float* bias, float* y, int y_row,
                          int B, int H, int W, int C, int k, int add_input, int flip, void* stream);
int bbd_dwconv_tokens_wgrad(const float* x, int x_row, const float* grad_y, int gy_row, float* partial,
                            float* grad_weight, float* grad_bias, int B, int H, int W, int C, int k, int accumulate,
                            void* stream);
/* The same for n_groups <= 4 consecutive-or-not channel groups with their own window sizes in ONE launch each (the head
 * groups of MPViT's ConvRelPosEnc, networksvit/mpvit.py:262-330): group g covers channels [c0[g], c0[g] + cn[g]) of the
 * x / y / grad_y rows with window k[g]; weights / biases / grad_weights / grad_biases are HOST arrays of device pointers
 * (a NULL biases array or entry: no bias).  c0 / cn / k are host arrays.                                              */
int bbd_dwconv_tokens_groups_fwd(const float* x, int x_row, float* y, int y_row, int n_groups, const int32_t* c0,
                                 const int32_t* cn, const int32_t* k, const void* const* weights, const void* const* biases,
                                 int B, int H, int W, int add_input, int flip, void* stream);
long bbd_dwconv_tokens_groups_wgrad_scratch_floats(int B, int H, int W, int n_groups, const int32_t* cn, const int32_t* k);
int bbd_dwconv_tokens_groups_wgrad(const float* x, int x_row, const float* grad_y, int gy_row, float* partial, int n_groups,
                                   const int32_t* c0, const int32_t* cn, const int32_t* k, const void* const* grad_weights,
                                   const void* const* grad_biases, int B, int H, int W, int accumulate, void* stream);

/* Residual + stochastic depth + LayerNorm on token-layout activations [rows = B*N, C] (csrc/bbd_tokens.hip), the glue of
 * the reference's MHCABlock (networksvit/mpvit.py:397-440: x = x + drop_path(branch); z = norm(x)) as one pass each way.
 *   fwd: y = x + branch * mask[row / N];  z = LayerNorm(y) * weight + bias;  stats[row] = (mean, rstd).
 *        branch == NULL: plain LayerNorm of x (y is not written);  mask == NULL: no stochastic depth;
 *        weight == NULL: residual only (z, stats, bias unused).
 *   bwd: g = grad_y + dLayerNorm(grad_z);  grad_x = g;  grad_branch = g * mask[row / N] (NULL: not wanted);
 *        grad_weight / grad_bias through `partial` (bbd_token_ln_scratch_floats(rows, C) floats): one partial row per
 *        workgroup, summed in a fixed order by a second launch (deterministic).  grad_y may be NULL.
 *   C % 4 == 0 and C <= 1024 (bbd_token_ln_supported).                                                             */
int bbd_token_ln_supported(int C);
long bbd_token_ln_scratch_floats(int rows, int C);
int bbd_token_ln_fwd(const float* x, const float* branch, const float* mask, const float* weight, const float* bias,
                     float* y, float* z, float* stats, int rows, int N, int C, double eps, void* stream);
int bbd_token_ln_bwd(const float* grad_z, const float* grad_y, const float* y, const float* stats, const float* weight,
                     const float* mask, float* grad_x, float* grad_branch, float* partial, float* grad_weight,
                     float* grad_bias, int rows, int N, int C, void* stream);

/* out[c] = sum over rows of x[row, c] for a [rows, C] matrix, C % 4 == 0: the bias gradient of the token-parallel
 * nn.Linear layers (qkv, proj, fc1, fc2 of networksvit/mpvit.py:51-78, 333-394) on [B*N, C] token activations, in two
 * launches (one partial row per workgroup, fixed-order sum of the partial rows: deterministic).
 * partial: bbd_colsum_scratch_floats(rows, C) floats.                                                                */
long bbd_colsum_scratch_floats(long rows, int C);
int bbd_colsum(const float* x, float* partial, float* out, long rows, int C, void* stream);

/* Factorised attention of MPViT (networksvit/mpvit.py:333-394) on the packed qkv activation.
 *   qkv [B, N, 3, h, Ch] = the qkv Linear's output (C = h*Ch); convv [B,N,C] = ConvRelPosEnc's conv(v)
 *   fwd : out[b,n,h,vc] = sum_kc q[b,n,h,kc] ctxs[b,h,kc,vc] + q[b,n,h,vc] convv[b,n,h,vc],
 *         ctxs = scale * softmax_N(k)^T v per head; also returns kmax / krsum [B,C] (softmax statistics of
 *         k over the tokens) and ctxs [B, h, Ch, Ch] for the backward.
 *   bwd : grad_out [B,N,C] -> grad_qkv [B,N,3C] (dq | dk | dv), grad_convv [B,N,C]; dctx = work buffer
 *         [B, h, Ch, Ch].  scratch: bbd_factor_att_scratch_floats(B,N,C,Ch) floats for both calls.
 *   Deterministic (per-token-segment partial sums combined in fixed order).  Supported shapes:
 *   bbd_factor_att_supported(C, Ch) != 0: Ch divides C, C <= 1024, C*Ch <= 12288, and the dynamic LDS of each of the
 *   four launches (context in the form the shape takes, output, backward) fits a workgroup (160 KiB; the launches
 *   opt in above 64 KiB, the row-per-thread context form - 128 < C <= 512, Ch <= 48 - stays within 64 KiB).  True for
 *   every stage of MPViT tiny / xsmall / small and up to (512,16), (576,18); false e.g. for (768,16), (1024,12),
 *   (256,1), (512,2), (510,5), (504,6).  Both calls return BBD_E_BADARG for a shape the predicate refuses.        */
int bbd_factor_att_supported(int C, int Ch);
int bbd_factor_att_segments(int B, int N);
long bbd_factor_att_scratch_floats(int B, int N, int C, int Ch);
int bbd_factor_att_fwd(const float* qkv, const float* convv, float* kmax, float* krsum, float* ctxs, float* scratch,
                       float* out, int B, int N, int C, int Ch, double scale, void* stream);
int bbd_factor_att_bwd(const float* qkv, const float* convv, const float* kmax, const float* krsum, const float* ctxs,
                       const float* grad_out, float* dctx, float* scratch, float* grad_qkv, float* grad_convv, int B,
                       int N, int C, int Ch, double scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BBD_HIP_H */
