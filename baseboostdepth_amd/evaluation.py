"""Validation metrics on the device.

`GroundTruthSet` keeps a whole split's ground-truth depth maps (ragged sizes) resident in HBM as
one buffer plus an int descriptor table, so scoring an image is one kernel launch with no host
round trip - the reference re-uploads the map, builds the crop mask in numpy, gathers with it and
sorts twice per image (trainer.py:594-617, evaluate_depth.py:244-297).

`depth_metrics` is the single entry for the KITTI metrics: one `bbd_depth_metrics` launch for a batch of predictions.

The SYNS-Patches metrics (evaluate_depth.py:26-102 with `--eval_split SYNS [--chamfer]`) are layered on it, each
layer callable on its own: `pred_edges` (log, blur, Sobel, threshold), `distance_transform` (exact squared Euclidean
distance maps), `edge_metrics` (edge accuracy / completeness and `err`), `pointcloud_metrics` (F-score and IoU of the
back-projected clouds, all-pairs nearest neighbour) and `syns_metrics`, the reference's 9-column row.

The KITTI odometry evaluation (evaluate_pose.py) is `pose_ate` - chained poses, local ground truth, the trajectory error
of every track and its mean / std in one `bbd_pose_ate` call - `pose_trajectory` - the whole trajectory chained from the
single steps, aligned to ground truth, with the devkit's t_rel / r_rel and the aligned ATE in one `bbd_pose_trajectory`
call - and `evaluate_pose`, the evaluator above them.
"""
import collections

import numpy as np
import torch

from . import ops
from .tables import split64, upload
from ._lib import (ALIGN_OUT, EVAL_DESC, EVAL_OUT, EVAL_PRED_IS_DISP, EVAL_MEDIAN_MIDPOINT, EVAL_NO_MEDIAN_SCALING,
                   SYNS_OUT, SYNS_CLOUD_OUT, SYNS_RAYS_PIXEL, TRAJ_MAX_LEN, TRAJ_MODES, BbdError, ptr)

METRIC_NAMES = ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]   # trainer.py:156
GARG_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)     # trainer.py:603-604


def garg_window(gh, gw):
    """[r0,r1) x [c0,c1) exactly as the reference computes it (float64 products truncated to int32)."""
    c = np.array([GARG_CROP[0] * gh, GARG_CROP[1] * gh, GARG_CROP[2] * gw, GARG_CROP[3] * gw]).astype(np.int32)
    return int(c[0]), int(c[1]), int(c[2]), int(c[3])


class GroundTruthSet:
    """Ragged ground-truth depth maps of a split, packed once into device memory."""

    def __init__(self, gt_depths, device, crop=True, edges=None):
        """`edges` (SYNS: gt_edges.npz, maps of shape [GH,GW] or [GH,GW,1], non-zero = edge) are packed as bytes at
        the same offsets as the depth maps; without them the set is what it always was."""
        maps = [np.ascontiguousarray(np.asarray(g, dtype=np.float32)) for g in gt_depths]
        assert all(m.ndim == 2 for m in maps)
        self.edges = None
        if edges is not None:
            em = [np.asarray(e) for e in edges]
            em = [(e[..., 0] if e.ndim == 3 else e) != 0 for e in em]
            assert len(em) == len(maps) and all(e.shape == m.shape for e, m in zip(em, maps))
            flat_e = np.concatenate([e.ravel() for e in em]).astype(np.uint8) if em else np.zeros(0, np.uint8)
            self.edges = torch.from_numpy(flat_e).to(device)
        desc = np.zeros((len(maps), EVAL_DESC), dtype=np.int32)
        off = 0
        for i, m in enumerate(maps):
            gh, gw = m.shape
            win = garg_window(gh, gw) if crop else (0, gh, 0, gw)
            desc[i] = split64(off) + (gh, gw) + win
            off += m.size
        flat = np.concatenate([m.ravel() for m in maps]) if maps else np.zeros(0, np.float32)
        self.shapes = [m.shape for m in maps]
        self.buffer = torch.from_numpy(flat).to(device)
        self.desc_host = desc                   # the same rows on the host (ops.gt_viz / ops.error_map rebase them)
        self.desc = torch.from_numpy(desc).to(device)

    @classmethod
    def from_packed(cls, buffer, shapes, crop=True):
        """The set over maps that ALREADY lie back to back in the device buffer `buffer` (float32, map i of shape
        `shapes[i]` after map i - 1), as `kitti_utils.generate_depth_maps` leaves them: only the descriptor table is
        built and uploaded, the maps never visit the host."""
        shapes = [(int(gh), int(gw)) for gh, gw in shapes]
        assert buffer.dtype == torch.float32 and buffer.dim() == 1 and buffer.is_contiguous()
        assert buffer.numel() == sum(gh * gw for gh, gw in shapes)
        desc = np.zeros((len(shapes), EVAL_DESC), dtype=np.int32)
        off = 0
        for i, (gh, gw) in enumerate(shapes):
            win = garg_window(gh, gw) if crop else (0, gh, 0, gw)
            desc[i] = split64(off) + (gh, gw) + win
            off += gh * gw
        self = cls.__new__(cls)
        self.edges = None
        self.shapes = shapes
        self.buffer = buffer
        self.desc_host = desc
        self.desc = torch.from_numpy(desc).to(buffer.device)
        return self

    def __len__(self):
        return len(self.shapes)


def depth_metrics(pred, gts, indices, min_depth=1e-3, max_depth=80.0, clamp=(1e-3, 80.0), pred_is_disp=False,
                  median="torch", median_scaling=True, scale_factor=1.0, backend=None):
    """Scores pred[i] ([n,1,h,w] or [n,h,w]) against gts[indices[i]]; returns a [n, 12] device tensor
    (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, median_gt, median_pred, count, 0)."""
    backend = backend or ops.default_backend()
    pred = pred.detach()
    if pred.dim() == 4:
        assert pred.shape[1] == 1
        pred = pred[:, 0]
    pred = pred.contiguous().float()
    backend._check(pred, gts.buffer)
    n, h, w = pred.shape
    idx = torch.as_tensor(indices, dtype=torch.long, device=gts.desc.device).view(-1)
    assert idx.numel() == n
    desc = gts.desc.index_select(0, idx).contiguous()
    out = torch.empty(n, EVAL_OUT, device=pred.device, dtype=torch.float32)
    flags = (EVAL_PRED_IS_DISP if pred_is_disp else 0) | (EVAL_MEDIAN_MIDPOINT if median == "numpy" else 0) | \
            (0 if median_scaling else EVAL_NO_MEDIAN_SCALING)
    backend.run("bbd_depth_metrics", pred, ptr(pred), ptr(gts.buffer), ptr(desc), ptr(out), n, h, w,
                float(min_depth), float(max_depth), float(clamp[0]), float(clamp[1]), float(scale_factor), flags)
    return out


# the columns of a `depth_metrics_affine` row (BBD_ALIGN_OUT): the count stands where a `depth_metrics` row has it
ALIGN_COLUMNS = ["abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "scale", "shift", "silog", "count", "irmse"]


def depth_metrics_affine(pred_disp, gts, indices, min_depth=1e-3, max_depth=80.0, backend=None):
    """Scores pred_disp[i] ([n,1,h,w] or [n,h,w]), a disparity-like map in ANY affine gauge (a relative-depth model's
    output), against gts[indices[i]]: per image the scale and shift that fit it to 1 / ground truth by least squares on
    the pixels `depth_metrics` scores, then the errors of the aligned depth.  One
    `bbd_depth_metrics_affine` launch; returns a float64 [n, 12] device tensor with the columns `ALIGN_COLUMNS`
    (silog in percent, irmse in 1/km).  An image with fewer than two scored pixels or a constant prediction has NaNs
    and its count."""
    backend = backend or ops.default_backend()
    pred = pred_disp.detach()
    if pred.dim() == 4:
        assert pred.shape[1] == 1
        pred = pred[:, 0]
    pred = pred.contiguous().float()
    backend._check(pred, gts.buffer)
    n, h, w = pred.shape
    idx = torch.as_tensor(indices, dtype=torch.long, device=gts.desc.device).view(-1)
    assert idx.numel() == n
    desc = gts.desc.index_select(0, idx).contiguous()
    out = torch.empty(n, ALIGN_OUT, device=pred.device, dtype=torch.float64)
    backend.run("bbd_depth_metrics_affine", pred, ptr(pred), ptr(gts.buffer), ptr(desc), ptr(out), n, h, w,
                float(min_depth), float(max_depth), 0)
    return out


# ---------------------------------------------------------------------------- SYNS-Patches metrics
SYNS_MIN_DEPTH, SYNS_MAX_DEPTH = 1e-3, 125.0        # evaluate_depth.py:107-109
SYNS_EDGE_TH, SYNS_CLOUD_TH = 10.0, 0.1             # evaluate_depth.py:90, :85
SYNS_COLUMNS = ["abs_rel", "err", "sq_rel", "rmse", "rmse_log", "edge_Acc", "edge_comp", "f1", "iou1"]


class _SynsCall:
    """What every SYNS launch needs: the batch's descriptor rows and the strides that size the launches.  The strides
    come from the largest map of the WHOLE set, which the host knows without asking the device."""

    def __init__(self, pred, gts, indices, backend):
        self.backend = backend or ops.default_backend()
        pred = pred.detach()
        if pred.dim() == 4:
            assert pred.shape[1] == 1
            pred = pred[:, 0]
        self.pred = pred.contiguous().float()
        self.backend._check(self.pred, gts.buffer)
        self.n, self.h, self.w = self.pred.shape
        idx = torch.as_tensor(indices, dtype=torch.long, device=gts.desc.device).view(-1)
        assert idx.numel() == self.n
        self.desc = gts.desc.index_select(0, idx).contiguous()
        self.max_h, self.max_w, self.px_stride = syns_strides(gts)
        self.n_ints = self.backend.lib.syns_scratch_ints(self.n, self.px_stride)
        if self.n_ints < 0:
            raise BbdError("SYNS metrics: %d images of up to %d pixels are more than one scratch buffer holds; "
                           "split the batch" % (self.n, self.px_stride))

    def scratch(self):
        return torch.empty(self.n_ints, dtype=torch.int32, device=self.pred.device)

    def sizes(self):
        return self.n, self.h, self.w, self.px_stride, self.max_h, self.max_w


def syns_strides(gts):
    """(max GH, max GW, elements per image slot) of a set: the slot holds max GH x max GW, rounded up to 4 elements."""
    max_h, max_w = max(s[0] for s in gts.shapes), max(s[1] for s in gts.shapes)
    return max_h, max_w, (max_h * max_w + 3) // 4 * 4


def image_view(buf, gts, index, row):
    """Row `row` of a strided per-image buffer ([n, px_stride]) as the [GH, GW] map of gts[index]."""
    gh, gw = gts.shapes[int(index)]
    return buf[row, :gh * gw].view(gh, gw)


def pred_edges(pred, gts, indices, pred_is_disp=False, clamp=(1e-3, 80.0), backend=None):
    """evaluate_depth.py:260-265 / trainer.py:580-588 on the device: the prediction at ground-truth size (as
    `depth_metrics` resamples it), to_log, GaussianBlur 3x3 sigma 1, 5x5 Sobel in float64, magnitude > its mean.
    Returns (edge uint8 [n, px_stride], stats float64 [n, 2] = mean magnitude, number of edge pixels);
    `image_view(edge, gts, indices[i], i)` is image i's map."""
    c = _SynsCall(pred, gts, indices, backend)
    dev = c.pred.device
    edge = torch.zeros(c.n, c.px_stride, dtype=torch.uint8, device=dev)
    stats = torch.empty(c.n, 2, dtype=torch.float64, device=dev)
    scratch = c.scratch()
    c.backend.run("bbd_syns_pred_edges", c.pred, ptr(c.pred), ptr(c.desc), ptr(scratch), c.n_ints, ptr(edge),
                  ptr(stats), *c.sizes(), float(clamp[0]), float(clamp[1]), EVAL_PRED_IS_DISP if pred_is_disp else 0)
    return edge, stats


def distance_transform(maps, gts, indices, backend=None):
    """Exact SQUARED Euclidean distance (int32 [n, px_stride]) of every pixel to the nearest non-zero byte of
    maps[i] (uint8 [n, px_stride], image i shaped as gts[indices[i]]): scipy's distance_transform_edt(1 - map) ** 2.
    A map without a non-zero byte gives 2 ** 30 everywhere."""
    backend = backend or ops.default_backend()
    assert maps.dtype == torch.uint8 and maps.dim() == 2 and maps.is_contiguous()
    backend._check(maps)
    max_h, max_w, px_stride = syns_strides(gts)
    assert maps.shape[1] == px_stride
    idx = torch.as_tensor(indices, dtype=torch.long, device=gts.desc.device).view(-1)
    assert idx.numel() == maps.shape[0]
    desc = gts.desc.index_select(0, idx).contiguous()
    out = torch.zeros(maps.shape, dtype=torch.int32, device=maps.device)
    backend.run("bbd_syns_edt", maps, ptr(maps), ptr(desc), ptr(out), maps.shape[0], px_stride, max_h, max_w)
    return out


def _eval_flags(pred_is_disp, median_scaling):
    return (EVAL_PRED_IS_DISP if pred_is_disp else 0) | (0 if median_scaling else EVAL_NO_MEDIAN_SCALING)


def edge_metrics(pred, gts, indices, edge, rows, min_depth=SYNS_MIN_DEPTH, max_depth=SYNS_MAX_DEPTH,
                 clamp=(1e-3, 80.0), pred_is_disp=False, median_scaling=True, scale_factor=1.0, th=SYNS_EDGE_TH,
                 backend=None):
    """evaluate_depth.py:72-73, :89-95: float64 [n, 8] = edge_Acc, edge_comp, err, count(near), count(target),
    count(valid), count(predicted edge), 0.  `edge` is `pred_edges`' map, `rows` the `depth_metrics` rows of the same
    batch (their ratio is read on the device).  Both edge metrics are `th` when no predicted edge lies within `th`
    of a target edge, and NaN when the image has no valid ground-truth edge pixel at all: scipy's transform of a map
    without background is an artefact of its implementation, not a distance."""
    assert gts.edges is not None, "this GroundTruthSet was built without edge maps"
    c = _SynsCall(pred, gts, indices, backend)
    assert edge.dtype == torch.uint8 and edge.shape == (c.n, c.px_stride) and edge.is_contiguous()
    assert rows.dtype == torch.float32 and rows.shape == (c.n, EVAL_OUT) and rows.is_contiguous()
    c.backend._check(edge, rows, gts.edges)
    out = torch.empty(c.n, SYNS_OUT, dtype=torch.float64, device=c.pred.device)
    scratch = c.scratch()
    c.backend.run("bbd_syns_edge_metrics", c.pred, ptr(c.pred), ptr(gts.buffer), ptr(gts.edges), ptr(edge), ptr(c.desc),
                  ptr(rows), ptr(scratch), c.n_ints, ptr(out), *c.sizes(), float(min_depth), float(max_depth),
                  float(clamp[0]), float(clamp[1]), float(scale_factor), float(th),
                  _eval_flags(pred_is_disp, median_scaling))
    return out


def pointcloud_metrics(pred, gts, indices, rows, inv_K, min_depth=SYNS_MIN_DEPTH, max_depth=SYNS_MAX_DEPTH,
                       clamp=(1e-3, 80.0), pred_is_disp=False, median_scaling=True, rays="reference",
                       th=SYNS_CLOUD_TH, backend=None):
    """evaluate_depth.py:74-85 with `--chamfer`: float32 [n, 8] = f1, iou, precision, recall, count(pred within th),
    count(gt within th), points per cloud, 0.  Both clouds hold the valid ground-truth pixels only.

    rays="reference" pairs flat pixel k (row-major) with the ray of pixel (k // GH, k % GH): the reference builds its
    grid with torch.meshgrid(arange(w), arange(h)) in ij order and flattens it against the row-major depth map, so
    every published number carries that pairing.  rays="pixel" uses the pixel's own ray (k % GW, k // GW)."""
    assert rays in ("reference", "pixel")
    c = _SynsCall(pred, gts, indices, backend)
    assert rows.dtype == torch.float32 and rows.shape == (c.n, EVAL_OUT) and rows.is_contiguous()
    iK = torch.as_tensor(np.asarray(inv_K, dtype=np.float32)[:3, :3].copy()).contiguous().to(c.pred.device)
    c.backend._check(rows, iK)
    out = torch.empty(c.n, SYNS_CLOUD_OUT, dtype=torch.float32, device=c.pred.device)
    scratch = c.scratch()
    c.backend.run("bbd_syns_pointcloud", c.pred, ptr(c.pred), ptr(gts.buffer), ptr(c.desc), ptr(rows), ptr(iK),
                  ptr(scratch), c.n_ints, ptr(out), *c.sizes(), float(min_depth), float(max_depth), float(clamp[0]),
                  float(clamp[1]), float(th),
                  _eval_flags(pred_is_disp, median_scaling) | (SYNS_RAYS_PIXEL if rays == "pixel" else 0))
    return out


def syns_metrics(pred, gts, indices, inv_K=None, chamfer=False, mode="evaluate", median_scaling=True,
                 scale_factor=1.0, rays="reference", backend=None, return_rows=False):
    """One SYNS-Patches row per image, float64 [n, 9] on the device, in the reference's column order
    (`SYNS_COLUMNS`): abs_rel, err, sq_rel, rmse, rmse_log, edge_Acc, edge_comp, f1, iou1; the last two are NaN
    without `chamfer`.  Nothing synchronises with the host.

    mode="evaluate" is evaluate_depth.py: `pred` is a disparity, resized as cv2 does, depth range (1e-3, 125),
    np.median scaling, no crop.  mode="trainer" is Trainer.compute_depth_losses(SYNS=True) (trainer.py:576-617):
    `pred` is a depth, F.interpolate then clamp to [1e-3, 80], depth range (1e-3, 80), torch.median.
    `gts` must have been built with `crop=False` and `edges=`."""
    assert mode in ("evaluate", "trainer")
    ev = mode == "evaluate"
    lo, hi = (SYNS_MIN_DEPTH, SYNS_MAX_DEPTH) if ev else (1e-3, 80.0)
    rows = depth_metrics(pred, gts, indices, min_depth=lo, max_depth=hi, pred_is_disp=ev,
                         median="numpy" if ev else "torch", median_scaling=median_scaling, scale_factor=scale_factor,
                         backend=backend)
    edge, _ = pred_edges(pred, gts, indices, pred_is_disp=ev, backend=backend)
    em = edge_metrics(pred, gts, indices, edge, rows, min_depth=lo, max_depth=hi, pred_is_disp=ev,
                      median_scaling=median_scaling, scale_factor=scale_factor, backend=backend)
    out = torch.full((rows.shape[0], 9), float("nan"), dtype=torch.float64, device=rows.device)
    r64 = rows.double()
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = r64[:, 0], em[:, 2], r64[:, 1], r64[:, 2], r64[:, 3]
    out[:, 5], out[:, 6] = em[:, 0], em[:, 1]
    if chamfer:
        assert inv_K is not None, "the point-cloud metrics need the camera's inverse intrinsics"
        pc = pointcloud_metrics(pred, gts, indices, rows, inv_K, min_depth=lo, max_depth=hi, pred_is_disp=ev,
                                median_scaling=median_scaling, rays=rays, backend=backend)
        out[:, 7], out[:, 8] = pc[:, 0].double(), pc[:, 1].double()
    return (out, rows) if return_rows else out


# ---------------------------------------------------------------------------- evaluate_depth.py
STEREO_SCALE_FACTOR = 5.4          # evaluate_depth.py:45


def evaluate(opt, dataloader=None, gt_depths=None, models=None, batch_size=16, gt_edges=None, inv_K=None, backend=None,
             device=None):
    """KITTI branch of the reference's `evaluate(opt)` (evaluate_depth.py:104-317) for the ResNet and MonoViT (`--ViT`) models:
    predicts disparities for a split, scores them against `gt_depths.npz` with median (mono) or 5.4x
    (stereo) scaling, returns (mean_errors[7], ratios).  Differences by design: images are prepared by the
    device loader and each batch is scored by one `bbd_depth_metrics` launch while it is still in HBM
    (the reference copies every disparity map to the host, resizes with cv2 and runs numpy per image).

    `dataloader` / `gt_depths` / `models` may be injected (tests, synthetic splits); by default they are
    built from `opt.splits_dir/<eval_split>/{test_files.txt, gt_depths.npz}`, `opt.kt_path` and
    `opt.load_weights_folder`.  Where `gt_depths.npz` does not exist (the reference ships none) and the split is `eigen`
    or `eigen_zhou`, the ground truth is projected from the Velodyne scans under `opt.kt_path` on the device
    (`kitti_utils.generate_depth_maps`: what `export_gt_depth.py` writes, without the file).

    `opt.eval_split == "SYNS"` is the reference's SYNS-Patches branch: frames from `opt.syns_path`, `gt_depths.npz` and
    `gt_edges.npz` from the split directory (or `gt_depths` / `gt_edges`), depth range (1e-3, 125), no crop, and the
    7-column table abs_rel, err, sq_rel, rmse, rmse_log, edge_Acc, edge_comp - 9 columns with f1 and iou1 under
    `opt.chamfer` (`syns_metrics`).  Returns (mean_errors[7 or 9], ratios).

    Four options of the Monodepth2 family, each read with a default so that an `opt` without them behaves as before
    (DESIGN.md 6e), in both branches:
      `post_process`      every batch goes through the networks together with its left-right flipped copy and the two
                          predictions are blended by `ops.post_process_disp`; the blended disparities are scored.
      `save_pred_disps`   the scored disparities stay on the device, are concatenated and copied to the host once and
                          written to `<load_weights_folder>/disps_<eval_split>_split.npy` as float32 [N,h,w].
      `ext_disp_to_eval`  path of such a file: its disparities are scored instead of predictions - no weights, no
                          dataset, no loader.  `post_process` and `save_pred_disps` concern predictions and do nothing.
      `no_eval`           stop after the predictions (and the optional save): no ground truth is loaded, nothing is
                          scored, (None, None) is returned.

    `save_clouds` (a directory) writes, for the first `cloud_count` (8) images of the split, the point
    clouds the evaluation sees as binary PLY files `<index:04d>_pred.ply` and `<index:04d>_gt.ply`, exported by
    `ops.point_cloud` while the batch is in HBM: the prediction scaled by the ratio of the image's metrics row and
    clamped to the split's depth range, and the ground truth, both on the pixels the split scores (valid ground truth,
    inside the Garg window on KITTI), every `cloud_stride`-th of them, coloured by inverse depth.  KITTI takes the KITTI
    intrinsics at the ground-truth size, SYNS the dataset's; `cloud_rays` ("pixel" | "reference") chooses the pairing of
    pixels and rays (`pointcloud_metrics`).  It needs the metrics rows, so it is refused together with `no_eval`.

    `scale_recovery` ("median" | "ground" | "lsq"): under "ground" a KITTI mono prediction is scaled without
    ground truth - every batch goes through `ops.ground_scale` with the KITTI intrinsics of the prediction's own size
    (`camera_height` 1.65, `ground_angle` 5.0), its disparities are divided on the device by the scale of their image
    and scored without median scaling; `save_clouds` exports those scaled disparities.  The ratios line and the
    returned ratios are the recovered scales; an image without ground has a NaN scale, is named in a warning and left
    out of the mean.  Refused with `eval_stereo`, `disable_median_scaling` and the SYNS split.

    `scale_recovery` "lsq"  is the protocol of the relative-depth models (MiDaS, DPT, Depth Anything),
    whose disparity is known up to a scale AND a shift: every batch is scored by one `bbd_depth_metrics_affine` launch
    (`depth_metrics_affine`) in place of `bbd_depth_metrics` - per image the least-squares scale and shift that map the
    prediction to the inverse ground truth on the scored pixels, the aligned disparity capped at 1 / 80, then the seven
    errors, SILog and iRMSE - and the rows are read back once.  Printed: a warning that names the images that could not
    be aligned (fewer than two scored pixels, a constant or a non-finite prediction; left out of the means), a warning
    that names the images with scale <= 0 (scored, in the means), ` Alignment | scale med | shift med` in place of the
    ratios line, the seven-metric table, and a line with silog (percent) and irmse (1/km).  Returns (mean_errors[7],
    alignment [N, 2] = scale and shift, NaN rows for the images without alignment).  `post_process`,
    `save_pred_disps` (the unaligned disparities), `ext_disp_to_eval` and `no_eval` behave as under "median".  Refused
    (`options.alignment_conflict`) with `eval_stereo`, `disable_median_scaling`, a `pred_depth_scale_factor` other
    than 1, the SYNS split, `save_clouds` and the uncertainty options: their kernels read the median ratio of a
    metrics row and know no shift.

    Uncertainty (KITTI splits only), each field read with a default:
      `uncertainty`        "none" | "post": under "post" every batch runs with its flipped copy (`post_process` is
                           implied), the blended disparity is scored and |d - flip(d')| - the "Post" uncertainty of Poggi
                           et al. - comes out of the same `ops.post_process_uncert` launch.  Every batch then gets one
                           `ops.sparsification` call right after `depth_metrics`; its rows are read back with the metrics
                           rows, once.  After the metrics table a table of AUSE and AURG for abs_rel, rmse and a1 is
                           printed: the mean over the images that have a scored pixel (the others are named).
      `ext_uncert_to_eval` a float [N,h,w] .npy with the uncertainties of the disparities of `ext_disp_to_eval`.
      `save_pred_uncerts`  writes `uncerts_<eval_split>_split.npy` next to `disps_<eval_split>_split.npy`.
      `sparsification_intervals` (50) and `save_sparsification` (a .json: the mean curves and the six numbers).
    With an uncertainty, (mean_errors, ratios, scores) is returned, `scores` being the dict `save_sparsification`
    writes.  Refused with the SYNS split, `no_eval` and `scale_recovery ground`.

    `backend` and `device` are for tests (the host ports); by default the HIP backend and `cuda:<opt.cuda>`."""
    _align_options(opt)                                                  # raises before anything is touched
    uncert = _uncert_options(opt)                                        # as well
    from . import tuning
    tuning.use_shipped_db()      # (no Trainer is built here: the tuned MIOpen database is wired explicitly)
    import os
    from . import datasets, networks

    assert sum((opt.eval_mono, opt.eval_stereo)) == 1, \
        "Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo"
    device = torch.device("cuda:%d" % getattr(opt, "cuda", 0)) if device is None else torch.device(device)
    ext = getattr(opt, "ext_disp_to_eval", None)
    no_eval = bool(getattr(opt, "no_eval", False))
    clouds = _CloudSaver.from_options(opt, no_eval, backend)             # raises before any prediction
    _ground_options(opt)                                                 # as well
    split_dir = os.path.join(getattr(opt, "splits_dir", "splits"), opt.eval_split)
    syns = opt.eval_split == "SYNS"

    def score(source, save_path):
        if syns:
            return _evaluate_syns(opt, source, save_path, no_eval, gt_depths, gt_edges, inv_K, split_dir, device,
                                  backend, clouds)
        return _evaluate_kitti(opt, source, save_path, no_eval, gt_depths, split_dir, device, backend, clouds, uncert)

    if ext is not None:
        return score(_ExternalDisps(ext, batch_size, device, uncert["ext"] if uncert else None), None)
    if uncert is not None and uncert["save"]:
        uncert["save_path"] = _disps_path(opt).replace("disps_", "uncerts_")               # raises before any prediction
    save_path = _disps_path(opt) if getattr(opt, "save_pred_disps", False) else None      # raises before any prediction
    if models is None:
        folder = os.path.expanduser(opt.load_weights_folder)
        assert os.path.isdir(folder), "Cannot find a folder at {}".format(folder)
        enc_dict = torch.load(os.path.join(folder, "encoder.pth"), map_location=device)
        height, width = enc_dict["height"], enc_dict["width"]
        if getattr(opt, "ViT", False):                  # MonoViT checkpoints (evaluate_depth.py:141-149)
            from . import networksvit
            encoder = networksvit.mpvit_small(checkpoint=None)
            encoder.num_ch_enc = [64, 128, 216, 288, 288]
            decoder = networksvit.DepthDecoder()
        else:
            encoder = networks.ResnetEncoder(opt.num_layers, False)
            decoder = networks.DepthDecoder(encoder.num_ch_enc)
        own = encoder.state_dict()
        encoder.load_state_dict({k: v for k, v in enc_dict.items() if k in own})
        decoder.load_state_dict(torch.load(os.path.join(folder, "depth.pth"), map_location=device), strict=False)
    else:
        encoder, decoder = models
        height, width = opt.height, opt.width
    encoder.to(device).eval()
    decoder.to(device).eval()
    if dataloader is None:
        filenames = datasets.readlines(os.path.join(split_dir, "test_files.txt"))
        if syns:                                         # evaluate_depth.py:128-132
            ds = datasets.SYNSRAWDataset(filenames, 0, height, width, syns_path=opt.syns_path, is_train=False,
                                         naive_mix=True)
        else:
            ds = datasets.KITTIRAWDataset(filenames, 0, height, width, kt_path=opt.kt_path, is_train=False, kt=True,
                                          naive_mix=True)
        dataloader = datasets.DeviceLoader(ds, batch_size, datasets.DeviceCollate(height, width, [0], device),
                                           shuffle=False, drop_last=False, num_workers=getattr(opt, "num_workers", 8))
    if uncert is not None:
        print("-> uncertainty post: every batch runs with its flipped copy (post_process is implied)")
    post_process = bool(getattr(opt, "post_process", False)) or uncert is not None
    return score(_PredictedDisps(opt, dataloader, encoder, decoder, post_process, uncert is not None, backend), save_path)


class _PredictedDisps:
    """The disparities that are scored, batch by batch on the device: `disp_to_depth` of the networks' output and, with
    `post_process`, the flip blend of the batch and its mirrored copy ([n,h,w] then, [n,1,h,w] otherwise).  With `uncert`
    every item is the pair (blended disparities, their uncertainty), both from one `ops.post_process_uncert` launch."""
    count = None                 # known only after the loader has run dry

    def __init__(self, opt, dataloader, encoder, decoder, post_process, uncert=False, backend=None):
        self.opt, self.dataloader, self.encoder, self.decoder = opt, dataloader, encoder, decoder
        self.post_process, self.uncert, self.backend = post_process, uncert, backend

    def __iter__(self):
        from .layers import disp_to_depth
        for data in self.dataloader:
            x = data[("color", 0, 0)]
            if self.post_process:
                x = torch.cat((x, torch.flip(x, [3])), 0)
            out = self.decoder(self.encoder(x))
            pred_disp, _ = disp_to_depth(out[("disp", 0)], self.opt.min_depth, self.opt.max_depth)
            if self.uncert:
                yield ops.post_process_uncert(pred_disp, backend=self.backend)
            else:
                yield ops.post_process_disp(pred_disp, backend=self.backend) if self.post_process else pred_disp


class _ExternalDisps:
    """Disparities of a saved file (`--ext_disp_to_eval`): a numeric [N,h,w] array, cast to float32 and uploaded in
    batches of `batch_size`.  With `uncert_path` (`--ext_uncert_to_eval`: a file of the same shape, checked the same way)
    every item is the pair (disparities, their uncertainties)."""

    def __init__(self, path, batch_size, device, uncert_path=None):
        arr = self._load(path, "ext_disp_to_eval")
        self.uncert = None
        if uncert_path is not None:
            self.uncert = self._load(uncert_path, "ext_uncert_to_eval")
            if self.uncert.shape != arr.shape:
                raise ValueError("ext_uncert_to_eval: %s holds %s, the disparities of %s are %s"
                                 % (uncert_path, self.uncert.shape, path, arr.shape))
        print("-> Loading predictions from {}".format(path))
        if uncert_path is not None:
            print("-> Loading uncertainties from {}".format(uncert_path))
        self.arr, self.batch_size, self.device, self.count = arr, max(1, int(batch_size)), device, arr.shape[0]

    @staticmethod
    def _load(path, what):
        arr = np.load(path)
        if not isinstance(arr, np.ndarray) or arr.ndim != 3 or arr.dtype.kind not in "fiu" or 0 in arr.shape:
            raise ValueError("%s: %s must hold a numeric [N,h,w] array, got %s"
                             % (what, path, "%s %s" % (arr.dtype, arr.shape) if isinstance(arr, np.ndarray) else type(arr)))
        return arr

    def _chunk(self, arr, first):
        return torch.from_numpy(np.ascontiguousarray(arr[first:first + self.batch_size], dtype=np.float32)).to(self.device)

    def __iter__(self):
        for first in range(0, self.count, self.batch_size):
            if self.uncert is None:
                yield self._chunk(self.arr, first)
            else:
                yield self._chunk(self.arr, first), self._chunk(self.uncert, first)


def _disps_path(opt):
    """Where `save_pred_disps` writes (Monodepth2: disps_<split>_split.npy in the weights folder)."""
    import os
    folder = getattr(opt, "load_weights_folder", None)
    if folder is None or str(folder) == "None":
        raise ValueError("save_pred_disps writes into load_weights_folder, which is not set")
    return os.path.join(os.path.expanduser(str(folder)), "disps_{}_split.npy".format(opt.eval_split))


def _save_disps(kept, save_path):
    """All scored disparities as ONE float32 [N,h,w] array: concatenated on the device, one copy to the host."""
    disps = torch.cat([d[:, 0] if d.dim() == 4 else d for d in kept]).float().cpu().numpy()
    print("-> Saving predicted disparities to ", save_path)
    np.save(save_path, disps)


def _predict_only(source, save_path):
    """`no_eval`: the predictions and the optional save, nothing else (a saved file is only checked, not uploaded)."""
    kept = []
    with torch.no_grad():
        for pred_disp in (() if isinstance(source, _ExternalDisps) else source):
            if save_path is not None:
                kept.append(pred_disp)
    if save_path is not None:
        _save_disps(kept, save_path)
    print("-> Evaluation disabled. Done.")
    return None, None


def _check_count(source, gts):
    if source.count is not None and source.count != len(gts):
        raise ValueError("ext_disp_to_eval holds %d disparity maps, the ground truth of the split %d"
                         % (source.count, len(gts)))


class _CloudSaver:
    """`save_clouds`: the prediction and ground-truth clouds of the first `count` images of a split, written as
    `<index:04d>_pred.ply` / `<index:04d>_gt.ply` batch by batch.  Two `ops.point_cloud` calls and one read-back each
    per batch that still holds wanted images; nothing at all afterwards."""

    def __init__(self, folder, count, stride, rays, backend):
        self.folder, self.count, self.stride, self.rays, self.backend = folder, int(count), int(stride), rays, backend
        self.written = []

    @classmethod
    def from_options(cls, opt, no_eval, backend):
        folder = getattr(opt, "save_clouds", None)
        if folder is None:
            return None
        if no_eval:
            raise ValueError("save_clouds needs the evaluation: the clouds are scaled by the median-scaling ratio of each "
                             "image's metrics row, and no_eval produces no metrics rows")
        count, stride = int(getattr(opt, "cloud_count", 8)), int(getattr(opt, "cloud_stride", 1))
        rays = getattr(opt, "cloud_rays", "pixel")
        if count < 1 or stride < 1 or rays not in ("pixel", "reference"):
            raise ValueError("save_clouds: cloud_count and cloud_stride must be at least 1 and cloud_rays pixel or "
                             "reference, got %r, %r, %r" % (count, stride, rays))
        return cls(str(folder), count, stride, rays, backend)

    def batch(self, pred_disp, gts, first, rows, inv_K, min_depth, max_depth, scale_factor, median_scaling):
        """Images first .. first + n - 1 of the split are in `pred_disp`; `rows` are their metrics rows."""
        import os
        from . import pointcloud
        n = min(pred_disp.shape[0], self.count - first)
        if n <= 0:
            return
        os.makedirs(self.folder, exist_ok=True)
        idx = list(range(first, first + n))
        desc = gts.desc_host[idx]
        if inv_K is None:                              # KITTI: the datasets' matrix at every map's own size
            inv_K = np.stack([pointcloud.intrinsics(*gts.shapes[i]) for i in idx])
        kw = dict(gt=gts.buffer, stride=self.stride, min_depth=min_depth, max_depth=max_depth, mask_gt=True,
                  rays=self.rays, backend=self.backend)
        pred = ops.point_cloud(pred_disp[:n], desc, inv_K, rows=rows[:n].contiguous() if median_scaling else None,
                               pred_is_disp=True, scale_factor=scale_factor, clamp_depth=True, **kw)
        truth = ops.point_cloud(pred_disp[:n], desc, inv_K, from_gt=True, **kw)
        for name, cloud in (("pred", pred), ("gt", truth)):
            for i, arr in zip(idx, pointcloud.cloud_arrays(*cloud)):
                self.written.append(pointcloud.write_ply(os.path.join(self.folder, "%04d_%s.ply" % (i, name)), arr))

    def done(self):
        if self.written:
            print("-> Saved {:d} point clouds to {}".format(len(self.written), self.folder))


def _ground_options(opt):
    """`scale_recovery == "ground"` -> the keywords of `ops.ground_scale`; "median" (or an `opt` without the field) and
    "lsq" (which has options of its own: `_align_options`) -> None.  What the scale would collide with is refused."""
    mode = getattr(opt, "scale_recovery", "median")
    if mode in ("median", "lsq"):                         # lsq: `_align_options`
        return None
    if mode != "ground":
        raise ValueError("scale_recovery is median or ground, got %r" % (mode,))
    for name, set_ in (("eval_stereo", opt.eval_stereo), ("disable_median_scaling", opt.disable_median_scaling),
                       ("eval_split SYNS", opt.eval_split == "SYNS")):
        if set_:
            raise ValueError("scale_recovery ground scales a mono prediction on a KITTI split by the camera's height "
                             "above the road: it excludes %s" % name)
    return dict(camera_height=float(getattr(opt, "camera_height", 1.65)), angle_deg=float(getattr(opt, "ground_angle", 5.0)))


def _ground_summary(rows, ground_rows):
    """The printed summary and the result of a split scored under `scale_recovery ground`: the mean over the images
    that have a scale - the others are counted and named - and the ratios line from the ground rows."""
    ratios = ground_rows[:, 7]
    found = np.isfinite(ratios)
    if not found.all():
        lost = np.nonzero(~found)[0]
        print("   WARNING: no ground found in {:d} of {:d} images, left out of the mean: {}".format(
            len(lost), len(ratios), ", ".join(str(i) for i in lost)))
    if found.any():
        med = np.median(ratios[found])
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios[found] / med)))
    mean_errors = rows[found, :7].mean(0) if found.any() else np.full(7, np.nan)
    print("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    return mean_errors, ratios


def _align_options(opt):
    """Is the split scored under `scale_recovery lsq`?  What that collides with is refused
    (`options.alignment_conflict`)."""
    from .options import alignment_conflict
    conflict = alignment_conflict(opt)
    if conflict:
        raise ValueError(conflict)
    return getattr(opt, "scale_recovery", "median") == "lsq"


def _align_summary(rows):
    """The printed summary and the result of a split scored under `scale_recovery lsq` from its float64 rows
    [N, 12] (`ALIGN_COLUMNS`): the mean over the images that could be aligned - the others are counted and named - and
    the alignment line in place of the ratios line.  Returns (mean_errors[7], alignment [N, 2] = scale, shift)."""
    alignment = rows[:, 7:9].copy()
    fitted = ~np.isnan(rows[:, :10]).any(1) & ~np.isnan(rows[:, 11])
    if not fitted.all():
        lost = np.nonzero(~fitted)[0]
        print("   WARNING: no alignment for {:d} of {:d} images (fewer than two scored pixels, a constant or a non-finite "
              "prediction), left out of the means: {}".format(len(lost), len(rows), ", ".join(str(i) for i in lost)))
    with np.errstate(invalid="ignore"):
        flipped = np.nonzero(fitted & (rows[:, 7] <= 0))[0]
    if len(flipped):
        print("   WARNING: scale <= 0 in {:d} of {:d} images - the prediction is anti-correlated with the inverse ground "
              "truth; they are scored and stay in the means: {}".format(len(flipped), len(rows),
                                                                        ", ".join(str(i) for i in flipped)))
    if fitted.any():
        print(" Alignment | scale med: {:0.4g} | shift med: {:0.4g}".format(np.median(rows[fitted, 7]),
                                                                          np.median(rows[fitted, 8])))
    mean = rows[fitted].mean(0) if fitted.any() else np.full(rows.shape[1], np.nan)
    mean_errors = mean[:7]
    print("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    print("  " + ("{:>8} | " * 2).format("silog", "irmse"))
    print(("&{: 8.3f}  " * 2).format(mean[9], mean[11]) + "\\\\")
    return mean_errors, alignment


UNCERT_METRICS = ("abs_rel", "rmse", "a1")


def _uncert_options(opt):
    """The uncertainty options of `opt` -> None (none asked for) or dict(ext, save, intervals, json); what they collide
    with is refused (`options.uncertainty_conflict`)."""
    from .options import uncertainty_conflict
    conflict = uncertainty_conflict(opt)
    if conflict:
        raise ValueError(conflict)
    ext = getattr(opt, "ext_uncert_to_eval", None)
    if getattr(opt, "uncertainty", "none") != "post" and ext is None:
        return None
    return dict(ext=ext, save=bool(getattr(opt, "save_pred_uncerts", False)), save_path=None,
                intervals=int(getattr(opt, "sparsification_intervals", 50)), json=getattr(opt, "save_sparsification", None))


def sparsification_scores(spars, intervals):
    """The scores of a split from the float64 rows [N, 8 + 6 (K + 1)] of `ops.sparsification`: the mean over the images
    that have a scored pixel of AUSE, AURG and the six curves; `skipped` lists the others."""
    K = int(intervals)
    spars = np.asarray(spars, np.float64)
    has = spars[:, 6] > 0
    with np.errstate(invalid="ignore"):
        mean = spars[has].mean(0) if has.any() else np.full(spars.shape[1], np.nan)
    curves = mean[8:].reshape(2, 3, K + 1)
    return dict(intervals=K, images=int(has.sum()), skipped=[int(i) for i in np.nonzero(~has)[0]],
                fractions=[k / K for k in range(K + 1)],
                ause={m: float(mean[j]) for j, m in enumerate(UNCERT_METRICS)},
                aurg={m: float(mean[3 + j]) for j, m in enumerate(UNCERT_METRICS)},
                curves={name: {m: curves[w, j].tolist() for j, m in enumerate(UNCERT_METRICS)}
                        for w, name in enumerate(("sparse", "oracle"))})


def _uncert_summary(spars, uncert):
    """Prints the AUSE / AURG table of a split and writes `save_sparsification`; returns the scores."""
    scores = sparsification_scores(spars, uncert["intervals"])
    if scores["skipped"]:
        print("   WARNING: no scored pixel in {:d} of {:d} images, left out of the uncertainty scores: {}".format(
            len(scores["skipped"]), len(spars), ", ".join(str(i) for i in scores["skipped"])))
    print("\n  Uncertainty, sparsification at {:d} fractions (AUSE: lower is better, AURG: higher is better)".format(
        scores["intervals"]))
    print("  " + "{:>8} | ".format("") + ("{:>8} | " * 3).format(*UNCERT_METRICS))
    for name in ("ause", "aurg"):
        values = [scores[name][m] for m in UNCERT_METRICS]
        print("  " + "{:>8} | ".format(name.upper()) + ("{: 8.4f} | " * 3).format(*values))
    if uncert["json"] is not None:
        import json
        with open(uncert["json"], "w") as f:
            json.dump(scores, f, indent=1)
        print("-> Saved the sparsification curves to ", uncert["json"])
    return scores


def _evaluate_kitti(opt, source, save_path, no_eval, gt_depths, split_dir, device, backend=None, clouds=None, uncert=None):
    """The KITTI splits: every batch of `source` is scored by one `bbd_depth_metrics` launch while it is in HBM - and,
    with `uncert`, its uncertainty maps by one `bbd_sparsification` launch right after."""
    import os
    if no_eval:
        return _predict_only(source, save_path)
    gt_path = os.path.join(split_dir, "gt_depths.npz")
    if gt_depths is None and not os.path.isfile(gt_path) and opt.eval_split in ("eigen", "eigen_zhou"):
        # what export_gt_depth.py would have written, straight into the device buffer the metrics read
        from . import kitti_utils
        frames = kitti_utils.split_frames(split_dir, opt.eval_split, opt.kt_path)
        print("-> %s not found: ground truth of %d frames projected from the Velodyne scans under %s on the device"
              % (gt_path, len(frames), opt.kt_path))
        gt_depths = kitti_utils.generate_depth_maps(frames, device, vel_depth=True)
    if gt_depths is None:
        gt_depths = np.load(gt_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
    gts = gt_depths if isinstance(gt_depths, GroundTruthSet) else GroundTruthSet(gt_depths, device)
    _check_count(source, gts)

    median_scaling = not opt.disable_median_scaling
    scale = opt.pred_depth_scale_factor
    if opt.eval_stereo:                                   # evaluate_depth.py:233-237
        median_scaling, scale = False, STEREO_SCALE_FACTOR
    ground = _ground_options(opt)
    if ground is not None:                                # the scale comes from the ground rows: nothing else scales
        median_scaling, scale = False, 1
    rows, ground_rows, kept, first = [], [], [], 0
    spars, kept_uncerts = [], []
    if _align_options(opt):                               # the fit is the scaling: one launch per batch, its own rows
        with torch.no_grad():
            for pred_disp in source:
                n = pred_disp.shape[0]
                if save_path is not None:
                    kept.append(pred_disp)                # the unaligned disparities
                rows.append(depth_metrics_affine(pred_disp, gts, list(range(first, first + n)), min_depth=1e-3,
                                                 max_depth=80.0, backend=backend))
                first += n
        if save_path is not None:
            _save_disps(kept, save_path)
        rows = torch.cat(rows).cpu().numpy()              # the only host synchronisation of the scoring
        assert first == len(gts), "split has %d images, ground truth %d" % (first, len(gts))
        return _align_summary(rows)
    with torch.no_grad():
        for pred_disp in source:
            if uncert is not None:
                pred_disp, uncert_map = pred_disp
                if uncert["save_path"] is not None:
                    kept_uncerts.append(uncert_map)
            n = pred_disp.shape[0]
            if save_path is not None:
                kept.append(pred_disp)
            if ground is not None:
                from . import pointcloud
                ground_rows.append(ops.ground_scale(pred_disp, pointcloud.intrinsics(*pred_disp.shape[-2:]),
                                                    pred_is_disp=True, backend=backend, **ground)[0])
                # metres = scale / disparity: the disparities are divided by the scale, a NaN scale leaves NaNs
                pred_disp = pred_disp / ground_rows[-1][:, 7].view([n] + [1] * (pred_disp.dim() - 1))
            rows.append(depth_metrics(pred_disp, gts, list(range(first, first + n)), min_depth=1e-3, max_depth=80.0,
                                      pred_is_disp=True, median="numpy", median_scaling=median_scaling,
                                      scale_factor=scale, backend=backend))
            if uncert is not None:
                spars.append(ops.sparsification(pred_disp, uncert_map, gts, list(range(first, first + n)), rows[-1],
                                                intervals=uncert["intervals"], min_depth=1e-3, max_depth=80.0,
                                                scale_factor=scale, median_scaling=median_scaling, backend=backend))
            if clouds is not None:
                clouds.batch(pred_disp, gts, first, rows[-1], None, 1e-3, 80.0, scale, median_scaling)
            first += n
    if save_path is not None:
        _save_disps(kept, save_path)
    if kept_uncerts:
        print("-> Saving predicted uncertainties to ", uncert["save_path"])
        np.save(uncert["save_path"], torch.cat(kept_uncerts).float().cpu().numpy())
    if clouds is not None:
        clouds.done()
    rows = torch.cat(rows)
    if ground is not None:                                # the ground rows travel with the metrics rows
        rows = torch.cat([rows, torch.cat(ground_rows)], 1)
    if uncert is not None:                                # so do the sparsification rows: float32 widens exactly
        rows = torch.cat([rows.double(), torch.cat(spars)], 1)
    rows = rows.cpu().numpy().astype(np.float64)                     # the only host synchronisation of the scoring
    assert first == len(gts), "split has %d images, ground truth %d" % (first, len(gts))
    if ground is not None:
        return _ground_summary(rows[:, :EVAL_OUT], rows[:, EVAL_OUT:])
    rows, spars = rows[:, :EVAL_OUT], rows[:, EVAL_OUT:]
    mean_errors = rows[:, :7].mean(0)
    ratios = rows[:, 7] if median_scaling else None
    if median_scaling:
        med = np.median(ratios)
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    print("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    if uncert is not None:
        return mean_errors, ratios, _uncert_summary(spars, uncert)
    return mean_errors, ratios


def _evaluate_syns(opt, source, save_path, no_eval, gt_depths, gt_edges, inv_K, split_dir, device, backend=None,
                   clouds=None):
    """evaluate_depth.py with `--eval_split SYNS [--chamfer]`: every batch is scored while it is in HBM; the rows are
    read back once, at the end."""
    import os
    from . import datasets
    if no_eval:
        return _predict_only(source, save_path)
    if gt_depths is None:
        gt_depths = np.load(os.path.join(split_dir, "gt_depths.npz"), fix_imports=True, encoding="latin1",
                            allow_pickle=True)["data"]
    if gt_edges is None and not isinstance(gt_depths, GroundTruthSet):
        gt_edges = np.load(os.path.join(split_dir, "gt_edges.npz"), fix_imports=True, encoding="latin1",
                           allow_pickle=True)["data"]
    gts = gt_depths if isinstance(gt_depths, GroundTruthSet) else GroundTruthSet(gt_depths, device, crop=False,
                                                                                 edges=gt_edges)
    _check_count(source, gts)
    chamfer = bool(getattr(opt, "chamfer", False))
    if (chamfer or clouds is not None) and inv_K is None:
        inv_K = datasets.SYNSRAWDataset.load_intrinsic_syns()[1]
    median_scaling = not opt.disable_median_scaling
    scale = opt.pred_depth_scale_factor
    if opt.eval_stereo:
        median_scaling, scale = False, STEREO_SCALE_FACTOR
    out, ratio_rows, kept, first = [], [], [], 0
    with torch.no_grad():
        for pred_disp in source:
            n = pred_disp.shape[0]
            if save_path is not None:
                kept.append(pred_disp)
            res, rows = syns_metrics(pred_disp, gts, list(range(first, first + n)), inv_K=inv_K, chamfer=chamfer,
                                     mode="evaluate", median_scaling=median_scaling, scale_factor=scale,
                                     return_rows=True, backend=backend)
            out.append(res)
            ratio_rows.append(rows[:, 7])
            if clouds is not None:
                # as the clouds of the F-score: without opt.pred_depth_scale_factor (bbd_syns_pointcloud)
                clouds.batch(pred_disp, gts, first, rows, inv_K, SYNS_MIN_DEPTH, SYNS_MAX_DEPTH, 1.0, median_scaling)
            first += n
    if save_path is not None:
        _save_disps(kept, save_path)
    if clouds is not None:
        clouds.done()
    out = torch.cat(out).cpu().numpy()                                  # the only host synchronisation of the scoring
    ratios = torch.cat(ratio_rows).cpu().numpy().astype(np.float64) if median_scaling else None
    assert first == len(gts), "split has %d images, ground truth %d" % (first, len(gts))
    ncol = 9 if chamfer else 7
    mean_errors = out[:, :ncol].mean(0)
    if median_scaling:
        med = np.median(ratios)
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    print("\n  " + ("{:>8} | " * ncol).format(*SYNS_COLUMNS[:ncol]))
    print(("&{: 8.3f}  " * ncol).format(*mean_errors.tolist()) + "\\\\")
    return mean_errors, ratios


# ---------------------------------------------------------------------------- KITTI odometry (evaluate_pose.py)
PoseATE = collections.namedtuple("PoseATE", "direct chained gt_local ates summary")
PoseATE.__doc__ = """Result of `pose_ate`, device tensors: `direct` float32 [N,4,4] (= poses[0]), `chained` float32 [N,4,4],
`gt_local` float64 [M-S,4,4], `ates` float64 [2,N-S] (row 0 direct, row 1 chained), `summary` float64 [2,4] (mean,
population std, count, 0 per row)."""


def read_poses_file(path):
    """A KITTI odometry poses file as float64 [M, 12] (evaluate_pose.py:125, before its reshape)."""
    return np.loadtxt(path, dtype=np.float64, ndmin=2).reshape(-1, 12)


def pose_ate(poses, gt_global, skip=2, track_length=1, backend=None):
    """evaluate_pose.py:101-116 and :125-162 after the pose network, in ONE `bbd_pose_ate` call (three small launches, no
    host synchronisation): `poses` float32 [1+S, N, 4, 4] (or [1+S, N, 16]) holds, for window i, the direct pose of frames
    (i, i+S) in section 0 and the single-step pose of frames (i+k, i+k+1) in section 1+k; `gt_global` [M, 12] (or
    [M, 3, 4]) float64 are the rows of the sequence's poses file.  Returns a `PoseATE`.  Track i of [0, N-S) scores
    min(track_length, N-i) poses like Python's slices; a track whose predicted translations are all zero is NaN (0/0)
    and makes the mean and std of its row NaN, as in numpy."""
    backend = backend or ops.default_backend()
    S, L = int(skip), int(track_length)
    if S < 1 or L < 1:
        raise ValueError("pose_ate: skip and track_length must be at least 1 (got %d, %d)" % (S, L))
    poses = poses.detach()
    if poses.dtype != torch.float32 or poses.dim() not in (3, 4) or poses.shape[0] != 1 + S \
            or tuple(poses.shape[2:]) not in ((16,), (4, 4)):
        raise ValueError("pose_ate: poses must be float32 [1 + skip = %d, N, 4, 4], got %s %s"
                         % (1 + S, poses.dtype, tuple(poses.shape)))
    dev = poses.device
    N = poses.shape[1]
    poses = poses.reshape(1 + S, N, 16).contiguous()
    gt = torch.as_tensor(gt_global, dtype=torch.float64).reshape(-1, 12)
    M = gt.shape[0]
    if N > M - S:
        raise ValueError("pose_ate: %d windows of skip %d need %d ground-truth poses, the sequence has %d (N = %d > "
                         "M - S = %d)" % (N, S, N + S, M, N, M - S))
    if gt.device != dev:
        gt = upload(gt, dev)
    gt = gt.contiguous()
    backend._check(poses, gt)
    tracks = max(N - S, 0)
    chained = torch.empty(N, 4, 4, dtype=torch.float32, device=dev)
    gt_local = torch.empty(M - S, 4, 4, dtype=torch.float64, device=dev)
    ates = torch.empty(2, tracks, dtype=torch.float64, device=dev)
    summary = torch.empty(2, 4, dtype=torch.float64, device=dev)
    pose_ate_into(poses, gt, chained, gt_local, ates, summary, S, L, backend)
    return PoseATE(poses[0].view(N, 4, 4), chained, gt_local, ates, summary)


def pose_ate_into(poses, gt, chained, gt_local, ates, summary, skip, track_length, backend=None):
    """The `bbd_pose_ate` call itself on caller-owned, contiguous tensors of one device (shapes as `pose_ate` builds
    them); every element of the four outputs is written, nothing else is."""
    backend = backend or ops.default_backend()
    N, M = poses.shape[1], gt.shape[0]
    assert chained.numel() == N * 16 and gt_local.numel() == (M - skip) * 16 and summary.numel() == 8
    assert ates.numel() == 2 * max(N - skip, 0)
    backend._check(poses, gt, chained, gt_local, ates, summary)
    backend.run("bbd_pose_ate", summary, ptr(poses), ptr(gt), ptr(chained), ptr(gt_local), ptr(ates), ptr(summary),
                N, M, int(skip), int(track_length))


KITTI_LENGTHS = (100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0)     # the devkit's sub-sequence lengths, metres
PoseTrajectory = collections.namedtuple("PoseTrajectory", "traj gt_traj aligned transform dist pairs per_length summary")
PoseTrajectory.__doc__ = """Result of `pose_trajectory`, float64 device tensors, F = J + 1 frames: `traj` [F,4,4] (camera to
first frame, chained from the steps), `gt_traj` [F,4,4] (inv(G_0) G_j), `aligned` [F,4,4], `transform` [4,4] (R | t),
`dist` [F] (ground-truth path length), `pairs` [ceil(F/step), n_len, 4] = (last or -1, t_err, r_err, 0), `per_length`
[n_len, 3] = (mean t_err, mean r_err, count), `summary` [8] = (t_rel, r_rel, pair count, ate_rmse, ate_mean, ate_max,
c, F).  t_err is per unit of length (x 100 = %), r_err in radians per unit of length."""


def _traj_lengths(lengths):
    import ctypes
    lengths = [float(x) for x in lengths]
    if not 1 <= len(lengths) <= TRAJ_MAX_LEN or not all(np.isfinite(x) and x > 0 for x in lengths) \
            or any(b <= a for a, b in zip(lengths, lengths[1:])):
        raise ValueError("pose_trajectory: lengths must be 1 to %d positive, strictly increasing numbers, got %r"
                         % (TRAJ_MAX_LEN, lengths))
    return (ctypes.c_double * len(lengths))(*lengths)


def pose_trajectory(steps, gt_global, align="sim3", lengths=KITTI_LENGTHS, step=10, backend=None):
    """The KITTI devkit's odometry scores of a whole sequence in ONE `bbd_pose_trajectory` call (four small launches, no
    host synchronisation): `steps` float32 [J,4,4] (or [J,16]) are the pose network's matrices of the
    frame pairs (j, j+1) - section 1 of `pose_ate`'s `poses` with skip 1 - and `gt_global` [M,12] (or [M,3,4]) float64
    the rows of the poses file, M >= J + 1.  The steps are chained into a trajectory, aligned to ground truth
    (`align`: "sim3" Umeyama, "se3" rigid, "scale" the reference's least-squares scale only, "none"), and scored: the ATE
    of the aligned trajectory and, for first frames 0, `step`, 2 `step`, .. and every length of `lengths`, the devkit's
    translational and rotational sub-sequence errors.  Returns a `PoseTrajectory`.  A prediction that never moves has no
    scale: c and everything that depends on it are NaN under "sim3" and "scale"."""
    backend = backend or ops.default_backend()
    if align not in TRAJ_MODES:
        raise ValueError("pose_trajectory: align must be one of %s, got %r" % (", ".join(TRAJ_MODES), align))
    step = int(step)
    if step < 1:
        raise ValueError("pose_trajectory: step must be at least 1 (got %d)" % step)
    clen = _traj_lengths(lengths)
    steps = steps.detach()
    if steps.dtype != torch.float32 or steps.dim() not in (2, 3) or tuple(steps.shape[1:]) not in ((16,), (4, 4)) \
            or steps.shape[0] < 1:
        raise ValueError("pose_trajectory: steps must be float32 [J >= 1, 4, 4], got %s %s"
                         % (steps.dtype, tuple(steps.shape)))
    dev = steps.device
    J = steps.shape[0]
    F = J + 1
    steps = steps.reshape(J, 16).contiguous()
    gt = torch.as_tensor(gt_global, dtype=torch.float64).reshape(-1, 12)
    M = gt.shape[0]
    if M < F:
        raise ValueError("pose_trajectory: %d steps span %d frames, the ground truth has %d poses (M = %d < J + 1 = %d)"
                         % (J, F, M, M, F))
    if gt.device != dev:
        gt = upload(gt, dev)
    gt = gt.contiguous()
    backend._check(steps, gt)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)   # noqa: E731
    res = PoseTrajectory(new(F, 4, 4), new(F, 4, 4), new(F, 4, 4), new(4, 4), new(F), new(-(-F // step), len(clen), 4),
                         new(len(clen), 3), new(8))
    pose_trajectory_into(steps, gt, clen, res, step, align, backend)
    return res


def pose_trajectory_into(steps, gt, lengths, out, step, align, backend=None):
    """The `bbd_pose_trajectory` call itself on caller-owned, contiguous tensors of one device: `out` is a
    `PoseTrajectory` (or any sequence of its eight tensors, shapes as `pose_trajectory` builds them), `lengths` a
    sequence of numbers or a ctypes double array; every element of the eight outputs is written, nothing else is."""
    import ctypes
    backend = backend or ops.default_backend()
    if not isinstance(lengths, ctypes.Array):
        lengths = _traj_lengths(lengths)
    J, M, F, n_len = steps.shape[0], gt.shape[0], steps.shape[0] + 1, len(lengths)
    traj, gt_traj, aligned, transform, dist, pairs, per_length, summary = out
    assert steps.dtype == torch.float32 and steps.numel() == J * 16 and gt.dtype == torch.float64 and gt.numel() == M * 12
    assert all(t.dtype == torch.float64 for t in out)
    assert traj.numel() == F * 16 and gt_traj.numel() == F * 16 and aligned.numel() == F * 16 and transform.numel() == 16
    assert dist.numel() == F and pairs.numel() == -(-F // int(step)) * n_len * 4 and per_length.numel() == n_len * 3
    assert summary.numel() == 8
    backend._check(steps, gt, *out)
    backend.run("bbd_pose_trajectory", summary, ptr(steps), ptr(gt), ctypes.cast(lengths, ctypes.c_void_p), ptr(traj),
                ptr(gt_traj), ptr(aligned), ptr(transform), ptr(dist), ptr(pairs), ptr(per_length), ptr(summary), J, M,
                n_len, int(step), TRAJ_MODES[align])


def odom_sequence(eval_split):
    """`odom_<n>` -> n (evaluate_pose.py:50-53; every sequence with ground truth, 0-10, is accepted)."""
    parts = str(eval_split).split("_")
    if len(parts) != 2 or parts[0] != "odom" or not parts[1].isdigit() or not 0 <= int(parts[1]) <= 10:
        raise ValueError("eval_split should be odom_0 ... odom_10, got %r" % (eval_split,))
    return int(parts[1])


def odom_paths(opt):
    """(sequence, split file, odometry root, poses file) of `opt` (evaluate_pose.py:53-57, :124, kitti_dataset.py:71)."""
    import os
    seq = odom_sequence(opt.eval_split)
    root = getattr(opt, "odom_path", None)
    if root is None:
        root = os.path.join(os.path.dirname(opt.kt_path), "odom")
    return (seq, os.path.join(getattr(opt, "splits_dir", "splits"), "odom", "test_files_{:02d}.txt".format(seq)), root,
            os.path.join(root, "poses", "{:02d}.txt".format(seq)))


def evaluate_pose(opt, dataloader=None, gt_poses=None, models=None, batch_windows=64, backend=None, device=None):
    """The reference's `evaluate_pose.py`: the pose network's direct `skip_frame`-step pose and the pose chained from its
    single steps, scored against KITTI odometry ground truth (absolute trajectory error over `track_length`-pose tracks).
    Prints the reference's two `Trajectory error` lines, direct first, and returns a dict: `ate_mean`, `ate_std`,
    `ate_chained_mean`, `ate_chained_std`, `ates` (numpy [2, N-S]), `pred_poses`, `pred_poses_chained` (numpy [N,4,4]).

    Every frame is decoded and resized once into a pool [F,3,H,W] by the device loader; per chunk of `batch_windows`
    windows the 1+S pair sections are gathered (`ops.gather_pairs`) and go through the pose network as ONE batch, the
    matrices (`ops.pose_matrix`) land in a persistent [1+S, N, 16] buffer, and after the last chunk one `pose_ate` call
    scores all windows; the finished table is read back once.  (The reference decodes 8 frames per window, runs the
    network three times at batch 1, copies every pose to the host and scores in a Python loop.)

    `dataloader` / `gt_poses` / `models` may be injected.  The dataloader must yield the frames `windows(skip)` of the
    split's `KITTIOdomDataset` names, in that order, as `("color", 0, 0)`; by default the split is
    `opt.splits_dir/odom/test_files_<nn>.txt`, frames and `poses/<nn>.txt` come from `opt.odom_path` (default
    `dirname(opt.kt_path)/odom`) and weights from `pose_encoder.pth` / `pose.pth` in `opt.load_weights_folder`.
    Departures from the reference, both deliberate: only TRAILING windows without frames are dropped (a frame missing
    in the middle raises), and the input size is `opt.height x opt.width` (the reference fixes 192 x 640, the defaults).

    `opt.trajectory` adds the scores every KITTI odometry table reports (`pose_trajectory`), with no
    further network pass: the N + S - 1 single steps of the sequence are taken from the pose buffer - `poses[1][j]` for
    j < N, then `poses[1 + k][N - 1]` for k = 1 .. S - 1 - chained, aligned by `opt.trajectory_align` and scored; the
    results travel in the same read-back.  One more line is printed after the reference's two (alignment, frames, t_rel
    in %, r_rel in deg / 100 m, the ATE rmse in metres, the scale) and the dict gains `t_rel` (a fraction), `r_rel`
    (rad / m), `traj_ate_rmse`, `traj_scale`, `per_length` ([8, 3]: mean t_err, mean r_err, count for 100 .. 800 m),
    `traj_aligned` and `traj_gt` ([F,4,4]).  `opt.save_trajectory` writes the aligned poses as a KITTI poses file.

    `opt.save_map` (needs `opt.trajectory`) writes the scene map of the sequence as a binary PLY file (`_scene_map`,
    DESIGN.md 6j): the depth network (`encoder.pth` / `depth.pth` of the same folder, `opt.ViT` honoured, or `models[2:4]`)
    runs over every `opt.map_every`-th frame of the pool, and each batch goes into a `pointcloud.SceneMap` with its rows
    of the aligned trajectory and the alignment's scale, both still on the device.  One more line is printed and the dict
    gains `map_stats` (frames, candidates, kept, dropped_range, dropped_full, voxels) and `map_path`.

    `opt.save_plot` (needs `opt.trajectory`) writes a picture of the run (`_trajectory_plot`): the ground
    truth and the aligned prediction seen from above (`opt.plot_view`: or from the side), over the map's voxels where
    `opt.save_map` is given, with a disc at the start and a scale bar.  It is drawn on the device from what is already
    there and read back once.  One more line is printed and the dict gains `plot_stats` (view, m_per_px, scale_bar and
    the voxels offered, drawn, clipped, rejected) and `plot_path`.

    `opt.consistency` (needs `opt.trajectory`) scores whether the depth network and the pose network agree, without
    ground truth (`_consistency`): the disparities of every `opt.map_every`-th frame are predicted once, each
    frame's pixels are moved into its `opt.consistency_views` neighbours on either side with the aligned trajectory and
    compared with the depth predicted there, err = |z - d_b| / (z + d_b).  One more line is printed after the trajectory
    line and the dict gains `consistency` (views, threshold, min_views, frames, mean_err, agree_share, kept_share and the
    five totals valid, visible, consistent, err_sum, kept), from one read-back of the counters.  `opt.map_consistent`
    (needs `opt.save_map`) implies it and fuses the map from the filtered disparities - pixels that agree in fewer than
    `opt.consistency_min_views` neighbours are offered as disparity 0, which the map rejects like any other disparity
    without a finite depth: `map_stats["kept"]` falls by their number, no other statistic moves.
    `backend` / `device` are the seam of the test tier (default: the HIP backend on `cuda:<opt.cuda>`)."""
    import os
    from . import datasets, networks, tuning
    tuning.use_shipped_db()
    seq, split_file, odom_root, poses_file = odom_paths(opt)
    S, L = int(getattr(opt, "skip_frame", 2)), int(getattr(opt, "track_length", 1))
    device = torch.device(device if device is not None else "cuda:%d" % getattr(opt, "cuda", 0))
    height, width = opt.height, opt.width
    trajectory, save_trajectory = bool(getattr(opt, "trajectory", False)), getattr(opt, "save_trajectory", None)
    align = getattr(opt, "trajectory_align", "sim3")
    if save_trajectory and not trajectory:
        raise ValueError("evaluate_pose: --save_trajectory needs --trajectory")
    save_map = getattr(opt, "save_map", None)
    if save_map and not trajectory:
        raise ValueError("evaluate_pose: --save_map needs --trajectory")
    map_consistent = bool(getattr(opt, "map_consistent", False))
    if map_consistent and not save_map:
        raise ValueError("evaluate_pose: --map_consistent needs --save_map")
    consistency = bool(getattr(opt, "consistency", False)) or map_consistent
    if consistency and not trajectory:
        raise ValueError("evaluate_pose: --consistency needs --trajectory")
    map_opt = _map_options(opt) if save_map or consistency else None
    consist_opt = _consistency_options(opt) if consistency else None
    save_plot = getattr(opt, "save_plot", None)
    if save_plot and not trajectory:
        raise ValueError("evaluate_pose: --save_plot needs --trajectory")
    plot_opt = _plot_options(opt) if save_plot else None
    if trajectory and align not in TRAJ_MODES:
        raise ValueError("evaluate_pose: --trajectory_align must be one of %s, got %r" % (", ".join(TRAJ_MODES), align))
    # ---- host: the window tables and the ground truth, checked before anything is launched
    lines = datasets.KITTIOdomDataset(datasets.readlines(split_file), 0, height, width, kt_path=opt.kt_path, is_train=False,
                                      kt=True, naive_mix=True, odom_path=odom_root)
    frames, pairs, N = lines.windows(S)
    if gt_poses is None:
        gt_poses = read_poses_file(poses_file)
    gt_poses = torch.as_tensor(gt_poses, dtype=torch.float64).reshape(-1, 12)
    M = gt_poses.shape[0]
    if N > M - S:
        raise ValueError("evaluate_pose: the split has N = %d windows of skip %d but the ground truth has %d poses "
                         "(M - S = %d)" % (N, S, M, M - S))
    if models is None:
        folder = os.path.expanduser(opt.load_weights_folder)
        assert os.path.isdir(folder), "Cannot find a folder at {}".format(folder)
        encoder = networks.ResnetEncoder(opt.num_layers, False, 2)
        encoder.load_state_dict(torch.load(os.path.join(folder, "pose_encoder.pth"), map_location=device))
        decoder = networks.PoseDecoder(encoder.num_ch_enc, 1, 2)
        decoder.load_state_dict(torch.load(os.path.join(folder, "pose.pth"), map_location=device))
    else:
        encoder, decoder = models[:2]
    encoder.to(device).eval()
    decoder.to(device).eval()
    predictor = _map_predictor(opt, models, height, width, device, backend) if save_map or consistency else None
    if dataloader is None:
        pool_set = datasets.KITTIOdomDataset(frames, 0, height, width, kt_path=opt.kt_path, is_train=False, kt=True,
                                             naive_mix=True, odom_path=odom_root)
        dataloader = datasets.DeviceLoader(pool_set, 32, datasets.DeviceCollate(height, width, [0], device), shuffle=False,
                                           drop_last=False, num_workers=getattr(opt, "num_workers", 8))
    print("-> Computing pose predictions")
    F = len(frames)
    pool = torch.empty(F, 3, height, width, device=device)
    first = 0
    for data in dataloader:                              # each frame resized once, straight into the pool
        color = data[("color", 0, 0)]
        assert first + color.shape[0] <= F, "the dataloader yields more than the %d frames of the windows" % F
        pool[first:first + color.shape[0]].copy_(color)
        first += color.shape[0]
    assert first == F, "the windows need %d frames, the dataloader gave %d" % (F, first)
    # [2, 1+S, N]: first and second frame of every pair, each plane contiguous
    table = upload(pairs.transpose(2, 0, 1), device)
    poses = torch.empty(1 + S, N, 16, device=device)
    with torch.no_grad():
        for lo in range(0, N, max(1, int(batch_windows))):
            chunk = table[:, :, lo:lo + batch_windows]
            n = chunk.shape[2]
            x = ops.gather_pairs(pool, chunk[0].reshape(-1), chunk[1].reshape(-1), backend=backend)  # [(1+S) n, 6, H, W]
            axisangle, translation = decoder([encoder(x)])
            mats = ops.pose_matrix(axisangle[:, 0], translation[:, 0], backend=backend)
            poses[:, lo:lo + n] = mats.view(1 + S, n, 16)
        if trajectory:
            gt_poses = upload(gt_poses, device)          # one upload for both calls
        res = pose_ate(poses, gt_poses, skip=S, track_length=L, backend=backend)
        parts = [res.summary.reshape(-1), res.ates.reshape(-1), res.direct.reshape(-1).double(),
                 res.chained.reshape(-1).double()]                           # float32 -> float64 and back is exact
        if trajectory:
            if N < 1:
                raise ValueError("evaluate_pose: --trajectory needs at least one window")
            # frame pair (j, j+1): window j's first step, and past the last window its later steps
            steps = torch.cat([poses[1], poses[2:, N - 1]]) if S > 1 else poses[1]
            tr = pose_trajectory(steps, gt_poses, align=align, backend=backend)
            parts += [tr.summary, tr.per_length.reshape(-1), tr.aligned.reshape(-1), tr.gt_traj.reshape(-1)]
        packed = torch.cat(parts)
    host = packed.cpu().numpy()                          # the only host synchronisation: the finished tables
    tracks = res.ates.shape[1]
    summary, ates = host[:8].reshape(2, 4), host[8:8 + 2 * tracks].reshape(2, tracks)
    mats = host[8 + 2 * tracks:8 + 2 * tracks + 32 * N].astype(np.float32).reshape(2, N, 4, 4)
    out = {"ate_mean": float(summary[0, 0]), "ate_std": float(summary[0, 1]), "ate_chained_mean": float(summary[1, 0]),
           "ate_chained_std": float(summary[1, 1]), "ates": ates, "pred_poses": mats[0], "pred_poses_chained": mats[1]}
    print("\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(out["ate_mean"], out["ate_std"]))
    print("\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(out["ate_chained_mean"], out["ate_chained_std"]))
    if trajectory:
        rest = host[8 + 2 * tracks + 32 * N:]
        n_len, frames_scored = len(KITTI_LENGTHS), N + S
        tsum, per_length = rest[:8], rest[8:8 + 3 * n_len].reshape(n_len, 3)
        both = rest[8 + 3 * n_len:].reshape(2, frames_scored, 4, 4)
        out.update({"t_rel": float(tsum[0]), "r_rel": float(tsum[1]), "traj_ate_rmse": float(tsum[3]),
                    "traj_scale": float(tsum[6]), "per_length": per_length, "traj_aligned": both[0], "traj_gt": both[1]})
        print("   Full trajectory ({}, {:d} frames): t_rel {:0.3f} %, r_rel {:0.3f} deg/100m, ATE {:0.3f} m, scale {:0.4f}\n"
              .format(align, frames_scored, 100.0 * out["t_rel"], 100.0 * np.degrees(out["r_rel"]), out["traj_ate_rmse"],
                      out["traj_scale"]))
        if save_trajectory:
            np.savetxt(save_trajectory, both[0].reshape(frames_scored, 16)[:, :12], fmt="%.6e")
        if (save_map or consistency) and F != frames_scored:
            raise ValueError("evaluate_pose: %s needs the frames of one side of one sequence: the pool holds %d frames, "
                             "the trajectory %d" % ("--save_map" if save_map else "--consistency", F, frames_scored))
        filtered = None
        if consistency:
            out["consistency"], filtered = _consistency(predictor, pool, tr, map_opt["every"], consist_opt, map_consistent,
                                                        backend)
            print("   Depth-pose consistency (views {views:d}, threshold {threshold:g}, {frames:d} frames): mean err "
                  "{mean_err:0.4f}, {:0.2f} % of visible samples agree, {:0.2f} % of valid pixels kept\n"
                  .format(100.0 * out["consistency"]["agree_share"], 100.0 * out["consistency"]["kept_share"],
                          **out["consistency"]))
        if save_map:
            out["map_stats"], scene = _scene_map(predictor, pool, tr, map_opt, save_map, backend, disps=filtered)
            out["map_path"] = save_map
            print("   Scene map: {frames:d} frames, {candidates:d} candidates, {kept:d} kept, {voxels:d} voxels -> {}\n"
                  .format(save_map, **out["map_stats"]))
        if save_plot:
            out["plot_stats"] = _trajectory_plot(tr, both, scene if save_map else None, map_opt, plot_opt, save_plot,
                                                 device, backend)
            out["plot_path"] = save_plot
            print("   Plot: {view}, {m_per_px:.4g} m/px, scale bar {scale_bar:g} m, {drawn:d} of {offered:d} voxels -> {}\n"
                  .format(save_plot, **out["plot_stats"]))
    return out


def _map_options(opt):
    """The --map_* options of `opt` with their defaults, checked."""
    m = {"voxel": float(getattr(opt, "map_voxel", 0.2)), "every": int(getattr(opt, "map_every", 1)),
         "stride": int(getattr(opt, "map_stride", 2)), "min_depth": float(getattr(opt, "map_min_depth", 0.5)),
         "max_depth": float(getattr(opt, "map_max_depth", 30.0)), "min_points": int(getattr(opt, "map_min_points", 1)),
         "capacity": int(getattr(opt, "map_capacity", 1 << 24))}
    if not (m["voxel"] > 0.0 and np.isfinite(m["voxel"])):
        raise ValueError("evaluate_pose: --map_voxel must be positive, got %r" % m["voxel"])
    if min(m["every"], m["stride"], m["min_points"], m["capacity"]) < 1:
        raise ValueError("evaluate_pose: --map_every, --map_stride, --map_min_points and --map_capacity must be at least 1")
    if not m["min_depth"] <= m["max_depth"]:
        raise ValueError("evaluate_pose: --map_min_depth %r exceeds --map_max_depth %r" % (m["min_depth"], m["max_depth"]))
    return m


def _map_predictor(opt, models, height, width, device, backend):
    """The depth network of --save_map: `models[2:4]` where a depth pair was injected, else the weights folder's."""
    import os
    from .inference import DepthPredictor
    kw = dict(min_depth=getattr(opt, "min_depth", 0.1), max_depth=getattr(opt, "max_depth", 100.0), backend=backend)
    if models is not None and len(models) >= 4:
        return DepthPredictor(models[2], models[3], height, width, device, **kw)
    folder = os.path.expanduser(opt.load_weights_folder)
    predictor = DepthPredictor.from_weights(folder, vit=bool(getattr(opt, "ViT", False)),
                                            num_layers=getattr(opt, "num_layers", 18), device=device, **kw)
    if (predictor.feed_height, predictor.feed_width) != (height, width):
        raise ValueError("evaluate_pose: --save_map feeds the depth network the frames of the pose evaluation, %d x %d, "
                         "but %s was trained at %d x %d; pass --height %d --width %d"
                         % (height, width, folder, predictor.feed_height, predictor.feed_width, predictor.feed_height,
                            predictor.feed_width))
    return predictor


def _scene_map(predictor, pool, tr, m, path, backend=None, disps=None):
    """The scene map of a sequence: every `every`-th frame of `pool` [F,3,H,W] through the depth network in batches, each
    batch straight into `SceneMap.add` with its rows of `tr.aligned` and the scale `tr.summary[6:7]` (1 under se3 / none)
    - nothing is read back before `finish`.  `disps` ([R,H,W], one row per selected frame: `_consistency`'s filtered
    disparities) takes the place of the network pass.  Writes `path`; returns the statistics and the map."""
    from . import pointcloud
    F, _, H, W = pool.shape
    scene = pointcloud.SceneMap(m["voxel"], m["capacity"], pool.device, backend)
    inv_K = upload(pointcloud.intrinsics(H, W), pool.device)
    min_disp, max_disp = 1.0 / predictor.max_depth, 1.0 / predictor.min_depth
    rows = list(range(0, F, m["every"]))
    with torch.no_grad():
        for lo in range(0, len(rows), predictor.batch_size):
            sel = slice(rows[lo], rows[min(lo + predictor.batch_size, len(rows)) - 1] + 1, m["every"])
            rgb = pool[sel].contiguous()
            if disps is None:
                disp = min_disp + (max_disp - min_disp) * predictor.disparity(rgb)
            else:
                disp = disps[lo:lo + predictor.batch_size]
            scene.add(disp, rgb, tr.aligned[sel].contiguous(), inv_K, scale=tr.summary[6:7], stride=m["stride"],
                      min_depth=m["min_depth"], max_depth=m["max_depth"])
        vertices, _, stats = scene.finish(m["min_points"])
    pointcloud.write_ply(path, vertices)
    stats["frames"] = len(rows)
    return stats, scene


CONSISTENCY_CHUNK = 64           # frames per `ops.depth_consistency` call of `_consistency`, neighbours not counted


def _consistency_options(opt):
    """The --consistency_* options of `opt` with their defaults, checked."""
    from ._lib import CONSIST_MAX_VIEWS
    c = {"views": int(getattr(opt, "consistency_views", 1)), "threshold": float(getattr(opt, "consistency_threshold", 0.05)),
         "min_views": int(getattr(opt, "consistency_min_views", 1))}
    if not 1 <= 2 * c["views"] <= CONSIST_MAX_VIEWS:
        raise ValueError("evaluate_pose: --consistency_views must lie in [1, %d], got %d" % (CONSIST_MAX_VIEWS // 2, c["views"]))
    if not c["threshold"] >= 0.0:
        raise ValueError("evaluate_pose: --consistency_threshold must not be negative, got %r" % c["threshold"])
    if c["min_views"] < 0:
        raise ValueError("evaluate_pose: --consistency_min_views must not be negative, got %d" % c["min_views"])
    return c


def consistency_offsets(views):
    """The neighbours of --consistency_views k: -1, 1, -2, 2, ... -k, k."""
    return tuple(o for k in range(1, int(views) + 1) for o in (-k, k))


def _consistency(predictor, pool, tr, every, c, want_filtered, backend=None):
    """Depth-pose consistency of a sequence: every `every`-th frame of `pool` [F,3,H,W] through the depth network once,
    into one [R,H,W] buffer of scaled disparities; then `ops.depth_consistency` over it in chunks of CONSISTENCY_CHUNK frames, each
    with the `views` neighbours it needs on either side (they ride along without sources of their own, and what the call
    writes for them is dropped), with the rows of `tr.aligned` and the scale `tr.summary[6:7]`.  The per-frame counters
    are summed on the device and read back once.  Returns (the `consistency` dict, the filtered disparities [R,H,W] on
    the device or None)."""
    from . import pointcloud
    F, _, H, W = pool.shape
    dev = pool.device
    K = upload(np.ascontiguousarray(pointcloud.camera_matrix(H, W)[:3, :3]), dev)
    inv_K = upload(pointcloud.intrinsics(H, W), dev)
    min_disp, max_disp = 1.0 / predictor.max_depth, 1.0 / predictor.min_depth
    rows = list(range(0, F, every))
    R, k = len(rows), c["views"]
    chunk = int(CONSISTENCY_CHUNK)
    disps = torch.empty(R, H, W, dtype=torch.float32, device=dev)
    filtered = torch.empty(R, H, W, dtype=torch.float32, device=dev) if want_filtered else None
    poses = tr.aligned[::every].contiguous()
    table = pointcloud.neighbour_sources(R, consistency_offsets(k))
    totals = torch.zeros(5, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for lo in range(0, R, predictor.batch_size):
            sel = slice(rows[lo], rows[min(lo + predictor.batch_size, R) - 1] + 1, every)
            disp = min_disp + (max_disp - min_disp) * predictor.disparity(pool[sel].contiguous())
            disps[lo:lo + disp.shape[0]] = disp[:, 0] if disp.dim() == 4 else disp
        for lo in range(0, R, chunk):
            hi = min(lo + chunk, R)
            a, b = max(lo - k, 0), min(hi + k, R)             # the chunk with its neighbours
            local = table[a:b].copy()
            local[local >= 0] -= a
            local[:lo - a] = -1                                # the neighbours are sources only
            local[hi - a:] = -1
            res = ops.depth_consistency(disps[a:b], poses[a:b], K, inv_K, local, scale=tr.summary[6:7],
                                        threshold=c["threshold"], min_views=c["min_views"], want_filtered=want_filtered,
                                        backend=backend)
            totals += res.counters[lo - a:hi - a].sum(0)
            if want_filtered:
                filtered[lo:hi] = res.filtered[lo - a:hi - a]
    valid, visible, consistent, err_sum, kept = (int(v) for v in totals.cpu().tolist())      # the one read-back
    share = lambda part, whole: part / whole if whole else float("nan")                      # noqa: E731
    out = dict(c, frames=R, valid=valid, visible=visible, consistent=consistent, err_sum=err_sum, kept=kept,
               mean_err=share(err_sum / 16777216.0, visible), agree_share=share(consistent, visible),
               kept_share=share(kept, valid))
    return out, filtered


PLOT_GT, PLOT_PRED, PLOT_START, PLOT_BAR = (40, 40, 40), (214, 39, 40), (31, 119, 180), (0, 0, 0)


def _plot_options(opt):
    """The --plot_* options of `opt` with their defaults, checked."""
    p = {"view": getattr(opt, "plot_view", "top"), "size": int(getattr(opt, "plot_size", 1024)),
         "ceiling": float(getattr(opt, "plot_ceiling", 3.0)), "point_size": int(getattr(opt, "plot_point_size", 1))}
    if p["view"] not in ("top", "side"):
        raise ValueError("evaluate_pose: --plot_view is top or side, got %r" % (p["view"],))
    if not 16 <= p["size"] <= 16384:
        raise ValueError("evaluate_pose: --plot_size must lie in [16, 16384], got %d" % p["size"])
    if p["point_size"] not in (1, 3, 5, 7):
        raise ValueError("evaluate_pose: --plot_point_size is 1, 3, 5 or 7, got %d" % p["point_size"])
    if not (p["ceiling"] > 0.0 and np.isfinite(p["ceiling"])):     # the cameras themselves must stay below the near plane
        raise ValueError("evaluate_pose: --plot_ceiling must be positive and finite, got %r" % p["ceiling"])
    return p


def scale_bar_length(metres):
    """The largest of 1, 2, 5 x 10^k that is <= `metres` (> 0)."""
    k = int(np.floor(np.log10(metres)))
    best = None
    for e in (k - 1, k, k + 1):
        for m in (1.0, 2.0, 5.0):
            c = m * 10.0 ** e
            if c <= metres and (best is None or c > best):
                best = c
    return best


def plot_layout(both, p):
    """What `--save_plot` draws besides the two trajectories, from the host copy `both` [2,F,4,4] (aligned prediction,
    ground truth): the view and its metres per pixel, the scale bar's length and its two world positions."""
    from . import pointcloud
    pos = np.ascontiguousarray(both[:, :, :3, 3], dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(pos).all():
        raise ValueError("evaluate_pose: --save_plot needs finite trajectories (a prediction that never moves has no sim3 "
                         "scale; --trajectory_align se3 needs none)")
    lo, hi = pos.min(0), pos.max(0)
    size = p["size"]
    # top: y points down, so the highest camera has the smallest y; what lies more than the ceiling above it is clipped
    near = lo[1] - p["ceiling"] if p["view"] == "top" else None
    view, mpp = pointcloud.ortho_view(lo, hi, size, size, plane=p["view"], near=near)
    bar = scale_bar_length(0.25 * size * mpp)
    # the bar: lower left, 4 % of the picture in from both edges, through pixel centres (an edge of the bar then runs
    # between two rows of centres, not through one), at the first camera's place on the depth axis
    px0, py = np.floor(0.04 * size) + 0.5, np.floor(0.96 * size) + 0.5
    a, b, c = (0, 2, 1) if p["view"] == "top" else (2, 1, 0)
    ends = np.zeros((2, 3), np.float64)
    for k, px in enumerate((px0, px0 + bar / mpp)):
        ends[k, a] = (px - view[0, 3]) / view[0, a]
        ends[k, b] = (py - view[1, 3]) / view[1, b]
        ends[k, c] = pos[0, c]
    return view, mpp, bar, ends


def _trajectory_plot(tr, both, scene, m, p, path, device, backend=None):
    """The picture of `--save_plot`.  The view comes from the host copy of the trajectories that the
    evaluation's read-back delivered; everything drawn is still on the device: the map's voxels underneath
    (`SceneMap.render`), then, each above the one before, the ground truth (layer 1), the aligned prediction (layer 2),
    the start disc and the scale bar (layer 3).  One read-back: the finished picture with the counters."""
    from . import pointcloud
    view, mpp, bar, ends = plot_layout(both, p)
    canvas = pointcloud.Canvas(p["size"], p["size"], device, backend)
    view_dev = upload(view, device)
    F = tr.aligned.numel() // 16
    with torch.no_grad():
        if scene is not None:
            scene.render(canvas, view_dev, min_points=m["min_points"], size=p["point_size"])
        gt_xyz = tr.gt_traj.reshape(F, 16)[:, 3::4][:, :3].contiguous()
        pred_xyz = tr.aligned.reshape(F, 16)[:, 3::4][:, :3].contiguous()
        canvas.lines(gt_xyz, view=view_dev, colour=PLOT_GT, width=3.0, layer=1)
        canvas.lines(pred_xyz, view=view_dev, colour=PLOT_PRED, width=2.0, layer=2)
        canvas.lines(gt_xyz[:1], view=view_dev, colour=PLOT_START, width=9.0, layer=3)
        canvas.lines(ends, view=view_dev, colour=PLOT_BAR, width=3.0, layer=3)
        stats = canvas.save(path)
    stats.update(view=p["view"], m_per_px=mpp, scale_bar=bar)
    return stats
