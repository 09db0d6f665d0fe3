#!/usr/bin/env python3
"""Golden vectors for the checkpoint comparison sheets, from the reference's own lines (validation.py) executed with
torch CPU, numpy and matplotlib:

  disparity pictures     validation.py:205-214  F.interpolate of the network output to the original size, Normalize(min,
                         max), ScalarMappable('magma')
  ground-truth pictures  validation.py:250-254  1 / gt, values above 80 zeroed, Normalize(min, max), magma
  per-frame abs_rel      validation.py:232-269  the live reference's `layers.disp_to_depth` and `validation.compute_errors`
                         (both imported unmodified through tools/refshim.py); cv2 is not installed here, so
                         `cv2.resize` is `oracle.eval_ref.cv2_resize_linear_ref`, as for tests/golden/eval_cases.npz

Output: tests/golden/compare_cases.npz (arrays only).  No NaNs in the fixtures: matplotlib draws them in its "bad"
colour, `bbd_viz_lut_index` gives them entry 0 on purpose.

    python tools/make_golden_compare.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import refshim  # noqa: E402
from oracle.eval_ref import cv2_resize_linear_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "compare_cases.npz")
torch.set_num_threads(1)

# (name, network h, w, original H0, W0, kind).  ATen blends in one of two orders, chosen by H0 + W0 <= 128.
DISP_CASES = [("up_small", 24, 40, 48, 76, "smooth"), ("up_big", 48, 160, 80, 250, "smooth"),
              ("same", 32, 64, 32, 64, "smooth"), ("down", 64, 208, 40, 130, "smooth"),
              ("constant", 16, 32, 40, 70, "constant")]
# (name, GH, GW, kind)
GT_CASES = [("sparse_31", 20, 31, "sparse"), ("zero_32", 8, 32, "zero"), ("cut", 12, 40, "cut"), ("dense_31", 9, 31, "dense"),
            ("sparse_32", 16, 32, "sparse")]
# (name, network h, w, GH, GW)
FRAME_CASES = [("frame_a", 24, 80, 47, 150), ("frame_b", 24, 80, 48, 152)]


def synth_disp(gen, h, w, kind):
    if kind == "constant":
        return torch.zeros(1, 1, h, w)
    low = torch.rand(1, 1, h // 8 + 1, w // 8 + 1, generator=gen)
    disp = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=True)
    return (disp + 0.02 * torch.rand(1, 1, h, w, generator=gen)).clamp(0.001, 0.999).float().contiguous()


def synth_gt(gen, gh, gw, kind):
    depth = (2.0 + 70.0 * torch.rand(gh, gw, generator=gen)).float()
    if kind == "zero":
        return np.zeros((gh, gw), np.float32)
    if kind == "dense":
        return depth.numpy()
    keep = torch.rand(gh, gw, generator=gen) < 0.1
    gt = torch.where(keep, depth, torch.zeros(())).numpy().astype(np.float32)
    if kind == "cut":
        gt[3, 5] = 0.01           # 1 / 0.01 = 100 > 80: zeroed
        gt[7, 20] = 0.004
        gt[2, 2] = 1.0 / 64.0     # 64 < 80: stays, and is the maximum
    return gt


def import_validation():
    """The reference's validation.py as a module: its imports this image lacks are answered with empty stubs."""
    refshim.install_stubs()
    if not hasattr(sys.modules["cv2"], "setNumThreads"):
        sys.modules["cv2"].setNumThreads = lambda n: None          # validation.py:28 calls it at import
    for name in ("tqdm",):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    tv = sys.modules.get("torchvision")
    if tv is not None and not hasattr(tv, "datasets"):
        tv.datasets = types.ModuleType("torchvision.datasets")
        sys.modules["torchvision.datasets"] = tv.datasets
    refshim.import_reference()
    import validation
    return validation


def main():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib as mpl
    import matplotlib.cm as cm
    _, ref_layers, _ = refshim.import_reference()
    validation = import_validation()
    out = {}
    gen = torch.Generator().manual_seed(4711)

    for name, h, w, H0, W0, kind in DISP_CASES:                        # validation.py:205-214
        disp = synth_disp(gen, h, w, kind)
        disp_resized = torch.nn.functional.interpolate(disp, (H0, W0), mode="bilinear", align_corners=False)
        disp_resized_np = disp_resized.squeeze().cpu().numpy()
        normalizer = mpl.colors.Normalize(vmin=disp_resized_np.min(), vmax=disp_resized_np.max())
        mapper = cm.ScalarMappable(norm=normalizer, cmap="magma")
        colormapped_im = (mapper.to_rgba(disp_resized_np)[:, :, :3] * 255).astype(np.uint8)
        out["disp/%s/disp" % name] = disp.numpy()
        out["disp/%s/size" % name] = np.array([H0, W0], np.int32)
        out["disp/%s/vmin" % name] = np.float32(disp_resized_np.min())
        out["disp/%s/vmax" % name] = np.float32(disp_resized_np.max())
        out["disp/%s/colour" % name] = colormapped_im
        print("disp", name, disp_resized_np.shape, float(disp_resized_np.min()), float(disp_resized_np.max()))

    for name, gh, gw, kind in GT_CASES:                                 # validation.py:250-254
        gt_depth = synth_gt(gen, gh, gw, kind)
        with np.errstate(divide="ignore"):
            gt_depth_play = 1 / gt_depth
        gt_depth_play[gt_depth_play > 80] = 0
        normalizer = mpl.colors.Normalize(vmin=gt_depth_play.min(), vmax=gt_depth_play.max())
        mapper = cm.ScalarMappable(norm=normalizer, cmap="magma")
        colormapped_im = (mapper.to_rgba(gt_depth_play)[:, :, :3] * 255).astype(np.uint8)
        assert gt_depth_play.dtype == np.float32 and not np.isnan(gt_depth_play).any()
        out["gt/%s/gt" % name] = gt_depth
        out["gt/%s/vmin" % name] = np.float32(gt_depth_play.min())
        out["gt/%s/vmax" % name] = np.float32(gt_depth_play.max())
        out["gt/%s/colour" % name] = colormapped_im
        print("gt", name, gt_depth.shape, float(gt_depth_play.min()), float(gt_depth_play.max()),
              "non-zero %.2f" % float((gt_depth != 0).mean()))

    MIN_DEPTH, MAX_DEPTH = 0.1, 80
    for name, h, w, gh, gw in FRAME_CASES:                              # validation.py:197-199, :232-269
        disp = synth_disp(gen, h, w, "smooth")
        pred_disp, _ = ref_layers.disp_to_depth(disp, MIN_DEPTH, MAX_DEPTH)
        pred_disp = pred_disp.cpu()[:, 0].numpy()[0]
        dense = 1.0 / cv2_resize_linear_ref(pred_disp, gw, gh)
        noise = 1.0 + 0.2 * torch.randn(gh, gw, generator=gen).numpy().astype(np.float32)
        keep = torch.rand(gh, gw, generator=gen).numpy() < 0.2
        gt_depth = np.where(keep, dense * np.float32(1.9) * noise, 0).astype(np.float32)
        gt_depth[0:2, :] = 90.0
        gt_height, gt_width = gt_depth.shape[:2]
        resized = cv2_resize_linear_ref(pred_disp, gt_width, gt_height)
        pred_depth = 1 / resized
        mask = np.logical_and(gt_depth > MIN_DEPTH, gt_depth < MAX_DEPTH)
        crop = np.array([0.40810811 * gt_height, 0.99189189 * gt_height,
                         0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)
        crop_mask = np.zeros(mask.shape)
        crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
        mask = np.logical_and(mask, crop_mask)
        pred_depth = pred_depth[mask]
        gt_sel = gt_depth[mask]
        ratio = np.median(gt_sel) / np.median(pred_depth)
        pred_depth *= ratio
        pred_depth[pred_depth < MIN_DEPTH] = MIN_DEPTH
        pred_depth[pred_depth > MAX_DEPTH] = MAX_DEPTH
        abs_rel = validation.compute_errors(gt_sel, pred_depth)
        out["frame/%s/disp" % name] = disp.numpy()
        out["frame/%s/pred_disp" % name] = pred_disp
        out["frame/%s/gt" % name] = gt_depth
        out["frame/%s/abs_rel" % name] = np.float64(abs_rel)
        out["frame/%s/ratio" % name] = np.float64(ratio)
        out["frame/%s/count" % name] = np.int64(mask.sum())
        print("frame", name, int(mask.sum()), float(abs_rel), float(ratio))

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KB")


if __name__ == "__main__":
    main()
