"""Numpy restatement of `bbd_error_map` (include/bbd_hip.h), built on the oracle's cv2-style resize and Garg mask
(oracle/eval_ref.py).  Every operation is float32, in the kernel's order, so the comparison is bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.eval_ref import cv2_resize_linear_ref, garg_mask  # noqa: E402

F = np.float32


def lut_index_ref(v, vmin, vmax):
    """bbd_viz_lut_index for an array (float32): Normalize, times 256, truncate; 256 and above -> 255, NaN -> 0."""
    v = np.asarray(v, F)
    vmin, vmax = F(vmin), F(vmax)
    if vmax == vmin:
        return np.zeros(v.shape, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        xi = ((v - vmin) / (vmax - vmin)) * F(256.0)
        idx = np.where(xi < F(256.0), np.maximum(np.nan_to_num(xi, nan=0.0).astype(np.int64), 0), 255)
    return np.where(np.isnan(xi), 0, idx)


def error_plane_ref(pred_disp, gt, ratio, count, min_depth=0.1, max_depth=80.0, scale_factor=1.0, median_scaling=True,
                    crop=True):
    """float32 [GH,GW]: the abs_rel summand at the pixels bbd_depth_metrics scores, NaN elsewhere."""
    gh, gw = gt.shape
    plane = np.full((gh, gw), np.nan, F)
    if count == 0:
        return plane
    mask = garg_mask(gt, min_depth, max_depth) if crop else np.logical_and(gt > min_depth, gt < max_depth)
    with np.errstate(divide="ignore"):
        p = (F(1.0) / cv2_resize_linear_ref(np.asarray(pred_disp, F), gw, gh)) * F(scale_factor)
    if median_scaling:
        p = p * F(ratio)
    p = np.where(p < F(min_depth), F(min_depth), p)
    p = np.where(p > F(max_depth), F(max_depth), p).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = (np.abs(gt - p) / gt).astype(F)
    plane[mask] = e[mask]
    return plane


def error_map_ref(pred_disp, gt, ratio, count, lut, image=None, err_max=0.5, radius=2, **kw):
    """(picture uint8 [GH,GW,3], plane float32 [GH,GW]) as bbd_error_map writes them for one map."""
    plane = error_plane_ref(pred_disp, gt, ratio, count, **kw)
    gh, gw = gt.shape
    best = np.full((gh, gw), -np.inf, F)                      # (no NaN errors in the cases: a plain maximum)
    padded = np.full((gh + 2 * radius, gw + 2 * radius), np.nan, F)
    padded[radius:radius + gh, radius:radius + gw] = plane
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            shifted = padded[dy:dy + gh, dx:dx + gw]
            best = np.where(np.isnan(shifted), best, np.maximum(best, shifted))
    any_valid = best > -np.inf
    if image is None:
        background = np.zeros((gh, gw, 3), np.uint8)
    else:
        grey = (image.astype(np.int64).sum(-1) // 6).astype(np.uint8)
        background = np.stack([grey] * 3, -1)
    idx = lut_index_ref(np.where(any_valid, best, F(0.0)), 0.0, err_max)
    picture = np.where(any_valid[..., None], np.asarray(lut)[idx], background).astype(np.uint8)
    return picture, plane
