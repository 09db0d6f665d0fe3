"""Shared inputs and checks of the SYNS-Patches tests (CPU tier through the host port, GPU tier through the kernels,
tools/make_golden_syns.py).  Every input is regenerated from a seed; the golden file stores expected outputs only.

Rules (written down before any kernel was run):
  * edge maps: the float32 log and blur are the only stages whose rounding order can differ from the float64
    reference, so a pixel may differ only where |mag - mean| <= delta = 96 * sqrt(2) * 4 * 2^-24 * max|L|
    (96 = sum of absolute Sobel taps, 4 float32 roundings between L and B).  Pixels in that band are left out, and
    their share must be <= 1e-3 of the image.
  * edge metrics: compared against the reference's metrics computed from the map under test (once it has passed the
    rule above); what remains is the order of an fp64 sum of <= 467k non-negative terms, n * 2^-53 ~ 5e-11: rtol 1e-9.
    Counts are equal.
  * distance transforms, nearest-neighbour distances, precision / recall / F-score / IoU: equal.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import syns_ref  # noqa: E402
from oracle import eval_ref  # noqa: E402

BAND_SHARE_CAP = 1e-3
METRIC_RTOL = 1e-9
GOLDEN = os.path.join(ROOT, "tests", "golden", "syns_cases.npz")

# name -> (seed, prediction h, w, ground-truth GH, GW, kind)
CASES = {
    "ramp_a": (3, 48, 160, 94, 310, "ramp"),
    "ramp_b": (4, 48, 160, 90, 300, "ramp"),         # same prediction size, other ground-truth size: one ragged launch
    "noise": (5, 32, 64, 64, 96, "noise"),
    "same_size": (6, 60, 100, 60, 100, "ramp"),
    "full": (7, 192, 640, 376, 1242, "ramp"),
}


def make_depth(seed, h, w, kind="ramp"):
    """Depth map [h,w] float32: a ramp (far at the top) with 25 rectangles of constant depth and 1 % smooth
    multiplicative noise, or uniform noise 2 + 50 * rand."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (2.0 + 50.0 * rng.random((h, w))).astype(np.float32)
    d = np.repeat(np.linspace(60.0, 3.0, h)[:, None], w, 1)
    for _ in range(25):
        y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
        hh, ww = rng.integers(2, max(3, h // 3)), rng.integers(2, max(3, w // 4))
        d[y0:y0 + hh, x0:x0 + ww] = rng.uniform(2.0, 70.0)
    ys, xs = np.mgrid[0:h, 0:w]
    noise = 1.0 + 0.01 * np.sin(ys / 7.0 + rng.uniform(0, 6)) * np.cos(xs / 11.0 + rng.uniform(0, 6))
    return (d * noise).astype(np.float32)


def make_gt(seed, gh, gw, density=0.7):
    """(gt depth [GH,GW] float32 with holes, a few values beyond 125 m; gt edges [GH,GW,1] bool: the depth
    discontinuities of the structure, as SYNS-Patches provides them)."""
    rng = np.random.default_rng(seed + 1000)
    d = make_depth(seed + 2000, gh, gw).astype(np.float64) * (1.0 + 0.05 * rng.standard_normal((gh, gw)))
    jump = np.zeros((gh, gw), bool)
    jump[:, 1:] |= np.abs(np.diff(np.log(d), axis=1)) > 0.25
    jump[1:, :] |= np.abs(np.diff(np.log(d), axis=0)) > 0.25
    d[rng.random((gh, gw)) > density] = 0.0
    d[rng.random((gh, gw)) < 0.01] = 130.0
    return d.astype(np.float32), jump[..., None]


def case_inputs(name):
    seed, h, w, gh, gw, kind = CASES[name]
    depth = make_depth(seed, h, w, kind)
    gt, gt_edge = make_gt(seed, gh, gw)
    return depth, gt, gt_edge


def resized(pred, gh, gw, mode):
    """The prediction at ground-truth size as the reference computes it: mode 'evaluate' takes a disparity (cv2-style
    linear resize, 1 / x), mode 'trainer' a depth (F.interpolate bilinear, clamp to [1e-3, 80])."""
    if mode == "evaluate":
        with np.errstate(divide="ignore"):
            return (np.float32(1) / eval_ref.cv2_resize_linear_ref(np.asarray(pred, np.float32), gw, gh)).astype(np.float32)
    t = torch.from_numpy(np.asarray(pred, np.float32))[None, None]
    return torch.clamp(F.interpolate(t, [gh, gw], mode="bilinear", align_corners=False), 1e-3, 80)[0, 0].numpy()


def depth_range(mode):
    return (np.float32(1e-3), np.float32(125.0)) if mode == "evaluate" else (np.float32(1e-3), np.float32(80.0))


def scaled(pred_gt, gt, mode, median_scaling=True):
    """(median-scaled, clamped prediction; ratio): evaluate_depth.py:277-292 / trainer.py:609-610 without a crop."""
    lo, hi = depth_range(mode)
    m = np.logical_and(gt > lo, gt < hi)
    ratio = np.float32(1)
    if median_scaling:
        if mode == "evaluate":
            ratio = np.float32(np.median(gt[m]) / np.median(pred_gt[m]))
        else:
            ratio = (torch.median(torch.from_numpy(gt[m])) / torch.median(torch.from_numpy(pred_gt[m]))).numpy()
    p = (pred_gt * ratio).astype(np.float32)
    return np.clip(p, lo, hi), ratio


def check_edge_map(got, pred_gt, what="", cap=BAND_SHARE_CAP):
    """The band rule.  `got` [GH,GW] (0/1), `pred_gt` the prediction at ground-truth size.  Returns the band share.
    `cap=None` only where the test does not choose the prediction (the output of a randomly initialised network): the
    cap is a condition on the INPUT, asserted wherever inputs are chosen; no pixel may differ outside the band either
    way."""
    want, mag, mean, delta = syns_ref.pred_edges(pred_gt)
    band = np.abs(mag - mean) <= delta
    share = band.mean()
    print("%s edge map: delta %.3e, band share %.3e, differing pixels %d (outside the band %d)"
          % (what, delta, share, int((np.asarray(got, bool) != want).sum()), int(((np.asarray(got, bool) != want) & ~band).sum())))
    assert cap is None or share <= cap, "%s: %.3e of the image lies within delta of the threshold" % (what, share)
    assert not ((np.asarray(got, bool) != want) & ~band).any(), "%s: edge pixels differ outside the rounding band" % what
    return share


def check_edge_metrics(row, edge, pred_gt, gt, gt_edge, mode, median_scaling=True, what=""):
    """`row`: the 8 doubles of bbd_syns_edge_metrics; `edge`: the map they were computed from."""
    lo, hi = depth_range(mode)
    want = syns_ref.edge_metrics(edge, gt, gt_edge, lo, hi)
    p, _ = scaled(pred_gt, gt, mode, median_scaling)
    want_err = syns_ref.err(p, gt, lo, hi) if want["n_valid"] else np.nan
    print("%s edge metrics: got Acc %.12g comp %.12g err %.12g | want %.12g %.12g %.12g | counts %s"
          % (what, row[0], row[1], row[2], want["edge_Acc"], want["edge_comp"], want_err, [int(c) for c in row[3:7]]))
    assert [int(c) for c in row[3:7]] == [want["n_near"], want["n_tgt"], want["n_valid"], want["n_edge"]], what
    np.testing.assert_allclose(row[:2], [want["edge_Acc"], want["edge_comp"]], rtol=METRIC_RTOL, atol=0, equal_nan=True)
    return want, want_err


def pack_bits(a):
    return np.packbits(np.asarray(a, bool).reshape(-1))


def unpack_bits(b, shape):
    return np.unpackbits(b)[:int(np.prod(shape))].reshape(shape).astype(bool)


def make_syns_tree(root, n, gh=94, gw=310, seed=0):
    """A SYNS-Patches-shaped directory of n synthetic PNGs (<root>/images/<folder>/<frame>.png); returns the split
    lines `folder frame`."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        folder, frame = "%02d" % (i // 2), "%d" % (i % 2)
        os.makedirs(os.path.join(root, "images", folder), exist_ok=True)
        ys, xs = np.mgrid[0:gh, 0:gw]
        img = np.stack([(ys * 2 + i * 17) % 256, (xs + i * 31) % 256, (ys + xs) % 256], -1).astype(np.uint8)
        img[rng.integers(0, gh - 20):, rng.integers(0, gw - 40):] //= 2
        Image.fromarray(img).save(os.path.join(root, "images", folder, frame + ".png"))
        lines.append("%s %s" % (folder, frame))
    return lines
