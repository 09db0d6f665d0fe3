"""CPU reference of bbd_point_cloud (test infrastructure only - never imported by the product path).

numpy in float32, one operation per line in the order csrc/bbd_cloud_math.h states; numpy does not contract a product
and a sum into one operation, so kernel, host port and this file perform the same IEEE operations and agree to the bit.
The resampled prediction of a disparity is what the other references already use, oracle/eval_ref.cv2_resize_linear_ref.
For a depth ATen's own F.interpolate agrees with the kernels' bbd_up_src / bbd_up_blend only to an ulp at arbitrary size
ratios (tests/syns_checks.py allows for that with a band), which equality cannot use, so `upsampled` below restates
those two functions of csrc/bbd_math.h.  Their fused multiply-adds are formed in float64 - the product of two float32
values is exact there - and rounded to float32: that is the fused result except where the float64 sum falls within
2^-53 of the midpoint of two float32 values, which the fixed seeds of the tests do not meet."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import eval_ref  # noqa: E402

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                   ("alpha", "u1")])
ONE = np.float32(1)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _up_src(n_out, n_in):
    """bbd_up_src for every output index: (i0, i1, l0, l1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = scale * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.where(src < 0, np.float32(0), src).astype(np.float32)
    i = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = (src - i.astype(np.float32)).astype(np.float32)
    return i, i + (i < n_in - 1), (ONE - l1).astype(np.float32), l1


def upsampled(img, gh, gw):
    """F.interpolate(bilinear, align_corners=False) as bbd_up_src / bbd_up_blend compute it (csrc/bbd_math.h)."""
    h, w = img.shape
    y0, y1, ly0, ly1 = (v[:, None] for v in _up_src(gh, h))
    x0, x1, lx0, lx1 = (v[None, :] for v in _up_src(gw, w))
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    if gh + gw <= 128:                                   # ATen's kernel for small outputs: four placed products
        acc = (ly0 * lx1) * b
        acc = _fma(ly0 * lx0, a, acc)
        acc = _fma(ly1 * lx0, c, acc)
        return _fma(ly1 * lx1, d, acc)
    top = _fma(lx0, a, lx1 * b)
    bot = _fma(lx0, c, lx1 * d)
    return _fma(ly0, top, ly1 * bot)


def resampled(pred, gh, gw, pred_is_disp, clamp=(1e-3, 80.0), scale_factor=1.0):
    """bbd_eval_resample at every pixel of a gh x gw map."""
    pred = np.asarray(pred, np.float32)
    with np.errstate(all="ignore"):
        if pred_is_disp:
            return ((ONE / eval_ref.cv2_resize_linear_ref(pred, gw, gh)) * np.float32(scale_factor)).astype(np.float32)
        t = upsampled(pred, gh, gw)
        t = np.where(t < np.float32(clamp[0]), np.float32(clamp[0]), t)
        return np.where(t > np.float32(clamp[1]), np.float32(clamp[1]), t).astype(np.float32)


def candidates(gh, gw, window=None, stride=1):
    """Flat pixel indices y * gw + x of the candidates, raster order."""
    r0, r1, c0, c1 = window if window is not None else (0, gh, 0, gw)
    r0, r1, c0, c1 = max(r0, 0), min(r1, gh), max(c0, 0), min(c1, gw)
    ys, xs = np.arange(r0, max(r1, r0), stride), np.arange(c0, max(c1, c0), stride)
    return (ys[:, None] * gw + xs[None, :]).reshape(-1).astype(np.int64)


def lut_index(d, lo, hi):
    with np.errstate(all="ignore"):
        a = ONE / hi
        t = (ONE / d - a) / (ONE / lo - a)
        u = (t * np.float32(256)).astype(np.float32)
        safe = np.where(u > 0, np.minimum(u, np.float32(255)), np.float32(0))          # NaN and negatives -> 0
        return safe.astype(np.int64)                                                    # truncation of [0, 255]


def cloud(pred, shape, inv_K, lut, gt=None, window=None, stride=1, ratio=None, rgb=None, min_depth=1e-3,
          max_depth=80.0, clamp=(1e-3, 80.0), pred_is_disp=False, scale_factor=1.0, from_gt=False, clamp_depth=False,
          mask_gt=False, rays="pixel"):
    """The vertices of ONE image (structured array, `VERTEX`) and the depth of every candidate before the keep rule."""
    gh, gw = shape
    lo, hi = np.float32(min_depth), np.float32(max_depth)
    k = candidates(gh, gw, window, stride)
    with np.errstate(all="ignore"):
        if from_gt:
            d = np.asarray(gt, np.float32).reshape(-1)[k]
        else:
            d = resampled(pred, gh, gw, pred_is_disp, clamp, scale_factor).reshape(-1)[k]
            if ratio is not None:
                d = (d * np.float32(ratio)).astype(np.float32)
        raw = d.copy()
        keep = np.ones(k.shape, bool)
        if mask_gt:
            g = np.asarray(gt, np.float32).reshape(-1)[k]
            keep &= (g > lo) & (g < hi)
        keep &= ~np.isnan(d)
        if clamp_depth:
            d = np.where(d < lo, lo, d)
            d = np.where(d > hi, hi, d)
        else:
            keep &= (d >= lo) & (d <= hi)
        k, d = k[keep], d[keep].astype(np.float32)
        u, v = (k % gw, k // gw) if rays == "pixel" else (k // gh, k % gh)
        u, v = u.astype(np.float32), v.astype(np.float32)
        iK = np.asarray(inv_K, np.float32)
        out = np.zeros(len(k), VERTEX)
        for j, name in enumerate("xyz"):
            out[name] = ((iK[j, 0] * u + iK[j, 1] * v) + iK[j, 2]) * d
        col = np.asarray(rgb, np.uint8).reshape(-1, 3)[k] if rgb is not None else np.asarray(lut, np.uint8)[lut_index(d, lo, hi)]
    out["red"], out["green"], out["blue"], out["alpha"] = col[:, 0], col[:, 1], col[:, 2], 255
    return out, raw
