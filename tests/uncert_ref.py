"""Numpy restatement of `bbd_post_process_uncert` and `bbd_sparsification` (include/bbd_hip.h).  The float32
terms are computed operation by operation in float32 (the oracle's cv2-style resize, then one numpy operation per IEEE
operation); keys, ranks and the tie rule are integers (`np.lexsort`); the sums are `math.fsum` - exactly rounded, so the
reference owes nothing to the order the kernels add in."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.eval_ref import cv2_resize_linear_ref  # noqa: E402

F = np.float32
SUMMARY = 8


def flip_uncert(disp):
    """|disp[i] - flip(disp[n + i])| for disp float32 [2n,h,w]: one float32 subtraction."""
    disp = np.asarray(disp, F)
    n = disp.shape[0] // 2
    return np.abs(disp[:n] - disp[n:, :, ::-1]).astype(F)


def order_key(v):
    """The monotone unsigned key of float32 values: every NaN made 0x7fc00000 and -0 made +0 first; a NaN ranks above
    +inf."""
    v = np.array(v, F)
    bits = v.view(np.uint32).copy()
    bits[np.isnan(v)] = 0x7fc00000
    bits[bits == 0x80000000] = 0
    neg = (bits & 0x80000000) != 0
    return np.where(neg, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def ordering(values):
    """Slots by key descending, slot ascending among equal keys."""
    key = order_key(values).astype(np.int64)
    return np.lexsort((np.arange(key.size), -key))


def valid_mask(gt, window, min_depth, max_depth):
    gh, gw = gt.shape
    r0, r1, c0, c1 = window
    inside = np.zeros((gh, gw), bool)
    inside[max(r0, 0):min(r1, gh), max(c0, 0):min(c1, gw)] = True
    return inside & (gt > F(min_depth)) & (gt < F(max_depth))


def terms(pred, uncert, gt, window, ratio, min_depth=1e-3, max_depth=80.0, scale_factor=1.0, median_scaling=True):
    """The float32 terms of the scored pixels of one map, in pixel order: dict(u, e_abs, e_sq, th, a1, mask)."""
    gt = np.asarray(gt, F)
    gh, gw = gt.shape
    mask = valid_mask(gt, window, min_depth, max_depth)
    with np.errstate(all="ignore"):
        p = (F(1.0) / cv2_resize_linear_ref(np.asarray(pred, F), gw, gh)) * F(scale_factor)
        if median_scaling:
            p = p * F(ratio)
        p = np.where(p < F(min_depth), F(min_depth), p)
        p = np.where(p > F(max_depth), F(max_depth), p).astype(F)
        u = cv2_resize_linear_ref(np.asarray(uncert, F), gw, gh)[mask]
        g, p = gt[mask], p[mask]
        df = (g - p).astype(F)
        e_abs = (np.abs(df) / g).astype(F)
        e_sq = (df * df).astype(F)
        t0, t1 = (g / p).astype(F), (p / g).astype(F)
        th = np.where(t0 > t1, t0, t1).astype(F)
    return dict(u=u.astype(F), e_abs=e_abs, e_sq=e_sq, th=th, a1=th < F(1.25), mask=mask)


def _fsum(x):
    x = np.asarray(x, np.float64)
    return float("nan") if np.isnan(x).any() else math.fsum(x.tolist())


def trapz(c):
    K = len(c) - 1
    return sum((c[k] + c[k + 1]) / 2.0 for k in range(K)) / K


def curves(t, K):
    """(curves float64 [2,3,K+1], a1 counts int64 [2,K], N) of one map's terms."""
    N = int(t["u"].size)
    out = np.full((2, 3, K + 1), np.nan)
    counts = np.zeros((2, K), np.int64)
    if N == 0:
        return out, counts, 0
    by_u = ordering(t["u"])
    orders = [[by_u, by_u, by_u], [ordering(t["e_abs"]), ordering(t["e_sq"]), ordering(t["th"])]]
    for which in range(2):
        for k in range(K):
            r = k * N // K
            left = N - r
            out[which, 0, k] = _fsum(t["e_abs"][orders[which][0][r:]]) / left
            out[which, 1, k] = math.sqrt(_fsum(t["e_sq"][orders[which][1][r:]]) / left)
            counts[which, k] = int(t["a1"][orders[which][2][r:]].sum())
            out[which, 2, k] = float(counts[which, k]) / float(left)
        out[which, :, K] = (0.0, 0.0, 1.0)
    return out, counts, N


def row(t, K):
    """(out row float64 [8 + 6 (K + 1)], a1 counts) of one map's terms."""
    c, counts, N = curves(t, K)
    out = np.full(SUMMARY + 6 * (K + 1), np.nan)
    out[6], out[7] = N, 0.0
    if N:
        for m in range(3):
            ts, to = trapz(c[0, m]), trapz(c[1, m])
            out[m] = to - ts if m == 2 else ts - to
            out[3 + m] = ts - c[0, m, 0] if m == 2 else c[0, m, 0] - ts
        out[SUMMARY:] = c.ravel()
    return out, counts


def sparsification(pred, uncert, gts, windows, ratios, K=50, **kw):
    """dict(out float64 [n, 8 + 6 (K + 1)], counts int64 [n,2,K], terms: the per-map terms)."""
    rows, counts, all_terms = [], [], []
    for i, gt in enumerate(gts):
        t = terms(pred[i], uncert[i], gt, windows[i], ratios[i], **kw)
        r, c = row(t, K)
        rows.append(r)
        counts.append(c)
        all_terms.append(t)
    return dict(out=np.stack(rows), counts=np.stack(counts), terms=all_terms)
