"""Numpy float64 statement of the affine-invariant depth evaluation, written from its description and
sharing no code with the kernel, its math header or the host port: `np.sum` in numpy's own (pairwise) order.

For one image: the scored pixels are those inside the crop window with min_depth < g < max_depth (float32 compares);
x is the cv2-style linear resize of the prediction (float32), t = 1 / g in float64; centred least squares of t on x
gives scale and shift; the aligned disparity is capped below at 1 / max_depth, inverted, rounded to float32 and clamped
to the depth range; the seven KITTI errors are formed in float32 and averaged in float64; SILog and iRMSE follow."""
import numpy as np

COLUMNS = 12
F32 = np.float32


def _axis(n_out, n_in):
    """Taps and weight of cv2's INTER_LINEAR along one axis: half-pixel centres, the coordinate computed in float64 and
    rounded to float32, taps outside the image collapse onto the border with weight 0."""
    c = ((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5).astype(F32)
    i0 = np.floor(c).astype(np.int64)
    f = (c - i0.astype(F32)).astype(F32)
    under, over = i0 < 0, i0 >= n_in - 1
    i0[under], f[under] = 0, 0.0
    i0[over], f[over] = n_in - 1, 0.0
    return i0, np.minimum(i0 + 1, n_in - 1), f


def resize_linear(img, gh, gw):
    """cv2.resize(img, (gw, gh), INTER_LINEAR) of a float32 image: the horizontal pass, then the vertical one, every
    product and sum rounded to float32."""
    img = np.asarray(img, F32)
    h, w = img.shape
    x0, x1, fx = _axis(gw, w)
    y0, y1, fy = _axis(gh, h)
    one = F32(1.0)
    with np.errstate(invalid="ignore"):
        rows = (img[:, x0] * (one - fx)[None, :]).astype(F32) + (img[:, x1] * fx[None, :]).astype(F32)
        return ((rows[y0] * (one - fy)[:, None]).astype(F32) + (rows[y1] * fy[:, None]).astype(F32)).astype(F32)


def scored(gt, window, min_depth, max_depth):
    gt = np.asarray(gt, F32)
    r0, r1, c0, c1 = window
    mask = np.zeros(gt.shape, bool)
    mask[max(r0, 0):r1, max(c0, 0):c1] = True
    return mask & (gt > F32(min_depth)) & (gt < F32(max_depth))


def samples(pred, gt, window, min_depth=1e-3, max_depth=80.0):
    """(x float32 [N], g float32 [N]) of the scored pixels, in row-major order."""
    gt = np.asarray(gt, F32)
    mask = scored(gt, window, min_depth, max_depth)
    return resize_linear(pred, *gt.shape)[mask], gt[mask]


def fit(x32, g32):
    x, t = x32.astype(np.float64), 1.0 / g32.astype(np.float64)
    n = len(x)
    mx, mt = np.sum(x) / n, np.sum(t) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sum((x - mx) * (t - mt)) / np.sum((x - mx) ** 2)
    return scale, mt - scale * mx


def aligned_depth(x32, scale, shift, min_depth=1e-3, max_depth=80.0):
    """(p float32 [N], capped bool [N]): the aligned depth of every sample and whether the disparity cap took it."""
    with np.errstate(invalid="ignore"):
        a = scale * x32.astype(np.float64) + shift
        capped = a < 1.0 / max_depth
        a = np.where(capped, 1.0 / max_depth, a)
        p = (1.0 / a).astype(F32)
        p = np.where(p < F32(min_depth), F32(min_depth), p)
        p = np.where(p > F32(max_depth), F32(max_depth), p)
    return p.astype(F32), capped


def row(pred, gt, window, min_depth=1e-3, max_depth=80.0):
    """The 12 columns abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, scale, shift, silog, count, irmse of one image."""
    x, g = samples(pred, gt, window, min_depth, max_depth)
    n = len(x)
    out = np.full(COLUMNS, np.nan)
    out[10] = n
    with np.errstate(invalid="ignore"):
        if n < 2 or np.max(x) == np.min(x):                   # degenerate: nothing to fit a line to
            return out
        scale, shift = fit(x, g)
        p, _ = aligned_depth(x, scale, shift, min_depth, max_depth)
        th = np.maximum(g / p, p / g)
        df = g - p
        d = np.log(p) - np.log(g)                              # float32
        mean = lambda v: np.sum(v.astype(np.float64)) / n      # noqa: E731
        out[0] = mean(np.abs(df) / g)
        out[1] = mean(df * df / g)
        out[2] = np.sqrt(mean(df * df))
        out[3] = np.sqrt(mean(d * d))
        # a NaN of the fit reaches every column: the compares are false on it and would read 0
        lost = np.nan if np.isnan(scale) or np.isnan(shift) else 0.0
        for k, bound in enumerate((1.25, 1.25 ** 2, 1.25 ** 3)):
            out[4 + k] = mean(th < F32(bound)) + lost
        out[7], out[8] = scale, shift
        d64 = d.astype(np.float64)
        out[9] = 100.0 * np.sqrt(np.maximum(np.sum(d64 * d64) / n - (np.sum(d64) / n) ** 2, 0.0))
        inv = 1.0 / p.astype(np.float64) - 1.0 / g.astype(np.float64)
        out[11] = 1000.0 * np.sqrt(np.sum(inv * inv) / n)
    return out


def rows(preds, gts, windows, min_depth=1e-3, max_depth=80.0):
    return np.stack([row(p, g, w, min_depth, max_depth) for p, g, w in zip(preds, gts, windows)])


def median_scaled_abs_rel(pred_disp, gt, window, min_depth=1e-3, max_depth=80.0):
    """abs_rel of the same disparity under median scaling (what `--scale_recovery median` scores), for comparison."""
    x, g = samples(pred_disp, gt, window, min_depth, max_depth)
    p = (F32(1.0) / x).astype(F32)
    p = (p * F32(np.median(g) / np.median(p))).astype(F32)
    p = np.clip(p, F32(min_depth), F32(max_depth))
    return float(np.mean(np.abs(g - p).astype(np.float64) / g))
