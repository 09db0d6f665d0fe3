"""numpy restatement of the training-log panel's tile kinds, written from the description in include/bbd_hip.h and
independently of bbd_panel_math.h: what tests/test_panel_port.py holds the host port (and through it the HIP kernels)
to, byte for byte."""
import numpy as np

F = np.float32


def quantise(x):
    """fp32 in [0,1] -> uint8, rounded to nearest; NaN -> 0."""
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, x, F(0))
        c = np.where(c < 1, c, F(1)).astype(F)
    return (c * F(255) + F(0.5)).astype(np.int32).astype(np.uint8)


def color_tile(img):
    """[3,H,W] -> [H,W,3] uint8."""
    return quantise(img).transpose(1, 2, 0)


def scalar_tile(plane, lut):
    """[H,W] fp32, lut uint8 [256,3] -> ([H,W,3] uint8, (min, max)): matplotlib's Normalize + 256-entry lookup between
    the plane's nanmin and nanmax; a constant plane and NaNs take entry 0."""
    plane = np.asarray(plane, dtype=F)
    finite = plane[~np.isnan(plane)]
    if finite.size == 0:
        return np.broadcast_to(lut[0], plane.shape + (3,)).copy(), (F("nan"), F("nan"))
    lo, hi = finite.min(), finite.max()
    if hi == lo:
        return np.broadcast_to(lut[0], plane.shape + (3,)).copy(), (lo, hi)
    with np.errstate(invalid="ignore"):
        xi = ((plane - lo) / (hi - lo)).astype(F) * F(256)
        idx = np.where(xi < 256, np.trunc(xi), 255.0)
        idx = np.where(np.isnan(xi), 0.0, idx)
    idx = np.clip(idx, 0, 255).astype(np.int64)
    return lut[idx], (lo, hi)


def argmin_tile(ids, palette, n_t, n_e):
    """[H,W] uint8 ids, palette uint8 [20,3] -> [H,W,3]."""
    ids = np.asarray(ids).astype(np.int64)
    out = np.zeros(ids.shape + (3,), dtype=np.uint8)
    true = ids < n_t
    err = (ids >= n_t) & (ids < n_t + n_e)
    out[true] = palette[ids[true]]
    out[err] = palette[ids[err] - n_t] >> 1
    return out


def place(cells, rows, cols, H, W):
    """{(row, col): [H,W,3]} -> [rows*H, cols*W, 3]; cells not named are zero."""
    out = np.zeros((rows * H, cols * W, 3), dtype=np.uint8)
    for (r, c), tile in cells.items():
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = tile
    return out


def cell(panel, r, c, H, W):
    return panel[r * H:(r + 1) * H, c * W:(c + 1) * W]
