"""The shared cases of the semi-global stereo matcher (bbd_sgm_hints) for both test tiers: the smallest
shapes at which a rule, a lane layout or a border can still go wrong.  `reference(name)` is tests/sgm_ref.py (numpy,
written from the rules), `port_result(name)` the host port over csrc/bbd_sgm_math.h, `run(name, backend, device)` the
product's `ops.stereo_hints` on a backend.  Everything is integer: results are compared byte for byte."""
import functools

import numpy as np
import torch

import sgm_ref

# name: (B, H, W, D, paths, uniqueness, fill, side flags, kind)
CASES = {
    "low":      (1, 5, 40, 64, 8, 5, False, (0,), "floats"),         # H below the census height, W below D
    "two":      (2, 12, 70, 64, 8, 5, True, (0, 0), "planes"),
    "lanes2":   (1, 9, 150, 128, 4, 5, False, (0,), "planes"),       # two disparities a lane, W no multiple of 64, 4 paths
    "mixed":    (3, 16, 33, 64, 8, 0, False, (0, 1, 1), "planes"),   # mixed side flags, uniqueness off
    "lanes3":   (1, 6, 90, 192, 8, 5, True, (1,), "planes"),         # three disparities a lane (unaligned element loads)
    "wide":     (1, 7, 300, 256, 8, 5, False, (0,), "planes"),       # the largest D
    "constant": (1, 8, 48, 64, 8, 5, True, (0,), "constant"),        # all ties: the written rules decide
    "none":     (1, 6, 40, 64, 8, 99, True, (0,), "noise"),          # rows without a valid pixel stay invalid under fill
    "planted":  (1, 24, 160, 64, 8, 5, False, (0,), "planted"),
}
PLANTED_SHIFT = 11
# The interior of the planted-shift case: every pixel at least this far from the four borders and from the zone x < d0
# whose match lies outside the image.  A census window reaches 4 columns and 3 rows; next to the zone x < d0 the right
# image's window is clamped while the left one is not, and next to it the horizontal paths have not yet seen an
# unambiguous pixel.  8 = two window half-widths is the smallest margin tried; the reference meets it at 100 %
# (tests/test_sgm_port.py asserts that before any other result is held against the reference).
PLANTED_MARGIN = 8


def _bytes(rng, *shape):
    return rng.integers(0, 256, shape).astype(np.float32) / np.float32(255.0)


def _shifted(rng, left, shift):
    """The partner of `left` [3,H,W] for matches at x - shift: right(x) = left(x + shift), fresh random columns where
    the shift leaves none."""
    W = left.shape[2]
    right = _bytes(rng, *left.shape)
    if shift < W:
        right[:, :, :W - shift] = left[:, :, shift:]
    return right


@functools.lru_cache(maxsize=None)
def make(name):
    B, H, W, D, paths, uniq, fill, side, kind = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    left = np.zeros((B, 3, H, W), np.float32)
    right = np.zeros_like(left)
    for b in range(B):
        if kind == "floats":                                  # no byte values: the rounding of the grey rule
            left[b] = rng.random((3, H, W), np.float32) * np.float32(1.1) - np.float32(0.05)
            right[b] = _shifted(rng, left[b], 6) + (rng.random((3, H, W), np.float32) - 0.5) * np.float32(0.02)
            left[b, 0, 0, 0], left[b, 1, 0, 1] = np.nan, np.inf
        elif kind == "constant":
            left[b], right[b] = 0.5, 0.5
        elif kind == "noise":
            left[b], right[b] = _bytes(rng, 3, H, W), _bytes(rng, 3, H, W)
        elif kind == "planted":
            left[b] = _bytes(rng, 3, H, W)
            right[b] = _shifted(rng, left[b], PLANTED_SHIFT)
        else:                                                 # two fronto-parallel planes and a little noise
            left[b] = _bytes(rng, 3, H, W)
            near, far = int(rng.integers(8, min(D, W) // 2)), int(rng.integers(1, 6))
            right[b] = _shifted(rng, left[b], far)
            right[b][:, H // 2:] = _shifted(rng, left[b], near)[:, H // 2:]
            noise = rng.integers(-2, 3, right[b].shape).astype(np.float32) / np.float32(255.0)
            right[b] = np.clip(right[b] + noise, 0, 1)
        if side[b]:                                           # the mirrored pair of the same scene
            left[b], right[b] = left[b][:, :, ::-1].copy(), right[b][:, :, ::-1].copy()
    return dict(left=left, right=right, side=np.array(side, np.int32), D=D, paths=paths, uniqueness=uniq, fill=fill)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = make(name)
    return sgm_ref.stereo_hints(c["left"], c["right"], c["side"], c["D"], c["paths"], uniqueness=c["uniqueness"],
                                fill=c["fill"])


def run(name, backend, device, **over):
    from baseboostdepth_amd import ops
    c = dict(make(name), **over)
    disp16, count = ops.stereo_hints(torch.from_numpy(c["left"]).to(device), torch.from_numpy(c["right"]).to(device),
                                     torch.from_numpy(c["side"]).to(device), c["D"], c["paths"],
                                     uniqueness=c["uniqueness"], fill=c["fill"], backend=backend)
    return disp16.cpu().numpy(), count.cpu().numpy()


@functools.lru_cache(maxsize=None)
def port_result(name):
    from ports import PortBackend
    return run(name, PortBackend(), "cpu")


def same(got, want):
    """Byte equality of (disp16, valid_count) pairs, shapes and types included."""
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def planted_interior(disp16):
    m, d0 = PLANTED_MARGIN, PLANTED_SHIFT
    return disp16[:, m:-m, d0 + m:-m]
