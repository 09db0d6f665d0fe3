"""Backend-agnostic checks of the colour-mapped disparity (`ops.disp_viz`) - used by the CPU host-port tier
(tests/test_viz_port.py) and by the GPU tier (tests/test_gpu_predict.py).

The acceptance rules, in one place:
  * s (scaled disparity at the original size) is bit-equal to the fixture; against a reference computed live by
    torch on this host's CPU it is compared with rtol 3e-5 / atol 2e-6 (ATen's CPU kernels round per host);
  * vmin is bit-equal to the minimum of the s the backend produced (and, for fixtures, of the fixture's s - the same
    array); the two order statistics in `stats` equal np.partition's; vmax is within 2 float32 ulps of np.percentile;
  * colours (a) EQUAL the documented LUT formula evaluated in numpy from the backend's own s, vmin, vmax, and
    (b) differ from matplotlib's (fixture) or the live reference's on at most max(2, 1e-4 * H0 * W0) pixels, every
    one of them exactly one LUT step away from the reference's entry.
"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "viz_cases.npz")
CASES = ["small_up", "small_down", "small_same", "big_up", "big_down", "big_same", "constant", "tied_max"]
MIN_DEPTH, MAX_DEPTH = 0.1, 80.0


def lut_formula(s, vmin, vmax, lut):
    """The documented colour rule in numpy float32: index trunc((s - vmin) / (vmax - vmin) * 256), 256 -> 255, above
    -> 255, vmax == vmin -> 0; colour = lut[index]."""
    s = np.asarray(s, np.float32)
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    if vmax == vmin:
        return lut[np.zeros(s.shape, np.int64)]
    x = (s - vmin) / (vmax - vmin)
    xi = x * np.float32(256)
    idx = np.minimum(xi, np.float32(255.5)).astype(np.int64)     # truncation; everything >= 256 lands on 255
    idx[xi >= 256] = 255
    return lut[np.clip(idx, 0, 255)]


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    assert a > 0 and b > 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def live_reference(disp, H0, W0, lut, percentile=95):
    """test_simple.py:135-148 on this host: torch CPU interpolation, disp_to_depth's scaling, np.percentile, and the
    LUT formula.  disp: torch [1,1,h,w] on the CPU."""
    d = torch.nn.functional.interpolate(disp, (H0, W0), mode="bilinear", align_corners=False)
    min_disp, max_disp = 1 / MAX_DEPTH, 1 / MIN_DEPTH
    s = (min_disp + (max_disp - min_disp) * d).squeeze().numpy()
    vmax = np.percentile(s, percentile)
    return s, s.min(), vmax, lut_formula(s, s.min(), vmax, lut)


def check_stats(s, stats, percentile=95):
    """vmin / order statistics / vmax of one image against numpy on the SAME s."""
    flat = np.ascontiguousarray(s, np.float32).ravel()
    n = flat.size
    vmin, vmax, lower, upper = (np.float32(v) for v in stats)
    assert vmin == flat.min()
    q = np.float32(percentile) / np.float32(100)
    vi = np.float32(n - 1) * q
    lo_rank = n - 1 if vi >= n - 1 else int(np.floor(vi))
    hi_rank = min(lo_rank + 1, n - 1)
    part = np.partition(flat, [lo_rank, hi_rank])
    assert lower == part[lo_rank] and upper == part[hi_rank], (lower, upper, part[lo_rank], part[hi_rank])
    want = np.percentile(flat, percentile)
    assert want.dtype == np.float32
    u = ulps(vmax, want)
    print("vmax %r  np.percentile %r  ulps %d" % (float(vmax), float(want), u))
    assert u <= 2, (vmax, want)


def _entries(lut, colour):
    return np.nonzero((lut == colour[None, :]).all(1))[0]


def check_colours(got, s, stats, lut, reference):
    """(a) equality with the formula on the backend's own numbers, (b) the capped one-step rule against `reference`."""
    assert got.dtype == np.uint8 and got.shape == s.shape + (3,)
    assert np.array_equal(got, lut_formula(s, stats[0], stats[1], lut))
    diff = (got != reference).any(-1)
    count, cap = int(diff.sum()), max(2, int(1e-4 * s.size))
    print("pixels differing from the reference: %d of %d (cap %d)" % (count, s.size, cap))
    assert count <= cap, (count, cap)
    for y, x in zip(*np.nonzero(diff)):
        gi, ri = _entries(lut, got[y, x]), _entries(lut, reference[y, x])
        assert gi.size and ri.size
        assert np.abs(gi[:, None] - ri[None, :]).min() == 1, (y, x, gi, ri)


def run_fixture_case(name, backend, device, vectors=None):
    from baseboostdepth_amd import ops
    v = vectors if vectors is not None else np.load(GOLDEN)
    lut = ops.magma_lut("cpu").numpy()
    disp = torch.from_numpy(v[name + "/disp"]).to(device)
    H0, W0 = (int(k) for k in v[name + "/size"])
    colour, floats, stats = ops.disp_viz(disp, [(H0, W0)], MIN_DEPTH, MAX_DEPTH, 95.0, want_float=True, backend=backend)
    s, st, col = floats[0].cpu().numpy(), stats[0].cpu().numpy(), colour[0].cpu().numpy()
    want_s = v[name + "/s"]
    assert s.shape == (H0, W0) and np.array_equal(s.view(np.uint32), want_s.view(np.uint32)), name
    assert np.float32(st[0]) == want_s.min() == v[name + "/vmin"]
    check_stats(want_s, st)
    assert ulps(st[1], v[name + "/vmax"]) <= 2
    check_colours(col, s, st, lut, v[name + "/colour"])
    return col, s, st
