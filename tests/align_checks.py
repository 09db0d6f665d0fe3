"""Case builders and assertions of the affine-invariant depth evaluation, shared by the CPU tier (tests/test_align_port.py,
tests/test_align_cli.py: the host port) and the GPU tier (tests/test_gpu_align.py: the kernel).  What a case needs to
be a case - spread of the prediction, number of scored pixels, share of capped pixels - is asserted here in numpy
(tests/align_ref.py) before a test relies on it; the reference rows are computed once per case."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_ref  # noqa: E402
from baseboostdepth_amd import evaluation  # noqa: E402

SIZES = [(40, 100), (37, 123), (64, 96), (64, 96)]        # 64 x 96 = 6144 pixels: the 1024-thread loops wrap
PRED_SIZES = [(24, 80), (96, 160)]                        # up-samples for every map / down-samples for the first two
GAUGES = [(0.37, 0.004), (2.5, -0.003), (1.3, 0.01), (0.8, -0.002)]      # x = (1 / z - o0) / s0
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0
ERR_COLUMNS = [0, 1, 2, 3, 4, 5, 6, 9, 11]
ERR_TOL = dict(rtol=3e-5, atol=2e-6)                      # tests/test_gpu_eval.py
FIT_RTOL = 1e-6                                           # scale and shift against numpy: seven orders above the
#                                                           spread between summation orders (below 4e-14)


class Case:
    def __init__(self, preds, gts, crop):
        self.preds = np.ascontiguousarray(preds, np.float32)          # [n,h,w]
        self.gts = [np.ascontiguousarray(g, np.float32) for g in gts]
        self.crop = crop
        self._want = None

    def windows(self):
        return [evaluation.garg_window(*g.shape) if self.crop else (0, g.shape[0], 0, g.shape[1]) for g in self.gts]

    def want(self):
        """The numpy reference rows [n, 12]; computed once, never written to."""
        if self._want is None:
            self._want = align_ref.rows(self.preds, self.gts, self.windows(), MIN_DEPTH, MAX_DEPTH)
            self._want.setflags(write=False)
        return self._want

    def run(self, backend, device, order=None):
        """The rows of `evaluation.depth_metrics_affine` as float64 numpy [n, 12]; `order` permutes the batch."""
        order = list(range(len(self.gts))) if order is None else list(order)
        truth = evaluation.GroundTruthSet(self.gts, device, crop=self.crop)
        pred = torch.from_numpy(self.preds[order]).to(device)
        out = evaluation.depth_metrics_affine(pred, truth, order, MIN_DEPTH, MAX_DEPTH, backend=backend)
        assert out.dtype == torch.float64 and tuple(out.shape) == (len(order), 12) and out.device == pred.device
        return out.cpu().numpy()

    def metrics_counts(self, backend, device):
        """Column 10 of `evaluation.depth_metrics` for the same inputs."""
        truth = evaluation.GroundTruthSet(self.gts, device, crop=self.crop)
        rows = evaluation.depth_metrics(torch.from_numpy(self.preds).to(device), truth, list(range(len(self.gts))),
                                        min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_is_disp=True, median="numpy",
                                        backend=backend)
        return rows[:, 10].cpu().numpy().astype(np.float64)


def _depth(shape, k):
    """A smooth dense depth in (1, 79) at the pixel centres of a `shape` grid: near at the bottom, far at the top."""
    h, w = shape
    v = ((np.arange(h) + 0.5) / h)[:, None]
    u = ((np.arange(w) + 0.5) / w)[None, :]
    return 1.8 + 70.0 * (1.0 - v) ** 2 * (0.6 + 0.4 * np.cos(3.0 * u + k)) + 3.0 * u * v


def _sparse(depth, rng, keep=0.3):
    g = depth.astype(np.float32)
    g[rng.random(g.shape) >= keep] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def common_case(pred_size, crop):
    """The ragged batch every tier scores: an affine distortion of the true inverse depth with 5 % multiplicative noise."""
    rng = np.random.default_rng(2024)
    gts, preds = [], []
    for k, (shape, (s0, o0)) in enumerate(zip(SIZES, GAUGES)):
        g = _sparse(_depth(shape, k), rng)
        assert g[g > 0].min() > 1.0 and g.max() < 79.0
        if k == 2:                                        # values beyond either end of the range: the two compares
            far = rng.random(shape) < 0.05
            g[far] = 90.0 + 10.0 * rng.random(far.sum()).astype(np.float32)
            g[rng.random(shape) < 0.05] = 5e-4
        gts.append(g)
        inv = 1.0 / _depth(pred_size, k)
        preds.append(((inv - o0) / s0 * (1.0 + 0.05 * rng.standard_normal(pred_size))).astype(np.float32))
    case = Case(np.stack(preds), gts, crop)
    counts = []
    for p, g, win in zip(case.preds, case.gts, case.windows()):
        x, _ = align_ref.samples(p, g, win, MIN_DEPTH, MAX_DEPTH)
        assert len(x) >= 64 and np.std(x.astype(np.float64)) / abs(np.mean(x.astype(np.float64))) >= 0.3
        counts.append(len(x))
    if crop:
        assert counts[1] < 1024                           # fewer scored pixels than threads
    else:
        assert max(counts) > 1024                         # and more: a partial sum has several terms
    assert all((r1 - r0) * (c1 - c0) > 1024 for r0, r1, c0, c1 in case.windows())       # the strided loops wrap
    assert (gts[2] > MAX_DEPTH).any() and ((gts[2] > 0) & (gts[2] < MIN_DEPTH)).any()
    return case


COMMON = [(size, crop) for size in PRED_SIZES for crop in (True, False)]


@functools.lru_cache(maxsize=None)
def exact_case(s0, o0):
    """The prediction has the size of the map and IS the inverse depth in another gauge: the fit must undo it."""
    rng = np.random.default_rng(7)
    shape = (40, 100)
    dense = _depth(shape, 0).astype(np.float32)
    x = ((1.0 / dense.astype(np.float64) - o0) / s0).astype(np.float32)
    return Case(x[None], [_sparse(dense, rng)], crop=False)


def assert_exact(row, s0, o0):
    assert row[0] < 1e-5 and row[4] == 1.0
    assert abs(row[7] / s0 - 1.0) < 1e-4
    assert abs(row[8] / o0 - 1.0) < 1e-4 if o0 != 0 else abs(row[8]) < 1e-7


EXACT_GAUGES = [(0.37, 0.004), (2.5, -0.003), (1.0, 0.0)]


@functools.lru_cache(maxsize=None)
def cap_case():
    """A fit that sends pixels below 1 / max_depth: a negative shift, far ground truth and additive noise on its small
    disparities.  At least 1 % of the scored pixels are capped, and the reference scores them at max_depth."""
    rng = np.random.default_rng(11)
    shape, pred_size = (48, 112), (24, 56)

    def depth(size):                                      # 77 m at the top row, 4 m at the bottom: a quarter beyond 60 m
        return np.repeat(78.0 - 75.0 * ((np.arange(size[0]) + 0.5) / size[0])[:, None], size[1], 1)

    g = _sparse(depth(shape), rng)
    x = ((1.0 / depth(pred_size) + 0.003) / 0.5 + 0.004 * rng.standard_normal(pred_size)).astype(np.float32)
    case = Case(x[None], [g], crop=False)
    xs, gs = align_ref.samples(case.preds[0], g, case.windows()[0], MIN_DEPTH, MAX_DEPTH)
    scale, shift = align_ref.fit(xs, gs)
    p, capped = align_ref.aligned_depth(xs, scale, shift, MIN_DEPTH, MAX_DEPTH)
    assert shift < 0 and capped.mean() >= 0.01 and (p[capped] == np.float32(MAX_DEPTH)).all()
    return case


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """Four images: a constant prediction; a map without a valid pixel; a map with exactly one; a NaN inside the support
    of the prediction.  (want_nan_row, want_count or None = the reference's) per image."""
    rng = np.random.default_rng(5)
    shape, pred_size = (40, 100), (24, 80)
    dense = _depth(shape, 1)
    live = (0.2 + rng.random((4,) + pred_size)).astype(np.float32)
    live[0] = 0.25
    live[3, 12, 40] = np.nan
    one = np.zeros(shape, np.float32)
    one[20, 50] = 10.0
    gts = [_sparse(dense, rng), np.zeros(shape, np.float32), one, _sparse(dense, rng)]
    case = Case(live, gts, crop=False)
    x, _ = align_ref.samples(case.preds[3], gts[3], case.windows()[3], MIN_DEPTH, MAX_DEPTH)
    assert np.isnan(x).any() and not np.isnan(x).all()    # the NaN lies among the scored samples
    want = case.want()
    assert want[0, 10] > 64 and want[1, 10] == 0 and want[2, 10] == 1 and want[3, 10] > 64
    return case


NAN_COLUMNS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]


def assert_degenerate(rows, case):
    assert np.isnan(rows[:, NAN_COLUMNS]).all()
    assert np.array_equal(rows[:, 10], case.want()[:, 10])


def assert_close(rows, want):
    """Rows against reference rows: the count exact, scale and shift to FIT_RTOL, the errors to the project's tolerances."""
    assert rows.shape == want.shape and np.array_equal(rows[:, 10], want[:, 10])
    assert np.isfinite(rows).all()
    np.testing.assert_allclose(rows[:, 7:9], want[:, 7:9], rtol=FIT_RTOL, atol=0)
    np.testing.assert_allclose(rows[:, ERR_COLUMNS], want[:, ERR_COLUMNS], **ERR_TOL)


def assert_same_fit(rows, other):
    """Device against port: scale, shift and count as bytes; the errors differ by the two logf implementations."""
    assert np.array_equal(rows[:, [7, 8, 10]].view(np.uint64), other[:, [7, 8, 10]].view(np.uint64))
    np.testing.assert_allclose(rows[:, ERR_COLUMNS], other[:, ERR_COLUMNS], **ERR_TOL)


# ---------------------------------------------------------------------------------------------- evaluate_depth.py
SPLIT_GAUGES = [(0.37, 0.015), (2.5, -0.02), (1.0, 0.0), (0.6, 0.02), (4.0, 0.01), (1.7, -0.03)]


def write_split(tmp_path):
    """A synthetic KITTI split of 6 frames under `tmp_path` and a disparity file that is, frame by frame, another affine
    gauge of the true inverse depth (a plane: linear in the pixel, so the resampling is exact up to rounding).
    Returns (disps, gts, argv)."""
    rng = np.random.default_rng(3)
    h, w = 33, 130
    shapes = [(40, 120), (38, 124), (40, 120), (36, 118), (44, 130), (40, 120)]

    def inverse_depth(shape, k):
        gh, gw = shape
        v = ((np.arange(gh) + 0.5) / gh)[:, None]
        u = ((np.arange(gw) + 0.5) / gw)[None, :]
        return 0.02 + (0.25 + 0.02 * k) * v + 0.05 * u

    gts = np.empty(len(shapes), dtype=object)
    disps = np.zeros((len(shapes), h, w), np.float32)
    for k, (shape, (s0, o0)) in enumerate(zip(shapes, SPLIT_GAUGES)):
        gts[k] = _sparse(1.0 / inverse_depth(shape, k), rng)
        disps[k] = ((inverse_depth((h, w), k) - o0) / s0).astype(np.float32)
    assert disps.min() > 0                                # the median protocol takes 1 / x
    # what the tests rely on, in numpy: the fit undoes the gauge, median scaling cannot
    windows = [evaluation.garg_window(*g.shape) for g in gts]
    lsq = np.mean([align_ref.row(d, g, win)[0] for d, g, win in zip(disps, gts, windows)])
    med = np.mean([align_ref.median_scaled_abs_rel(d, g, win) for d, g, win in zip(disps, gts, windows)])
    assert lsq < 1e-3 and med >= 10.0 * lsq
    split = tmp_path / "splits" / "eigen"
    split.mkdir(parents=True)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    np.save(tmp_path / "disps.npy", disps)
    return disps, gts, ("--eval_split", "eigen", "--splits_dir", tmp_path / "splits", "--ext_disp_to_eval",
                        tmp_path / "disps.npy")
