"""CPU tier of the uncertainty kernels: the host port (tests/host_port/bbd_uncert_port.cpp: the kernels' own
arithmetic and addition order, bbd_uncert_math.h) against the numpy reference (tests/uncert_ref.py) on every case of
tests/uncert_checks.py.

  a1 curves, N        by equality: counts of ranked pixels divided once
  other curve values  relative 1e-9 + absolute 1e-12.  The port adds float64 terms in the kernels' order, the reference
  and the six scores  with math.fsum; reordering a sum of N <= 2^19 non-negative terms moves it by at most N * 2^-53, about
                      6e-11 relative.  1e-9 leaves an order of magnitude and still exposes ONE misplaced pixel of 30 720
                      (its term is 3e-5 of the sum on average, and the cases' errors vary by far more than that).
  curve point 0       against rows[i][0], [2], [4] of `depth_metrics` on the port: a1 by float32 equality, abs_rel and
                      rmse within two float32 ulps (float64 results of differently ordered sums, rounded once).
  flip                `out` byte-equal to ops.post_process_disp, `uncert` byte-equal to numpy."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncert_checks as uc  # noqa: E402
import uncert_ref as ref  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, evaluation, ops  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def close(got, want):
    return np.isclose(got, want, rtol=1e-9, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("name", uc.CASES)
def test_host_port_matches_the_reference(port, name):
    uc.precondition(name)
    K = uc.make(name)["K"]
    got, want = uc.run(name, port, "cpu"), uc.reference(name)["out"]
    assert got.shape == want.shape == (len(uc.make(name)["gts"]), 8 + 6 * (K + 1))
    gs, gc = uc.split(got, K)
    ws, wc = uc.split(want, K)
    worst = np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)
    print("%s: largest relative difference %.3g" % (name, worst))
    assert uc.same_bytes(gs[:, 6:], ws[:, 6:])                                  # N and the spare zero
    assert np.array_equal(gc[:, :, 2], wc[:, :, 2], equal_nan=True)             # the a1 curves
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert close(gc, wc).all() and close(gs[:, :6], ws[:, :6]).all()


@pytest.mark.parametrize("name", uc.CASES)
def test_curve_point_zero_is_the_metrics_row(port, name):
    K = uc.make(name)["K"]
    summary, curves = uc.split(uc.run(name, port, "cpu"), K)
    rows = uc.rows(name)
    for i in range(rows.shape[0]):
        if summary[i, 6] == 0:
            assert rows[i, 10] == 0
            continue
        assert summary[i, 6] == rows[i, 10]
        abs_rel, rmse, a1 = (np.float32(v) for v in curves[i, 0, :, 0])
        print("%s[%d]: abs_rel %r / %r, rmse %r / %r, a1 %r / %r" % (name, i, abs_rel, rows[i, 0], rmse, rows[i, 2], a1, rows[i, 4]))
        assert a1 == rows[i, 4]
        for mine, theirs in ((abs_rel, rows[i, 0]), (rmse, rows[i, 2])):
            if np.isnan(theirs):
                assert np.isnan(mine)
            else:
                assert abs(float(mine) - float(theirs)) <= 2 * float(np.spacing(np.abs(theirs)))


@pytest.mark.parametrize("w", uc.FLIP_WIDTHS)
def test_flip_pass(port, w):
    out, uncert, blended = uc.run_flip(w, port, "cpu")
    assert uc.same_bytes(out, blended)
    assert uc.same_bytes(uncert, ref.flip_uncert(uc.make_flip(w))) and (uncert > 0).any()


def test_identical_calls_give_identical_bytes(port):
    assert uc.same_bytes(uc.run("spoilt", port, "cpu"), uc.run("spoilt", port, "cpu"))


def test_argument_errors_write_nothing(port):
    got = uc.bad_argument_sweep(port.status, "cpu")
    assert uc.same_bytes(got, uc.run("ragged", port, "cpu"))


def test_a_scratch_sized_for_fewer_pixels_gives_nan_rows(port):
    """The capacity is read from scratch_bytes; windows that exceed it cannot be refused on the host (the windows are on
    the device): nothing is sorted and every row is NaN, N included."""
    case = uc.make("ragged")
    n, h, w = case["pred"].shape
    K = case["K"]
    gts = evaluation.GroundTruthSet(case["gts"], "cpu", crop=True)
    short = ops.sparsification_scratch_bytes(gts.desc_host, n) - _lib.SPARS_SCRATCH_PIXEL
    out = torch.full((n, 8 + 6 * (K + 1)), 7.0, dtype=torch.float64)
    scratch = torch.zeros(short // 8 + 1, dtype=torch.int64)
    p = _lib.ptr
    rc = port.status("bbd_sparsification", p(torch.from_numpy(case["pred"])), p(torch.from_numpy(case["uncert"])),
                     p(gts.buffer), p(gts.desc), p(torch.from_numpy(uc.rows("ragged").copy())), p(out), p(scratch), short, n,
                     h, w, K, 1e-3, 80.0, 1.0, 0)
    assert rc == 0 and np.isnan(out[:, :7].numpy()).all() and (out[:, 7] == 0).all() and np.isnan(out[:, 8:].numpy()).all()


def test_value_errors(port):
    case = uc.make("tiny")
    gts = evaluation.GroundTruthSet(case["gts"], "cpu", crop=False)
    pred, uncert, rows = torch.from_numpy(case["pred"]), torch.from_numpy(case["uncert"]), torch.from_numpy(uc.rows("tiny").copy())
    for K in (0, 101):
        with pytest.raises(ValueError, match="intervals"):
            ops.sparsification(pred, uncert, gts, [0, 1, 2], rows, intervals=K, backend=port)
    with pytest.raises(ValueError, match="uncert"):
        ops.sparsification(pred, uncert[:, :, :3], gts, [0, 1, 2], rows, backend=port)
    with pytest.raises(ValueError, match="even"):
        ops.post_process_uncert(torch.rand(3, 4, 5), backend=port)
    with pytest.raises(ValueError, match="2n"):
        ops.post_process_uncert(torch.rand(4, 5), backend=port)
    out, uncert = ops.post_process_uncert(torch.rand(4, 1, 3, 5), backend=port)          # [2n,1,h,w] is taken
    assert tuple(out.shape) == tuple(uncert.shape) == (2, 3, 5)
    assert _lib.ABI_VERSION >= 23 and _lib.SPARS_SUMMARY == 8 and _lib.SPARS_MAX_INTERVALS == 100
