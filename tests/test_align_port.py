"""CPU tier of the affine-invariant depth evaluation: `evaluation.depth_metrics_affine` through the host
port of bbd_align.hip (tests/host_port/bbd_align_port.cpp: the kernel's own arithmetic and summation order) against
the numpy statement of the protocol (tests/align_ref.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_checks as A  # noqa: E402
from baseboostdepth_amd import _lib, evaluation  # noqa: E402


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


def test_abi_of_the_entry_point():
    assert _lib.ABI_VERSION >= 28 and _lib.ALIGN_OUT == 12 == len(evaluation.ALIGN_COLUMNS)
    proto = _lib.PROTOTYPES["bbd_depth_metrics_affine"]
    assert proto.has_stream and proto.restype is ctypes.c_int
    assert [name for _, name in proto.params] == ["pred", "gt", "desc", "out", "n", "h", "w", "min_depth", "max_depth",
                                                  "flags", "stream"]
    assert evaluation.ALIGN_COLUMNS[7:] == ["scale", "shift", "silog", "count", "irmse"]


@pytest.mark.parametrize("pred_size, crop", A.COMMON)
def test_port_against_the_numpy_reference(port, pred_size, crop):
    case = A.common_case(pred_size, crop)
    A.assert_close(case.run(port, "cpu"), case.want())


@pytest.mark.parametrize("pred_size, crop", A.COMMON)
def test_count_is_the_count_of_depth_metrics(port, pred_size, crop):
    case = A.common_case(pred_size, crop)
    assert np.array_equal(case.run(port, "cpu")[:, 10], case.metrics_counts(port, "cpu"))


def test_rows_do_not_depend_on_the_batch(port):
    case = A.common_case(A.PRED_SIZES[0], True)
    rows = case.run(port, "cpu")
    back = case.run(port, "cpu", order=[3, 2, 1, 0])
    assert np.array_equal(back[::-1].view(np.uint64), rows.view(np.uint64))
    pred4 = torch.from_numpy(case.preds)[:, None]                       # [n,1,h,w] is taken as [n,h,w]
    truth = evaluation.GroundTruthSet(case.gts, "cpu", crop=True)
    again = evaluation.depth_metrics_affine(pred4, truth, [0, 1, 2, 3], backend=port).numpy()
    assert np.array_equal(again.view(np.uint64), rows.view(np.uint64))


@pytest.mark.parametrize("s0, o0", A.EXACT_GAUGES)
def test_exact_recovery(port, s0, o0):
    A.assert_exact(A.exact_case(s0, o0).run(port, "cpu")[0], s0, o0)


def test_the_cap_scores_at_max_depth(port):
    case = A.cap_case()
    A.assert_close(case.run(port, "cpu"), case.want())


def test_degenerate_rows(port):
    case = A.degenerate_case()
    A.assert_degenerate(case.run(port, "cpu"), case)


def test_bad_arguments_are_refused(port):
    case = A.common_case(A.PRED_SIZES[0], True)
    truth = evaluation.GroundTruthSet(case.gts, "cpu")
    pred = torch.from_numpy(case.preds)
    out = torch.zeros(4, 12, dtype=torch.float64)
    n, h, w = pred.shape
    ptr = _lib.ptr
    good = dict(pred=ptr(pred), gt=ptr(truth.buffer), desc=ptr(truth.desc), out=ptr(out), n=n, h=h, w=w, min_depth=1e-3,
                max_depth=80.0, flags=0)

    def status(**change):
        return port.status("bbd_depth_metrics_affine", *dict(good, **change).values())

    assert status() == 0
    null = ctypes.c_void_p(0)
    for change in (dict(pred=null), dict(gt=null), dict(desc=null), dict(out=null), dict(n=0), dict(n=-1), dict(h=0),
                   dict(w=0), dict(flags=1), dict(flags=-1), dict(max_depth=1e-3), dict(max_depth=1e-4),
                   dict(min_depth=-1.0), dict(min_depth=float("nan")), dict(max_depth=float("nan"))):
        assert status(**change) == _lib.E_BADARG, change
    assert status(min_depth=0.0) == 0
