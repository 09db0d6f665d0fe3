"""CPU tier of depth-pose consistency: the host port of bbd_consist.hip (same bbd_consist_math.h) through the `backend=`
seam of `ops.depth_consistency` against the numpy reference (tests/consist_ref.py), byte for byte, on the cases of
tests/consist_checks.py; `pointcloud.neighbour_sources`; the ValueErrors; the composition with `SceneMap`."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import consist_checks as cc  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, ops, pointcloud  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.mark.parametrize("name", cc.CASES)
def test_host_port_matches_the_reference(port, name):
    cc.precondition(name)
    assert cc.differing(cc.run(name, port, "cpu"), cc.reference(name)) == []


def test_the_optional_outputs_are_optional(port):
    case = cc.make("neighbours")
    res = cc.call(case, port, "cpu", want_err=False, want_filtered=False)
    assert res.err is None and res.filtered is None
    assert cc.same_bytes(res.agree.numpy(), cc.reference("neighbours")["agree"])
    assert res.counters.dtype == torch.int64 and tuple(res.counters.shape) == (3, _lib.CONSIST_COUNTERS)
    assert tuple(res.transforms.shape) == (3, 2, 12) and res._fields == ("filtered", "seen", "agree", "err", "counters",
                                                                        "transforms")


def test_a_four_dimensional_disparity_and_flat_poses_are_taken(port):
    case = cc.make("neighbours")
    res = ops.depth_consistency(torch.from_numpy(case["disp"])[:, None], torch.from_numpy(case["poses"]).reshape(3, 16),
                                torch.from_numpy(case["K"]), torch.from_numpy(case["inv_K"]),
                                torch.from_numpy(case["sources"]), want_err=True, backend=port)
    assert cc.differing({k: getattr(res, k).numpy() for k in cc.OUTPUTS}, cc.reference("neighbours")) == []


def test_maps_too_thin_to_sample_have_no_visible_samples(port):
    for shape in ((2, 1, 9), (2, 7, 1)):
        res = ops.depth_consistency(torch.full(shape, 0.125), torch.eye(4, dtype=torch.float64).repeat(2, 1, 1),
                                    *cc.exact_camera(), np.array([[1], [0]], np.int32), want_err=True, backend=port)
        assert not res.seen.any() and res.counters[:, 1:4].sum() == 0 and res.counters[:, 0].tolist() == [shape[1] * shape[2]] * 2
        assert torch.isnan(res.err).all() and not res.filtered.any()


def test_neighbour_sources():
    assert pointcloud.neighbour_sources(4).tolist() == [[-1, 1], [0, 2], [1, 3], [2, -1]]
    assert pointcloud.neighbour_sources(3, (-1, 1, -2, 2)).tolist() == [[-1, 1, -1, 2], [0, 2, -1, -1], [1, -1, 0, -1]]
    assert pointcloud.neighbour_sources(1).tolist() == [[-1, -1]]
    table = pointcloud.neighbour_sources(5, (2,))
    assert table.dtype == np.int32 and table.flags.c_contiguous and table.tolist() == [[2], [3], [4], [-1], [-1]]
    for bad in ((0, (-1, 1)), (3, ())):
        with pytest.raises(ValueError, match="neighbour_sources"):
            pointcloud.neighbour_sources(*bad)


def test_value_errors(port):
    case = cc.make("neighbours")
    disp, poses = torch.from_numpy(case["disp"]), torch.from_numpy(case["poses"])
    K, inv_K, sources = case["K"], case["inv_K"], case["sources"]
    port.calls.clear()
    for args, kw, said in (
            ((disp.double(), poses, K, inv_K, sources), {}, "disp must be float32"),
            ((disp[0], poses, K, inv_K, sources), {}, "disp must be float32"),
            ((disp, poses.float(), K, inv_K, sources), {}, "poses must be float64"),
            ((disp, poses[:2], K, inv_K, sources), {}, "poses must be float64"),
            ((disp, poses, K[:2], inv_K, sources), {}, "K must be float32"),
            ((disp, poses, K, np.eye(4, dtype=np.float32), sources), {}, "inv_K must be float32"),
            ((disp, poses, K, inv_K, sources.astype(np.int64)), {}, "sources must be int32"),
            ((disp, poses, K, inv_K, sources[:2]), {}, "sources must be int32"),
            ((disp, poses, K, inv_K, np.zeros((3, 9), np.int32)), {}, "1 <= V <= 8"),
            ((disp, poses, K, inv_K, np.zeros((3, 0), np.int32)), {}, "1 <= V <= 8"),
            ((disp, poses, K, inv_K, sources), dict(threshold=-1.0), "threshold must not be negative"),
            ((disp, poses, K, inv_K, sources), dict(threshold=float("nan")), "threshold must not be negative"),
            ((disp, poses, K, inv_K, sources), dict(min_views=-1), "min_views must not be negative"),
            ((disp[:0], poses[:0], K, inv_K, sources[:0]), {}, "at least one frame")):
        with pytest.raises(ValueError, match="depth_consistency: .*" + said):
            ops.depth_consistency(*args, backend=port, **kw)
    assert port.calls == []


def test_argument_errors_write_nothing(port):
    cc.bad_argument_sweep(port.status, "cpu")


def test_identical_calls_give_identical_bytes(port):
    assert cc.differing(cc.run("spoilt", port, "cpu"), cc.run("spoilt", port, "cpu")) == []


def test_scene_map_of_the_filtered_disparities(port):
    cc.scene_map_composition(port, "cpu", with_state=True)
