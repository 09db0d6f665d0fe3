"""CPU tier of the scene map: the host port of bbd_map.hip (same bbd_map_math.h) through the `backend=` seam of
`pointcloud.SceneMap` / `ops.map_*` against the numpy reference (tests/map_ref.py; acceptance rules and cases:
tests/map_checks.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_checks as mc  # noqa: E402
import map_ref as ref  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, ops, pointcloud  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def test_the_reference_shows_the_cases_are_what_they_are_for():
    for name in ("merge", "probe"):
        case, p = mc.make(name), mc.reference(name)
        kept = p["verdict"] == ref.KEPT
        _, counts, keys = ref.fuse(p["key"][kept], p["q"][kept], p["rgb"][kept], case["voxel"])
        frame = np.repeat(np.arange(mc.N), kept.size // mc.N)[kept]
        meets = [np.unique(frame[p["key"][kept] == k]).size for k in keys]
        assert kept.sum() == 720 and keys.size < 128 and np.median(counts) >= 10 and max(meets) == 3, (name, keys.size)
    for name in ("fine", "overflow"):
        p = mc.reference(name)
        kept = p["verdict"] == ref.KEPT
        assert np.unique(p["key"][kept]).size == kept.sum()                          # nothing merges
    assert (mc.reference("overflow")["verdict"] == ref.KEPT).sum() == 240
    p = mc.reference("negative")
    assert (p["X"][p["verdict"] == ref.KEPT] < 0).all()
    p = mc.reference("far")
    per_frame = p["verdict"].reshape(mc.N, -1)
    assert (per_frame[1] == ref.OUT_OF_RANGE).all() and (per_frame[[0, 2]] == ref.KEPT).all()
    p = mc.reference("bad_disp")
    assert (p["verdict"] == ref.REJECTED).sum() == 6 + 5 + 4 + 7 + 1 + 1 and (p["verdict"] == ref.OUT_OF_RANGE).sum() == 0
    assert (mc.reference("nan_scale")["verdict"] == ref.REJECTED).all()
    assert mc.reference("merge_s2")["verdict"].size == 3 * 6 * 10 and mc.reference("merge_win")["verdict"].size == 3 * 10 * 17
    assert mc.reference("scaled")["verdict"].size == 3 * 5 * 9
    case, p = mc.make("merge_min3"), mc.reference("merge_min3")
    _, counts, _ = ref.fuse(p["key"], p["q"], p["rgb"], case["voxel"])
    assert (counts < 3).any() and (counts >= 3).any()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_host_port_matches_the_reference(port, name):
    out, counters = mc.run(name, port, "cpu")
    if name in mc.RAISES:
        assert isinstance(out, RuntimeError) and re.search(mc.RAISES[name], str(out)), out
    else:
        assert not isinstance(out, RuntimeError), out
    mc.check(name, out, counters, port)
    assert mc.same_result((out, counters), mc.run(name, port, "cpu"))                 # identical calls, identical bytes


@pytest.mark.parametrize("name", ["merge", "scaled", "far", "bad_disp"])
def test_one_call_of_three_frames_equals_three_calls_of_one(port, name):
    assert mc.same_result(mc.run(name, port, "cpu"), mc.run(name, port, "cpu", split=True))


def test_the_no_merge_flag_is_accepted(port):
    assert mc.same_result(mc.run("merge", port, "cpu"), mc.run("merge", port, "cpu", merge=False))


def test_overflow_is_counted_and_the_call_returns(port):
    out, counters = mc.run("overflow", port, "cpu")
    assert counters.tolist() == [240, 64, 0, 176]
    assert "64 slots" in str(out) and "176 points" in str(out) and "--map_capacity" in str(out)


def test_nan_scale_keeps_nothing(port):
    out, counters = mc.run("nan_scale", port, "cpu")
    assert counters.tolist() == [720, 0, 0, 0] and "no sim3 scale" in str(out)


def test_the_depth_flag_reads_depth(port):
    """The same surface given as depth and as disparity: the depths differ by the rounding of 1 / (1 / d) only."""
    case = mc.make("depth_in")
    as_disp = dict(case, disp=(np.float32(1) / case["disp"]), is_depth=False)
    a = ref.points(case["disp"], case["rgb"], case["poses"], mc.INV_K, **mc.call_kw(case))
    b = ref.points(as_disp["disp"], case["rgb"], case["poses"], mc.INV_K, **mc.call_kw(as_disp))
    assert np.abs(a["X"] - b["X"]).max() < 1e-5 and np.abs(a["X"] - b["X"]).max() > 0


def test_finish_only_reads_the_state(port):
    case = mc.make("merge")
    scene = mc.new_map(case, port, "cpu")
    mc.add(scene, case, "cpu", slice(0, 2))
    first = scene.finish()
    mc.add(scene, case, "cpu", slice(2, 3))
    whole = scene.finish()
    assert first[2]["kept"] == 480 and whole[2]["kept"] == 720
    assert mc.same_bytes(whole[0], mc.run("merge", port, "cpu")[0][0])
    scene.clear()
    assert mc.counters(scene).tolist() == [0, 0, 0, 0] and scene.finish()[2]["voxels"] == 0


def test_argument_errors_write_nothing(port):
    mc.bad_argument_sweep(port.status, "cpu")
    assert port.lib.map_state_bytes(1024) == 1024 * 48 + 32 and port.lib.map_state_bytes(1000) == -1
    assert port.lib.map_state_bytes(0) == -1 and port.lib.map_finish_scratch_ints(1024) == 4
    assert port.lib.map_finish_scratch_ints(64) == 1 and port.lib.map_finish_scratch_ints(3) == -1


def test_the_binding_checks_before_it_calls(port):
    case = mc.make("merge")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    state = ops.map_state(100, "cpu", port)
    assert state.T == 128 and (state.keys == -1).all() and not state.pos.any() and not state.col.any()
    disp, rgb, poses = t(case["disp"]), t(case["rgb"]), t(case["poses"])
    for kw in (dict(stride=0), dict(voxel=0.0), dict(voxel=float("nan")), dict(min_depth=2.0, max_depth=1.0)):
        with pytest.raises(ValueError, match="map_accumulate"):
            ops.map_accumulate(state, disp, rgb, poses, mc.INV_K, backend=port, **kw)
    for bad in (dict(disp=disp.double()), dict(rgb=rgb[:, :2]), dict(poses=poses.float()), dict(poses=poses[:2])):
        args = dict(disp=disp, rgb=rgb, poses=poses)
        args.update(bad)
        with pytest.raises(ValueError, match="map_accumulate"):
            ops.map_accumulate(state, args["disp"], args["rgb"], args["poses"], mc.INV_K, backend=port)
    with pytest.raises(ValueError, match="min_points"):
        ops.map_finish(state, 0.2, 0, backend=port)
    for capacity in (0, (1 << 30) + 1):
        with pytest.raises(ValueError, match="capacity"):
            ops.map_state(capacity, "cpu", port)
    with pytest.raises(ValueError, match="voxel"):
        pointcloud.SceneMap(0.0, 64, "cpu", port)
    assert pointcloud.SceneMap.DEFAULT_CAPACITY == 1 << 24 and _lib.ABI_VERSION >= 16
    assert not state.pos.any() and int(state.counters.sum()) == 0


def test_hip_backend_refuses_cpu_tensors():
    from baseboostdepth_amd.csrc.build import build
    build()
    with pytest.raises(_lib.BbdError):
        mc.run("merge", ops.HipBackend(), "cpu")
