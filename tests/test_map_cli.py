"""CPU tier of `evaluate_pose.py --trajectory --save_map`: `evaluation.evaluate_pose` end to end through the host ports
(tests/ports.py) on a synthetic 12-frame sequence with injected stand-ins for the pose and depth networks and
ground-truth poses.  The written file must equal the numpy reference (tests/map_ref.py) computed from the same
disparities and the returned aligned trajectory; without the flag nothing may differ."""
import os
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
from baseboostdepth_amd import evaluation, pointcloud  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

H, W, FRAMES, models, _setup = mc.SEQ_H, mc.SEQ_W, mc.SEQ_FRAMES, mc.models, mc.setup_sequence
RampDepthDecoder, PassEncoder = mc.RampDepthDecoder, mc.PassEncoder


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def _run(opt, loader, gt, port):
    return evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=models(), batch_windows=16, backend=port,
                                    device="cpu")


def _reference(pool, out, every, **kw):
    """The numpy reference's map from the stand-in's disparities, the returned aligned trajectory and scale."""
    with torch.no_grad():
        disp = RampDepthDecoder()(PassEncoder()(pool))[("disp", 0)][:, 0]
        scaled = (1.0 / 100.0 + (1.0 / 0.1 - 1.0 / 100.0) * disp).numpy()
    rows = slice(0, FRAMES, every)
    return ref.scene(scaled[rows], pool.numpy()[rows], out["traj_aligned"][rows], pointcloud.intrinsics(H, W),
                     scale=out["traj_scale"], **kw)


@pytest.mark.parametrize("align,flags,kw", [
    ("sim3", dict(), dict(voxel=0.2, stride=2, min_depth=0.5, max_depth=30.0)),                     # the defaults
    ("se3", dict(map_voxel=0.5, map_every=2, map_stride=1, map_min_depth=2.0, map_max_depth=4.5, map_min_points=2,
                 map_capacity=1000),
     dict(voxel=0.5, stride=1, min_depth=2.0, max_depth=4.5, min_points=2)),
])
def test_the_saved_map_equals_the_reference(port, tmp_path, capsys, align, flags, kw):
    path = str(tmp_path / "map.ply")
    opt, pool, gt, loader = _setup(tmp_path, trajectory=True, trajectory_align=align, save_trajectory=None, save_map=path,
                                   **flags)
    port.calls.clear()
    out = _run(opt, loader, gt, port)
    said = capsys.readouterr().out
    every = flags.get("map_every", 1)
    frames = len(range(0, FRAMES, every))
    assert port.calls.count("bbd_map_accumulate") == 1 and port.calls.count("bbd_map_finish") == 1     # one batch
    assert port.calls.count("bbd_pose_trajectory") == 1
    assert (out["traj_scale"] == 1.0) == (align == "se3") and np.isfinite(out["traj_scale"])
    want_v, want_c, want_stats = _reference(pool, out, every, **kw)
    got = pointcloud.read_ply(path)
    assert out["map_path"] == path and got.size > 20
    assert got.dtype == pointcloud.VERTEX_DTYPE and got.tobytes() == want_v.astype(pointcloud.VERTEX_DTYPE).tobytes()
    assert out["map_stats"] == dict(want_stats, frames=frames) and out["map_stats"]["voxels"] == got.size
    assert want_stats["candidates"] == frames * len(ref.grid(H, W, None, kw["stride"])[0])
    if flags:                                    # limits that reject some points, voxels in which points of a frame meet
        assert got.size < want_stats["kept"] < want_stats["candidates"] and want_c.max() >= 5
        assert got.size < _reference(pool, out, every, **dict(kw, min_points=1))[0].size           # --map_min_points
    lines = [l for l in said.splitlines() if l.strip()]
    assert lines[-2].strip().startswith("Full trajectory (")
    assert lines[-1].strip() == "Scene map: {:d} frames, {:d} candidates, {:d} kept, {:d} voxels -> {}".format(
        frames, want_stats["candidates"], want_stats["kept"], got.size, path)


def test_without_the_flag_nothing_differs(port, tmp_path, capsys):
    opt, pool, gt, loader = _setup(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None)
    port.calls.clear()
    plain = _run(opt, loader, gt, port)
    said = capsys.readouterr().out
    assert not any(name.startswith("bbd_map_") for name in port.calls)
    assert sorted(plain) == sorted(("ate_mean", "ate_std", "ate_chained_mean", "ate_chained_std", "ates", "pred_poses",
                                    "pred_poses_chained", "t_rel", "r_rel", "traj_ate_rmse", "traj_scale", "per_length",
                                    "traj_aligned", "traj_gt"))
    assert "Scene map" not in said and said.rstrip().splitlines()[-1].strip().startswith("Full trajectory (sim3, 12 frames)")
    # a two-model injection still means the pose pair
    pair = evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=models()[:2], batch_windows=16, backend=port,
                                    device="cpu")
    assert capsys.readouterr().out == said
    assert all(np.array_equal(np.asarray(plain[k]), np.asarray(pair[k]), equal_nan=True) for k in plain)
    flagged, _, _, loader = _setup(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                   save_map=str(tmp_path / "m.ply"))
    more = _run(flagged, loader, gt, port)
    assert capsys.readouterr().out.startswith(said)
    assert sorted(set(more) - set(plain)) == ["map_path", "map_stats"]
    for k in plain:                                        # the flag adds, it changes nothing
        assert np.array_equal(np.asarray(plain[k]), np.asarray(more[k]), equal_nan=True), k


def test_save_map_needs_the_trajectory(port, tmp_path):
    opt, _, gt, loader = _setup(tmp_path, save_map=str(tmp_path / "m.ply"))
    with pytest.raises(ValueError, match="--save_map needs --trajectory"):
        _run(opt, loader, gt, port)
    assert not os.path.exists(tmp_path / "m.ply")
    for bad in (dict(map_voxel=0.0), dict(map_every=0), dict(map_stride=0), dict(map_min_points=0), dict(map_capacity=0),
                dict(map_min_depth=5.0, map_max_depth=1.0)):
        opt = _setup(tmp_path, trajectory=True, save_map=str(tmp_path / "m.ply"), **bad)[0]
        with pytest.raises(ValueError, match="--map_"):
            _run(opt, loader, gt, port)


def test_a_table_that_is_too_small_names_the_flag(port, tmp_path):
    opt, _, gt, loader = _setup(tmp_path, trajectory=True, trajectory_align="sim3", save_map=str(tmp_path / "m.ply"),
                                map_voxel=1e-3, map_capacity=64)
    with pytest.raises(RuntimeError, match=r"64 slots is full.*--map_capacity"):
        _run(opt, loader, gt, port)
    assert not os.path.exists(tmp_path / "m.ply")


def test_options_parse_the_map_flags():
    o = MonodepthOptions().parse([])
    assert (o.save_map, o.map_voxel, o.map_every, o.map_stride, o.map_min_depth, o.map_max_depth, o.map_min_points,
            o.map_capacity) == (None, 0.2, 1, 2, 0.5, 30.0, 1, 1 << 24)
    o = MonodepthOptions().parse(["--trajectory", "--save_map", "m.ply", "--map_voxel", "0.1", "--map_every", "5",
                                  "--map_stride", "3", "--map_min_depth", "1", "--map_max_depth", "50",
                                  "--map_min_points", "2", "--map_capacity", "1000000"])
    assert (o.save_map, o.map_voxel, o.map_every, o.map_stride, o.map_min_depth, o.map_max_depth, o.map_min_points,
            o.map_capacity) == ("m.ply", 0.1, 5, 3, 1.0, 50.0, 2, 1000000)
