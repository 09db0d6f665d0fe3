"""CPU tier of `evaluate_pose.py --trajectory --consistency` and `--save_map ... --map_consistent`:
`evaluation.evaluate_pose` end to end through the host ports (tests/ports.py) on the synthetic 12-frame sequence of
tests/map_checks.py.  The printed line and the `consistency` dict must equal a by-hand composition of the ops, the
written map the by-hand map of the filtered disparities; without the flags nothing may differ."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import consist_checks as cc  # noqa: E402
import map_checks as mc  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import evaluation, pointcloud  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

H, W, FRAMES = mc.SEQ_H, mc.SEQ_W, mc.SEQ_FRAMES
PLAIN_KEYS = ("ate_mean", "ate_std", "ate_chained_mean", "ate_chained_std", "ates", "pred_poses", "pred_poses_chained",
              "t_rel", "r_rel", "traj_ate_rmse", "traj_scale", "per_length", "traj_aligned", "traj_gt")


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def _run(opt, loader, gt, port):
    return evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=mc.models(), batch_windows=16, backend=port,
                                    device="cpu")


def _lines(said):
    return [line.strip() for line in said.splitlines() if line.strip()]


@pytest.mark.parametrize("flags,kw", [
    (dict(), dict()),                                                                                # the defaults
    (dict(consistency_views=2, consistency_threshold=0.02, consistency_min_views=2, map_every=2),
     dict(views=2, threshold=0.02, min_views=2, every=2)),
])
def test_the_line_and_the_dict_equal_the_ops_composed_by_hand(port, tmp_path, capsys, flags, kw):
    opt, pool, gt, loader = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                              consistency=True, **flags)
    port.calls.clear()
    out = _run(opt, loader, gt, port)
    said = _lines(capsys.readouterr().out)
    assert port.calls.count("bbd_depth_consistency") == 1 and not any(c.startswith("bbd_map_") for c in port.calls)
    want, _ = cc.by_hand(cc.sequence_disparities(pool, "cpu"), out, port, **kw)
    assert out["consistency"] == want and sorted(set(out) - set(PLAIN_KEYS)) == ["consistency"]
    # the synthetic networks do not agree with one another, but the measure must have had something to measure
    assert want["valid"] == want["frames"] * H * W and want["visible"] > want["valid"] / 4
    assert 0 <= want["consistent"] <= want["visible"] and 0.0 <= want["mean_err"] <= 1.0
    assert said[-2].startswith("Full trajectory (sim3, 12 frames)") and said[-1] == cc.consistency_line(want)


def test_chunks_carry_their_neighbours(port, tmp_path, monkeypatch):
    """Frames in chunks of 5 and of 1, each with its neighbours, against one call over all twelve."""
    opt, pool, gt, loader = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                              consistency=True, consistency_views=2)
    whole = _run(opt, loader, gt, port)["consistency"]
    for chunk, calls in ((5, 3), (1, 12)):
        monkeypatch.setattr(evaluation, "CONSISTENCY_CHUNK", chunk)
        port.calls.clear()
        assert _run(opt, loader, gt, port)["consistency"] == whole
        assert port.calls.count("bbd_depth_consistency") == calls


def test_the_consistent_map_is_the_map_of_the_filtered_disparities(port, tmp_path, capsys):
    path, plain_path = str(tmp_path / "map.ply"), str(tmp_path / "plain.ply")
    flags = dict(trajectory=True, trajectory_align="sim3", save_trajectory=None, map_voxel=0.5, map_stride=1,
                 consistency_threshold=0.2)
    opt, pool, gt, loader = mc.setup_sequence(tmp_path, save_map=path, map_consistent=True, **flags)
    port.calls.clear()
    out = _run(opt, loader, gt, port)
    said = _lines(capsys.readouterr().out)
    assert port.calls.count("bbd_depth_consistency") == 1 and port.calls.count("bbd_map_accumulate") == 1
    want, filtered = cc.by_hand(cc.sequence_disparities(pool, "cpu"), out, port, threshold=0.2)
    assert out["consistency"] == want and 0 < want["kept"] < want["valid"]
    scene = pointcloud.SceneMap(0.5, 1 << 14, "cpu", port)
    scene.add(filtered, pool, torch.from_numpy(out["traj_aligned"]), pointcloud.intrinsics(H, W),
              scale=torch.tensor([out["traj_scale"]], dtype=torch.float64), stride=1, min_depth=0.5, max_depth=30.0)
    verts, _, stats = scene.finish(1)
    got = pointcloud.read_ply(path)
    assert got.size > 20 and got.tobytes() == verts.tobytes() and out["map_stats"] == dict(stats, frames=FRAMES)
    assert said[-3].startswith("Full trajectory (") and said[-2] == cc.consistency_line(want)
    assert said[-1].startswith("Scene map: 12 frames, 2880 candidates, %d kept" % stats["kept"])
    # against the map without the filter: what the filter takes away is rejected like every disparity without a finite
    # depth, so `kept` falls and no drop count moves (the map counts out-of-range drops only past its depth test)
    opt = mc.setup_sequence(tmp_path, save_map=plain_path, **flags)[0]
    plain = _run(opt, loader, gt, port)
    assert "consistency" not in plain
    assert out["map_stats"]["kept"] < plain["map_stats"]["kept"] and got.size < pointcloud.read_ply(plain_path).size
    for k in ("candidates", "dropped_range", "dropped_full"):
        assert out["map_stats"][k] == plain["map_stats"][k]
    # --consistency next to a plain --save_map scores, and leaves the map alone
    opt = mc.setup_sequence(tmp_path, save_map=path, consistency=True, **flags)[0]
    both = _run(opt, loader, gt, port)
    assert both["consistency"] == want and both["map_stats"] == plain["map_stats"]
    assert pointcloud.read_ply(path).tobytes() == pointcloud.read_ply(plain_path).tobytes()


def test_without_the_flags_nothing_differs(port, tmp_path, capsys):
    opt, _, gt, loader = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None)
    port.calls.clear()
    plain = _run(opt, loader, gt, port)
    said = capsys.readouterr().out
    assert "bbd_depth_consistency" not in port.calls and sorted(plain) == sorted(PLAIN_KEYS) and "consistency" not in said
    flagged = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None, consistency=True)[0]
    more = _run(flagged, loader, gt, port)
    assert capsys.readouterr().out.startswith(said)
    for k in plain:                                        # the flag adds, it changes nothing
        assert np.array_equal(np.asarray(plain[k]), np.asarray(more[k]), equal_nan=True), k


def test_the_flags_need_what_they_build_on(port, tmp_path):
    for flags, said in ((dict(consistency=True), "--consistency needs --trajectory"),
                        (dict(map_consistent=True), "--map_consistent needs --save_map"),
                        (dict(trajectory=True, map_consistent=True), "--map_consistent needs --save_map"),
                        (dict(map_consistent=True, save_map=str(tmp_path / "m.ply")), "--save_map needs --trajectory"),
                        (dict(trajectory=True, consistency=True, consistency_views=0), "--consistency_views"),
                        (dict(trajectory=True, consistency=True, consistency_views=5), "--consistency_views"),
                        (dict(trajectory=True, consistency=True, consistency_threshold=-0.1), "--consistency_threshold"),
                        (dict(trajectory=True, consistency=True, consistency_min_views=-1), "--consistency_min_views"),
                        (dict(trajectory=True, consistency=True, map_every=0), "--map_every")):
        opt, _, gt, loader = mc.setup_sequence(tmp_path, **flags)
        port.calls.clear()
        with pytest.raises(ValueError, match=said):
            _run(opt, loader, gt, port)
        assert port.calls == [] and not os.path.exists(tmp_path / "m.ply")


def test_options_parse_the_consistency_flags():
    o = MonodepthOptions().parse([])
    assert (o.consistency, o.consistency_views, o.consistency_threshold, o.consistency_min_views, o.map_consistent) == (
        False, 1, 0.05, 1, False)
    o = MonodepthOptions().parse(["--trajectory", "--consistency", "--consistency_views", "2", "--consistency_threshold",
                                  "0.01", "--consistency_min_views", "3", "--save_map", "m.ply", "--map_consistent"])
    assert (o.consistency, o.consistency_views, o.consistency_threshold, o.consistency_min_views, o.map_consistent) == (
        True, 2, 0.01, 3, True)
    assert evaluation.consistency_offsets(1) == (-1, 1) and evaluation.consistency_offsets(3) == (-1, 1, -2, 2, -3, 3)
