"""GPU tier of depth-pose consistency (bbd_consist.hip through the C ABI): on every case of tests/consist_checks.py the
device equals the host port and the numpy reference byte for byte - transforms, seen, agree, err, filtered and the
counters - and a second identical call gives the same bytes; the composition with `SceneMap`; and
`evaluate_pose(..., consistency=True, save_map=..., map_consistent=True)` end to end on a synthetic sequence.

No tolerance anywhere: the arithmetic has no transcendental function and is one IEEE operation where written, so a
difference between the device and the port - in a division, say - would be a finding, not noise."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import consist_checks as cc  # noqa: E402
import map_checks as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.mark.parametrize("name", cc.CASES)
def test_device_matches_the_port_and_the_reference(hip, port, name):
    cc.precondition(name)
    got = cc.run(name, hip, DEV)
    assert cc.differing(got, cc.run(name, port, "cpu")) == []                  # byte for byte the host port
    assert cc.differing(got, cc.reference(name)) == []                         # and the numpy reference
    assert cc.differing(got, cc.run(name, hip, DEV)) == []                     # identical calls, identical bytes


def test_the_optional_outputs_are_optional(hip):
    res = cc.call(cc.make("spoilt"), hip, DEV, want_err=False, want_filtered=False)
    want = cc.reference("spoilt")
    assert res.err is None and res.filtered is None
    assert cc.same_bytes(res.seen.cpu().numpy(), want["seen"]) and cc.same_bytes(res.counters.cpu().numpy(), want["counters"])


def test_argument_errors_launch_nothing(hip):
    lib = hip.lib

    def status(name, *args):
        return getattr(lib._dll, name)(*args, None)

    cc.bad_argument_sweep(status, DEV)


def test_scene_map_of_the_filtered_disparities(hip):
    cc.scene_map_composition(hip, DEV, with_state=False)


def test_evaluate_pose_scores_and_filters_on_the_device(hip, port, tmp_path, capsys):
    """The synthetic sequence of tests/test_consist_cli.py through `evaluate_pose` on the device.  The stand-in networks
    run on the device here, so the disparities are the device's; from THOSE disparities and the returned trajectory the
    dict must equal the ops composed by hand on the device and, fed the same numbers, on the CPU tier's host port; the
    written map is the by-hand map of the filtered disparities."""
    from baseboostdepth_amd import evaluation, pointcloud
    path = str(tmp_path / "map.ply")
    opt, pool, gt, loader = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                              save_map=path, map_voxel=0.5, map_stride=1, consistency=True,
                                              map_consistent=True, consistency_threshold=0.2)
    loader = [{k: v.to(DEV) for k, v in batch.items()} for batch in loader]
    out = evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=mc.models(), batch_windows=16, device=DEV)
    said = [line.strip() for line in capsys.readouterr().out.splitlines() if line.strip()]
    disp = cc.sequence_disparities(pool, DEV)
    want, filtered = cc.by_hand(disp, out, hip, threshold=0.2)
    on_port, port_filtered = cc.by_hand(disp.cpu(), out, port, threshold=0.2)
    assert out["consistency"] == want == on_port and cc.same_bytes(filtered.cpu().numpy(), port_filtered.numpy())
    assert 0 < want["kept"] < want["valid"] == mc.SEQ_FRAMES * mc.SEQ_H * mc.SEQ_W and want["visible"] > want["valid"] / 4
    assert said[-2] == cc.consistency_line(want) and said[-1].startswith("Scene map: 12 frames, 2880 candidates")
    second = pointcloud.SceneMap(0.5, 1 << 14, DEV)
    second.add(filtered, pool.to(DEV), torch.from_numpy(out["traj_aligned"]).to(DEV),
               pointcloud.intrinsics(mc.SEQ_H, mc.SEQ_W),
               scale=torch.tensor([out["traj_scale"]], dtype=torch.float64, device=DEV), stride=1, min_depth=0.5,
               max_depth=30.0)
    verts, _, again = second.finish(1)
    got = pointcloud.read_ply(path)
    assert got.size > 20 and got.tobytes() == verts.tobytes()
    assert again == {k: v for k, v in out["map_stats"].items() if k != "frames"} and again["kept"] < again["candidates"]
