"""GPU tier of the scene map (bbd_map.hip through the C ABI): the cases and checks of tests/map_checks.py, byte equality
with the host port on every case - vertices, counts, statistics and the four counters - identical bytes from identical
calls, and `evaluate_pose(..., save_map=)` end to end on a synthetic sequence."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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


@pytest.fixture(scope="module")
def port_results(port):
    """The host port's answer to every case, computed once."""
    return {name: mc.run(name, port, "cpu") for name in mc.CASES}


_DEVICE = {}


def device_run(hip, name):
    """The device's answer to a case, computed once."""
    if name not in _DEVICE:
        _DEVICE[name] = mc.run(name, hip, DEV)
    return _DEVICE[name]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_device_matches_the_reference_and_the_port(hip, port, port_results, name):
    out, counters = device_run(hip, name)
    if name in mc.RAISES:
        assert isinstance(out, RuntimeError) and re.search(mc.RAISES[name], str(out)), out
    else:
        assert not isinstance(out, RuntimeError), out
    mc.check(name, out, counters, port)
    assert mc.same_result((out, counters), port_results[name])                       # byte for byte the host port
    if name != "overflow":                                                            # the full table runs once
        assert mc.same_result((out, counters), mc.run(name, hip, DEV))                # identical calls, identical bytes


@pytest.mark.parametrize("name", ["merge", "scaled", "far", "bad_disp"])
def test_one_call_of_three_frames_equals_three_calls_of_one(hip, name):
    assert mc.same_result(device_run(hip, name), mc.run(name, hip, DEV, split=True))


@pytest.mark.parametrize("name", sorted(set(mc.CASES) - {"overflow"}))
def test_the_plain_form_gives_the_same_bytes(hip, name):
    """BBD_MAP_NO_MERGE - every point adds for itself - against the default, which sums runs of equal keys in the wave."""
    assert mc.same_result(device_run(hip, name), mc.run(name, hip, DEV, merge=False))


def test_overflow_is_counted_and_the_call_returns(hip):
    """The error path of the bounded probe loop: 240 distinct voxels for 64 slots.  Run once."""
    out, counters = device_run(hip, "overflow")
    assert counters.tolist() == [240, 64, 0, 176]
    assert "64 slots" in str(out) and "--map_capacity" in str(out)


def test_finish_only_reads_the_state(hip, port_results):
    case = mc.make("merge")
    scene = mc.new_map(case, hip, DEV)
    mc.add(scene, case, DEV, slice(0, 2))
    first = scene.finish()
    mc.add(scene, case, DEV, slice(2, 3))
    whole = scene.finish()
    assert first[2]["kept"] == 480 and whole[2]["kept"] == 720
    assert mc.same_bytes(whole[0], port_results["merge"][0][0])
    scene.clear()
    assert mc.counters(scene).tolist() == [0, 0, 0, 0] and scene.finish()[2]["voxels"] == 0


def test_argument_errors_launch_nothing(hip):
    lib = hip.lib

    def status(name, *args):
        return getattr(lib._dll, name)(*args, None)

    mc.bad_argument_sweep(status, DEV)
    assert lib.map_state_bytes(1024) == 1024 * 48 + 32 and lib.map_state_bytes(1000) == -1
    assert lib.map_finish_scratch_ints(1024) == 4 and lib.map_finish_scratch_ints(3) == -1


def test_evaluate_pose_saves_the_map_on_the_device(hip, tmp_path, capsys):
    """The synthetic sequence of tests/test_map_cli.py through `evaluate_pose` on the device: the file parses, holds
    `map_stats["voxels"]` vertices and equals what a second SceneMap fed the same device tensors produces."""
    from baseboostdepth_amd import evaluation, pointcloud
    path = str(tmp_path / "map.ply")
    opt, pool, gt, loader = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                              save_map=path, map_voxel=0.5, map_stride=1, map_min_points=2)
    loader = [{k: v.to(DEV) for k, v in batch.items()} for batch in loader]
    out = evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=mc.models(), batch_windows=16, device=DEV)
    said = capsys.readouterr().out
    got = pointcloud.read_ply(path)
    stats = out["map_stats"]
    assert out["map_path"] == path and got.size == stats["voxels"] > 20 and stats["frames"] == mc.SEQ_FRAMES
    assert stats["candidates"] == mc.SEQ_FRAMES * mc.SEQ_H * mc.SEQ_W and 0 < stats["kept"] <= stats["candidates"]
    assert stats["dropped_full"] == 0 and "Scene map: 12 frames, 2880 candidates" in said.rstrip().splitlines()[-1]
    frames = pool.to(DEV)
    with torch.no_grad():
        disp = 1.0 / 100.0 + (1.0 / 0.1 - 1.0 / 100.0) * mc.RampDepthDecoder()(mc.PassEncoder()(frames))[("disp", 0)]
    second = pointcloud.SceneMap(0.5, 1 << 14, DEV)
    second.add(disp, frames, torch.from_numpy(out["traj_aligned"]).to(DEV), pointcloud.intrinsics(mc.SEQ_H, mc.SEQ_W),
               scale=torch.tensor([out["traj_scale"]], dtype=torch.float64, device=DEV), stride=1, min_depth=0.5,
               max_depth=30.0)
    verts, counts, again = second.finish(2)
    assert got.tobytes() == verts.tobytes() and again == {k: v for k, v in stats.items() if k != "frames"}
    assert int(counts.min()) >= 2
