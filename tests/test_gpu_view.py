"""GPU tier of the view rasteriser (bbd_view.hip through the C ABI): every case of tests/view_checks.py byte for byte
against the host port - cells, counters and picture - identical bytes from identical calls and from every order and
split of the same primitives, the reference's acceptance on the device's own answer, the argument rules, and
`evaluate_pose(..., save_plot=)` end to end on a synthetic sequence."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import view_checks as vc  # noqa: E402

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


def _bg(name):
    return vc.BACKGROUNDS.get(name, (255, 255, 255))


@pytest.fixture(scope="module")
def port_results(port):
    """The host port's answer to every case, computed once."""
    return {name: vc.run(steps, port, "cpu", _bg(name)) for name, steps in vc.CASES.items()}


_DEVICE = {}


def device_run(hip, name):
    """The device's answer to a case, computed once."""
    if name not in _DEVICE:
        _DEVICE[name] = vc.run(vc.CASES[name], hip, DEV, _bg(name))
    return _DEVICE[name]


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_device_matches_the_port_and_the_reference(hip, port_results, name):
    got = device_run(hip, name)
    assert vc.same(got, port_results[name])                                      # byte for byte the host port
    assert vc.same(got, vc.run(vc.CASES[name], hip, DEV, _bg(name)))             # identical calls, identical bytes
    vc.accept(name, got, vc.reference(vc.CASES[name]), _bg(name))


@pytest.mark.parametrize("name", ["layers", "mixed", "zfight3", "persp5", "tie"])
def test_the_order_of_submission_does_not_matter(hip, name):
    first = device_run(hip, name)
    for steps in vc.orders(vc.CASES[name]):
        assert vc.same(first, vc.run(steps, hip, DEV, _bg(name)))


def test_a_view_on_the_device_is_taken_as_it_is(hip):
    """Views and polylines that are already device tensors (as `evaluate_pose` passes them) give the same bytes."""
    from baseboostdepth_amd import pointcloud
    canvas = pointcloud.Canvas(vc.W, vc.H, DEV, hip)
    view = torch.from_numpy(vc.PLAIN).to(DEV)
    canvas.lines(torch.from_numpy(vc.polyline()).to(DEV), view=view, width=5.0, colour=(31, 119, 180))
    cells = canvas.state.cells.cpu().numpy().view(np.uint64).reshape(-1)
    assert np.array_equal(cells, device_run(hip, "lines5")[0])
    canvas.clear()
    assert (canvas.state.cells == -1).all() and canvas.stats() == dict(offered=0, drawn=0, clipped=0, rejected=0)


def test_hip_backend_refuses_cpu_tensors(hip):
    from baseboostdepth_amd import _lib, ops, pointcloud
    with pytest.raises(_lib.BbdError, match="no CPU path"):
        pointcloud.Canvas(vc.W, vc.H, "cpu", hip)
    state = ops.view_state(vc.H, vc.W, DEV, hip)
    with pytest.raises(ValueError, match="view_points"):
        ops.view_points(state, torch.zeros(32, dtype=torch.uint8), vc.TOP, backend=hip)
    host = ops.ViewState(state.cells.cpu(), state.counters.cpu(), vc.H, vc.W)
    with pytest.raises(_lib.BbdError, match="no CPU path"):
        ops.view_resolve(host, backend=hip)


def test_argument_errors_launch_nothing(hip):
    lib = hip.lib

    def status(name, *args):
        return getattr(lib._dll, name)(*args, None)

    vc.bad_argument_sweep(status, DEV)


def test_evaluate_pose_saves_the_plot_on_the_device(hip, port, tmp_path, capsys):
    """The synthetic sequence of tests/test_view_cli.py through `evaluate_pose` on the device, with the map underneath:
    the picture equals what the host port draws from the same run's trajectories and finished voxels."""
    import map_checks as mc
    from PIL import Image
    from baseboostdepth_amd import evaluation, pointcloud
    path, ply = str(tmp_path / "plot.png"), str(tmp_path / "map.ply")
    opt, pool, gt, loader = mc.setup_sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                              save_map=ply, map_voxel=0.5, map_stride=1, save_plot=path, plot_size=96,
                                              plot_point_size=3)
    loader = [{k: v.to(DEV) for k, v in batch.items()} for batch in loader]
    out = evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=mc.models(), batch_windows=16, device=DEV)
    said = capsys.readouterr().out.rstrip().splitlines()[-1]
    stats = out["plot_stats"]
    assert out["plot_path"] == path and said.strip().startswith("Plot: top, ") and said.strip().endswith("-> " + path)
    assert stats["offered"] == out["map_stats"]["voxels"] and 0 < stats["drawn"] <= stats["offered"]
    both = np.stack([out["traj_aligned"], out["traj_gt"]])
    view, mpp, bar, ends = evaluation.plot_layout(both, dict(view="top", size=96, ceiling=3.0))
    canvas = pointcloud.Canvas(96, 96, "cpu", port)
    voxels = torch.from_numpy(pointcloud.read_ply(ply).view(np.uint8).copy())
    canvas.points(voxels, view=view, size=3)
    canvas.lines(both[1][:, :3, 3], view=view, colour=evaluation.PLOT_GT, width=3.0, layer=1)
    canvas.lines(both[0][:, :3, 3], view=view, colour=evaluation.PLOT_PRED, width=2.0, layer=2)
    canvas.lines(both[1][:1, :3, 3], view=view, colour=evaluation.PLOT_START, width=9.0, layer=3)
    canvas.lines(ends, view=view, colour=evaluation.PLOT_BAR, width=3.0, layer=3)
    want, want_stats = canvas.read()
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), want)
    assert {k: stats[k] for k in want_stats} == want_stats and (stats["m_per_px"], stats["scale_bar"]) == (mpp, bar)
