"""CPU tier of the picture command lines: `evaluate_pose.py --trajectory --save_plot` end to end through the host ports
(tests/ports.py) on the synthetic 12-frame sequence of tests/map_checks.py, and `test_simple.py --point_cloud
--cloud_view` with a stub predictor.  The written pictures must decode to what the numpy reference (tests/view_ref.py)
draws from the same run's trajectories, voxels and clouds, with a layout worked out here from the documented rules;
without the flags nothing may differ."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_checks as mc  # noqa: E402
import view_checks as vc  # noqa: E402
import view_ref as ref  # noqa: E402
from baseboostdepth_amd import evaluation, inference, ops, pointcloud  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

FRAMES, models, _setup = mc.SEQ_FRAMES, mc.models, mc.setup_sequence
GT, PRED, START, BAR = (40, 40, 40), (214, 39, 40), (31, 119, 180), (0, 0, 0)


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


def _run(opt, loader, gt, port):
    return evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=models(), batch_windows=16, backend=port,
                                    device="cpu")


def _layout(out, plane, size, ceiling):
    """The documented layout, from the returned trajectories: the view, metres per pixel, the bar and its two ends."""
    pred, gt = out["traj_aligned"][:, :3, 3].astype(np.float64), out["traj_gt"][:, :3, 3].astype(np.float64)
    pos = np.concatenate([pred, gt])
    lo, hi = pos.min(0), pos.max(0)
    a, b, c = (0, 2, 1) if plane == "top" else (2, 1, 0)              # along u, along v, depth
    sign = -1.0 if plane == "top" else 1.0
    mpp = max(hi[a] - lo[a], hi[b] - lo[b]) / (0.9 * size)            # a margin of 5 % on every side, one scale
    near = lo[1] - ceiling if plane == "top" else lo[0] - 1000.0
    V = np.zeros((4, 4))
    V[0, a], V[0, 3] = 1 / mpp, size / 2 - (lo[a] + hi[a]) / 2 / mpp
    V[1, b], V[1, 3] = sign / mpp, size / 2 - sign * (lo[b] + hi[b]) / 2 / mpp
    V[2, c], V[2, 3], V[3, 3] = 1.0, -near, 1.0
    bar = ref.scale_bar(size * mpp / 4)
    ends = np.zeros((2, 3))
    x0, y0 = int(0.04 * size) + 0.5, int(0.96 * size) + 0.5         # 4 % in from the lower left, on pixel centres
    for k, px in enumerate((x0, x0 + bar / mpp)):
        ends[k, a] = (lo[a] + hi[a]) / 2 + (px - size / 2) * mpp
        ends[k, b] = (lo[b] + hi[b]) / 2 + sign * (y0 - size / 2) * mpp
        ends[k, c] = pred[0, c]
    return V, mpp, bar, ends, pred, gt


def _reference(out, plane, size, ceiling, voxels=None, point_size=1):
    V, mpp, bar, ends, pred, gt = _layout(out, plane, size, ceiling)
    canvas = ref.Canvas(size, size)
    if voxels is not None:
        canvas.points(voxels, V, size=point_size)
    canvas.lines(gt, V, colour=GT, width=3.0, layer=1)
    canvas.lines(pred, V, colour=PRED, width=2.0, layer=2)
    canvas.lines(gt[:1], V, colour=START, width=9.0, layer=3)
    canvas.lines(ends, V, colour=BAR, width=3.0, layer=3)
    return canvas, mpp, bar


def _accept(picture, stats, want):
    """The decoded picture against the reference canvas, by the rules of `view_checks.accept`."""
    flat = picture.reshape(-1, 3).astype(np.uint64)
    excused = want.all_excused()
    covered = want.cells != ref.EMPTY
    assert [stats[k] for k in ("offered", "drawn", "clipped", "rejected")] == want.counters.tolist()
    assert np.array_equal(flat[~excused], want.image().reshape(-1, 3)[~excused])
    assert int((excused & covered).sum()) <= 0.01 * int(covered.sum())


@pytest.mark.parametrize("plane,size,with_map,flags", [
    ("top", 64, True, dict(map_voxel=0.5, map_stride=1, plot_point_size=3)),
    ("top", 50, False, dict(plot_ceiling=1.5)),
    ("side", 48, True, dict(map_voxel=0.5, map_min_points=2)),
])
def test_the_saved_plot_equals_the_reference(port, tmp_path, capsys, plane, size, with_map, flags):
    path, ply = str(tmp_path / "plot.png"), str(tmp_path / "map.ply")
    opt, pool, gt, loader = _setup(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                   save_map=ply if with_map else None, save_plot=path, plot_view=plane, plot_size=size,
                                   **flags)
    port.calls.clear()
    out = _run(opt, loader, gt, port)
    said = capsys.readouterr().out
    ceiling = flags.get("plot_ceiling", 3.0)
    voxels = pointcloud.read_ply(ply) if with_map else None
    want, mpp, bar = _reference(out, plane, size, ceiling, voxels, flags.get("plot_point_size", 1))
    picture = np.asarray(Image.open(path))
    assert picture.shape == (size, size, 3) and picture.dtype == np.uint8 and Image.open(path).format == "PNG"
    stats = out["plot_stats"]
    _accept(picture, stats, want)
    assert out["plot_path"] == path and stats["view"] == plane and stats["scale_bar"] == bar
    assert stats["m_per_px"] == pytest.approx(mpp, rel=1e-12)
    # all four overlays show, the start disc on top of both trajectories; with a map, voxels lie underneath
    colours = {tuple(c) for c in picture.reshape(-1, 3)}
    assert {GT, PRED, START, BAR, (255, 255, 255)} <= colours and (len(colours) > 5) == with_map
    if with_map:
        assert stats["offered"] == out["map_stats"]["voxels"] == len(voxels) and 0 < stats["drawn"] <= stats["offered"]
        assert port.calls.count("bbd_map_finish") == 2 and port.calls.count("bbd_view_points") == 1
        if plane == "top":                                            # the ceiling clips: the stand-in's ramp goes high
            assert stats["clipped"] > 0
    else:
        assert (stats["offered"], stats["drawn"]) == (0, 0) and "bbd_view_points" not in port.calls
    assert port.calls.count("bbd_view_lines") == 4 and port.calls.count("bbd_view_resolve") == 1
    assert port.calls.count("bbd_view_clear") == 1 and port.calls[-1] == "bbd_view_resolve"
    lines = [l for l in said.splitlines() if l.strip()]
    assert lines[-1].strip() == "Plot: {}, {:.4g} m/px, scale bar {:g} m, {:d} of {:d} voxels -> {}".format(
        plane, stats["m_per_px"], bar, stats["drawn"], stats["offered"], path)
    assert lines[-2].strip().startswith("Scene map:" if with_map else "Full trajectory (")


def test_without_the_flag_nothing_differs(port, tmp_path, capsys):
    opt, pool, gt, loader = _setup(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                   save_map=str(tmp_path / "m.ply"))
    port.calls.clear()
    plain = _run(opt, loader, gt, port)
    said = capsys.readouterr().out
    assert not any(name.startswith("bbd_view_") for name in port.calls)
    assert sorted(plain) == sorted(("ate_mean", "ate_std", "ate_chained_mean", "ate_chained_std", "ates", "pred_poses",
                                    "pred_poses_chained", "t_rel", "r_rel", "traj_ate_rmse", "traj_scale", "per_length",
                                    "traj_aligned", "traj_gt", "map_stats", "map_path"))
    assert "Plot" not in said and said.rstrip().splitlines()[-1].strip().startswith("Scene map: 12 frames")
    before = open(tmp_path / "m.ply", "rb").read()
    flagged, _, _, loader = _setup(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=None,
                                   save_map=str(tmp_path / "m.ply"), save_plot=str(tmp_path / "p.png"), plot_size=32)
    more = _run(flagged, loader, gt, port)
    assert capsys.readouterr().out.startswith(said)
    assert sorted(set(more) - set(plain)) == ["plot_path", "plot_stats"]
    assert open(tmp_path / "m.ply", "rb").read() == before            # the render leaves the map as finish left it
    for k in plain:                                                  # the flag adds, it changes nothing
        if k in ("map_stats", "map_path"):
            assert plain[k] == more[k]
        else:
            assert np.array_equal(np.asarray(plain[k]), np.asarray(more[k]), equal_nan=True), k


def test_save_plot_needs_the_trajectory(port, tmp_path):
    opt, _, gt, loader = _setup(tmp_path, save_plot=str(tmp_path / "p.png"))
    with pytest.raises(ValueError, match="--save_plot needs --trajectory"):
        _run(opt, loader, gt, port)
    assert not os.path.exists(tmp_path / "p.png")
    for bad in (dict(plot_view="front"), dict(plot_size=8), dict(plot_point_size=2), dict(plot_ceiling=0.0),
                dict(plot_ceiling=float("nan"))):
        opt = _setup(tmp_path, trajectory=True, save_plot=str(tmp_path / "p.png"), **bad)[0]
        with pytest.raises(ValueError, match="--plot_"):
            _run(opt, loader, gt, port)


def test_the_scale_bar_is_the_largest_of_1_2_5():
    for metres, want in ((0.99, 0.5), (1.0, 1.0), (1.99, 1.0), (2.0, 2.0), (4.999, 2.0), (5.0, 5.0), (9.99, 5.0),
                         (10.0, 10.0), (137.0, 100.0), (250.0, 200.0), (0.03, 0.02), (7e4, 5e4)):
        assert evaluation.scale_bar_length(metres) == pytest.approx(want, rel=1e-12) == pytest.approx(ref.scale_bar(metres))


def test_options_parse_the_plot_flags():
    o = MonodepthOptions().parse([])
    assert (o.save_plot, o.plot_view, o.plot_size, o.plot_ceiling, o.plot_point_size) == (None, "top", 1024, 3.0, 1)
    o = MonodepthOptions().parse(["--trajectory", "--save_plot", "p.png", "--plot_view", "side", "--plot_size", "512",
                                  "--plot_ceiling", "2.5", "--plot_point_size", "3"])
    assert (o.save_plot, o.plot_view, o.plot_size, o.plot_ceiling, o.plot_point_size) == ("p.png", "side", 512, 2.5, 3)
    for bad in (["--plot_view", "front"], ["--plot_point_size", "2"]):
        with pytest.raises(SystemExit):
            MonodepthOptions().parse(bad)


# ---------------------------------------------------------------------------------------------- test_simple.py
class StubPredictor:
    """`predict` as tests/test_cloud_cli.py's stub; `predict_cloud` exports a made-up disparity of every image through
    `ops.point_cloud` on the host port and, with `view=`, draws it through `inference.cloud_views` as the product does."""

    def __init__(self, port):
        self.port, self.cloud_calls = port, []

    def predict(self, images, want_float=False, post_process=False):
        return [inference.DepthPrediction(np.zeros(im.shape, np.uint8), 1.0, 2.0, None) for im in images]

    def predict_cloud(self, images, inv_K=None, scale=1.0, max_depth=None, stride=1, post_process=False, **view):
        self.cloud_calls.append(dict(view))
        sizes = [im.shape[:2] for im in images]
        yy, xx = np.meshgrid(np.linspace(0, 1, 6), np.linspace(0, 1, 8), indexing="ij")
        depth = 4.0 + 6.0 * yy * (1 - yy) + 3.0 * np.abs(xx - 0.4)                    # a bent wall, 4 .. 7.3
        disp = torch.from_numpy((1.0 / depth).astype(np.float32))[None].repeat(len(images), 1, 1)
        rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images]))
        cloud = ops.point_cloud(disp, ops.cloud_rows(sizes), inv_K, rgb=rgb, stride=stride, min_depth=0.0, max_depth=1e6,
                                pred_is_disp=True, scale_factor=scale, backend=self.port)
        clouds = pointcloud.cloud_arrays(*cloud)
        if not view:
            return clouds
        return clouds, inference.cloud_views(cloud, clouds, sizes, inv_K, view["view"], view["view_size"], self.port)


def _argv(src, dst, *extra):
    return ["--image_path", str(src), "--save_path", str(dst), "--ext", "png", "--weights", "w"] + list(extra)


def _write(path, h, w, seed):
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


@pytest.mark.parametrize("extra,yaw,pitch,size", [((), 15.0, -10.0, 3), (("--cloud_view_size", "1"), -30.0, 5.0, 1)])
def test_cloud_view_writes_the_orbited_picture(tmp_path, port, extra, yaw, pitch, size):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _write(src / "a.png", 37, 91, 1)
    _write(src / "b.png", 50, 64, 2)
    stub = StubPredictor(port)
    args = inference.parse_args(_argv(src, dst, "--point_cloud", "--cloud_view", str(yaw), str(pitch), *extra))
    inference.run_cli(args, predictor=stub)
    assert stub.cloud_calls == [dict(view=(yaw, pitch), view_size=size)]
    assert sorted(os.listdir(dst)) == ["a_Base.jpg", "a_Base.ply", "a_Base_view.png", "b_Base.jpg", "b_Base.ply",
                                       "b_Base_view.png"]
    for name, (h, w) in (("a", (37, 91)), ("b", (50, 64))):
        cloud = pointcloud.read_ply(str(dst / (name + "_Base.ply")))
        picture = np.asarray(Image.open(dst / (name + "_Base_view.png")))
        assert picture.shape == (h, w, 3) and len(cloud) == h * w
        K = np.linalg.inv(pointcloud.intrinsics(h, w).astype(np.float64))
        V = pointcloud.orbit_view(K, yaw, pitch, float(np.median(cloud["z"].astype(np.float64))))
        want = ref.Canvas(h, w)
        want.points(cloud, V, size=size)
        assert want.counters[0] == h * w and 0.5 * h * w < want.counters[1] and want.counters[3] == 0
        excused, covered = want.all_excused(), want.cells != ref.EMPTY
        flat = picture.reshape(-1, 3)
        assert np.array_equal(flat[~excused], want.image().reshape(-1, 3)[~excused])
        assert int((excused & covered).sum()) <= 0.01 * int(covered.sum())
        # turned, the picture is no longer the image: part of the canvas is bare, part of the cloud hidden
        assert 0.3 * h * w < int(covered.sum()) < h * w


def test_without_cloud_view_the_predictor_is_called_as_before(tmp_path, port):
    src = tmp_path / "in"
    src.mkdir()
    _write(src / "a.png", 20, 30, 3)
    stub = StubPredictor(port)
    inference.run_cli(inference.parse_args(_argv(src, tmp_path / "o", "--point_cloud")), predictor=stub)
    assert stub.cloud_calls == [{}] and sorted(os.listdir(tmp_path / "o")) == ["a_Base.jpg", "a_Base.ply"]
    a = inference.parse_args(_argv("x", "y"))
    assert (a.cloud_view, a.cloud_view_size) == (None, 3)
    for bad in (["--cloud_view", "10", "5"], ["--point_cloud", "--cloud_view", "10"],
                ["--point_cloud", "--cloud_view", "1", "2", "--cloud_view_size", "4"]):
        with pytest.raises(SystemExit):
            inference.parse_args(_argv("x", "y", *bad))
