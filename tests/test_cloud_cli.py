"""CPU tier of the point-cloud command lines: PLY files, intrinsics, `test_simple.py --point_cloud` with a stub predictor
and `evaluate_depth.py --save_clouds` on synthetic KITTI and SYNS splits, the kernels replaced by their host ports
(tests/ports.py)."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import syns_checks  # noqa: E402
from baseboostdepth_amd import evaluation, inference, ops, pointcloud  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

HEADER = """ply
format binary_little_endian 1.0
comment baseboostdepth_amd point cloud
element vertex %d
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
property uchar alpha
end_header
"""


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


# ---------------------------------------------------------------------------------------------- files and intrinsics
def _some_cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    arr = np.zeros(n, pointcloud.VERTEX_DTYPE)
    for f in "xyz":
        arr[f] = rng.standard_normal(n).astype(np.float32)
    for f in ("red", "green", "blue"):
        arr[f] = rng.integers(0, 256, n)
    arr["alpha"] = 255
    return arr


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_ply_round_trip_and_exact_header(tmp_path, n):
    arr = _some_cloud(n)
    path = pointcloud.write_ply(str(tmp_path / "c.ply"), arr)
    data = open(path, "rb").read()
    assert data == (HEADER % n).encode("ascii") + arr.tobytes()          # the bytes as they are, little-endian
    back = pointcloud.read_ply(path)
    assert back.dtype == pointcloud.VERTEX_DTYPE and np.array_equal(back.view(np.uint8), arr.view(np.uint8))
    assert [name for name in back.dtype.names] == ["x", "y", "z", "red", "green", "blue", "alpha"]
    assert back.dtype["x"] == np.dtype("<f4") and back.dtype["alpha"] == np.dtype("u1") and back.dtype.itemsize == 16


def test_read_ply_refuses_other_layouts(tmp_path):
    ascii_ply = ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                 "end_header\n0 0 0\n")
    (tmp_path / "a.ply").write_text(ascii_ply)
    with pytest.raises(ValueError, match="ascii"):
        pointcloud.read_ply(str(tmp_path / "a.ply"))
    (tmp_path / "b.ply").write_bytes((HEADER % 2).replace("little", "big").encode() + bytes(32))
    (tmp_path / "c.ply").write_bytes((HEADER % 2).replace("property uchar alpha\n", "").encode() + bytes(30))
    (tmp_path / "d.ply").write_bytes((HEADER % 2).encode() + bytes(31))                  # truncated
    (tmp_path / "e.ply").write_bytes(b"not a ply at all")
    for name in "bcde":
        with pytest.raises(ValueError):
            pointcloud.read_ply(str(tmp_path / (name + ".ply")))
    with pytest.raises(ValueError):
        pointcloud.write_ply(str(tmp_path / "f.ply"), np.zeros((3, 4), np.float32))


def test_intrinsics():
    K = pointcloud.camera_matrix(375, 1242)
    assert K.dtype == np.float32 and K.shape == (4, 4)
    assert K[0, 0] == np.float32(0.58) * np.float32(1242) and K[1, 1] == np.float32(1.92) * np.float32(375)
    assert K[0, 2] == 621 and K[1, 2] == 187.5
    from baseboostdepth_amd import datasets
    ds = datasets.KITTIDataset.__new__(datasets.KITTIDataset)
    ds.width, ds.height = 1242, 375
    want_K, want_inv = ds.load_intrinsic_kt(0)
    assert np.array_equal(K, want_K)
    inv = pointcloud.intrinsics(375, 1242)
    assert inv.dtype == np.float32 and inv.shape == (3, 3) and inv.flags["C_CONTIGUOUS"]
    assert np.array_equal(inv, want_inv[:3, :3].astype(np.float32))
    assert np.array_equal(inv, np.linalg.pinv(K)[:3, :3].astype(np.float32))
    np.testing.assert_allclose(1.0 / inv[0, 0], 0.58 * 1242, rtol=1e-6)
    np.testing.assert_allclose(1.0 / inv[1, 1], 1.92 * 375, rtol=1e-6)
    F = pointcloud.camera_matrix(60, 100, fov=90)
    assert F[0, 0] == F[1, 1] == np.float32(50.0 / np.tan(np.deg2rad(90.0) / 2)) and F[0, 2] == 50 and F[1, 2] == 30
    np.testing.assert_allclose(F[0, 0], 50.0, rtol=1e-6)
    np.testing.assert_allclose(1.0 / pointcloud.intrinsics(60, 100, fov=90)[0, 0], 50.0, rtol=1e-6)
    G = pointcloud.camera_matrix(60, 100, fxfycxcy=(70, 80, 49, 31))
    assert (G[0, 0], G[1, 1], G[0, 2], G[1, 2]) == (70, 80, 49, 31)
    given = np.array([[9, 0, 4], [0, 8, 3], [0, 0, 1]], np.float32)
    assert np.array_equal(pointcloud.camera_matrix(6, 8, K=given)[:3, :3], given)
    for bad in (dict(fov=90, fxfycxcy=(1, 1, 0, 0)), dict(fov=0), dict(fov=180), dict(K=np.eye(2)),
                dict(fxfycxcy=(0, 1, 0, 0))):
        with pytest.raises(ValueError):
            pointcloud.camera_matrix(6, 8, **bad)


# ---------------------------------------------------------------------------------------------- test_simple.py
class StubPredictor:
    """`predict` as tests/test_predict_cli.py's stub; `predict_cloud` exports a made-up disparity of every image through
    `ops.point_cloud` on the host port, coloured by the image."""

    def __init__(self, port):
        self.port, self.calls, self.cloud_calls = port, [], []

    def predict(self, images, want_float=False, post_process=False):
        self.calls.append(([im.shape for im in images], want_float))
        return [inference.DepthPrediction(np.zeros(im.shape, np.uint8), 1.0, 2.0,
                                          np.ones(im.shape[:2], np.float32) if want_float else None) for im in images]

    def predict_cloud(self, images, inv_K=None, scale=1.0, max_depth=None, stride=1, post_process=False):
        self.cloud_calls.append(dict(shapes=[im.shape for im in images], inv_K=np.array(inv_K), scale=scale,
                                     max_depth=max_depth, stride=stride, post_process=post_process))
        sizes = [im.shape[:2] for im in images]
        disp = torch.linspace(0.05, 0.5, 6 * 8).view(1, 6, 8).repeat(len(images), 1, 1)      # depths 2 ... 20
        rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images]))
        return pointcloud.cloud_arrays(*ops.point_cloud(
            disp, ops.cloud_rows(sizes), inv_K, rgb=rgb, stride=stride, min_depth=0.0,
            max_depth=1e6 if max_depth is None else max_depth, pred_is_disp=True, scale_factor=scale, backend=self.port))


def _write(path, h, w, seed=0):
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def _argv(src, dst, *extra):
    return ["--image_path", str(src), "--save_path", str(dst), "--ext", "png", "--weights", "w"] + list(extra)


def test_point_cloud_flag_writes_a_ply_next_to_the_jpeg(tmp_path, port):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _write(src / "a.png", 37, 91, 1)
    _write(src / "b.png", 50, 64, 2)
    stub = StubPredictor(port)
    inference.run_cli(inference.parse_args(_argv(src, dst, "--point_cloud")), predictor=stub)
    assert sorted(os.listdir(dst)) == ["a_Base.jpg", "a_Base.ply", "b_Base.jpg", "b_Base.ply"]
    a = pointcloud.read_ply(str(dst / "a_Base.ply"))
    assert len(a) == 37 * 91 and len(pointcloud.read_ply(str(dst / "b_Base.ply"))) == 50 * 64
    image = np.asarray(Image.open(src / "a.png").convert("RGB"))
    assert np.array_equal(np.stack([a["red"], a["green"], a["blue"]], 1), image.reshape(-1, 3)) and (a["alpha"] == 255).all()
    call, = stub.cloud_calls
    assert call["shapes"] == [(37, 91, 3), (50, 64, 3)] and call["scale"] == 1.0 and call["max_depth"] is None
    assert call["stride"] == 1 and call["post_process"] is False
    assert np.array_equal(call["inv_K"], np.stack([pointcloud.intrinsics(37, 91), pointcloud.intrinsics(50, 64)]))
    assert stub.calls == [([(37, 91, 3), (50, 64, 3)], False)]           # the picture is made as before


def test_cloud_options_reach_the_predictor(tmp_path, port):
    src = tmp_path / "in"
    src.mkdir()
    _write(src / "a.png", 20, 30)
    stub = StubPredictor(port)
    args = inference.parse_args(_argv(src, tmp_path / "o", "--point_cloud", "--cloud_scale", "5.4", "--cloud_max_depth", "30",
                                      "--cloud_stride", "3", "--fov", "90", "--post_process"))
    inference.run_cli(args, predictor=stub)
    call, = stub.cloud_calls
    assert call["scale"] == 5.4 and call["max_depth"] == 30.0 and call["stride"] == 3 and call["post_process"] is True
    assert np.array_equal(call["inv_K"][0], pointcloud.intrinsics(20, 30, fov=90))
    a = pointcloud.read_ply(str(tmp_path / "o" / "a_Base.ply"))
    assert 0 < len(a) < 7 * 10 and (a["z"] <= 30).all()                   # depths 10.8 ... 108: the far ones are dropped
    stub = StubPredictor(port)
    args = inference.parse_args(_argv(src, tmp_path / "p", "--point_cloud", "--intrinsics", "25", "26", "15", "10"))
    inference.run_cli(args, predictor=stub)
    assert np.array_equal(stub.cloud_calls[0]["inv_K"][0], pointcloud.intrinsics(20, 30, fxfycxcy=(25, 26, 15, 10)))


def test_without_the_flag_the_run_makes_the_calls_it_made_before(tmp_path, port):
    src = tmp_path / "in"
    src.mkdir()
    _write(src / "a.png", 37, 91, 1)

    class OldPredictor:                      # the interface before this feature: no predict_cloud at all
        def __init__(self):
            self.calls = []

        def predict(self, images, want_float=False):
            self.calls.append(([im.shape for im in images], want_float))
            return [inference.DepthPrediction(np.zeros(im.shape, np.uint8), 1.0, 2.0) for im in images]

    old = OldPredictor()
    inference.run_cli(inference.parse_args(_argv(src, tmp_path / "o")), predictor=old)
    stub = StubPredictor(port)
    inference.run_cli(inference.parse_args(_argv(src, tmp_path / "p", "--cloud_stride", "2", "--fov", "70")), predictor=stub)
    assert old.calls == stub.calls == [([(37, 91, 3)], False)] and stub.cloud_calls == []
    assert os.listdir(tmp_path / "o") == os.listdir(tmp_path / "p") == ["a_Base.jpg"]


def test_fov_and_intrinsics_exclude_one_another(capsys):
    with pytest.raises(SystemExit):
        inference.parse_args(_argv("x", "y", "--point_cloud", "--fov", "90", "--intrinsics", "1", "1", "0", "0"))
    assert "not allowed with" in capsys.readouterr().err
    for bad in (["--cloud_stride", "0"], ["--cloud_scale", "0"]):
        with pytest.raises(SystemExit):
            inference.parse_args(_argv("x", "y", *bad))
    a = inference.parse_args(_argv("x", "y"))
    assert (a.point_cloud, a.cloud_scale, a.cloud_max_depth, a.cloud_stride, a.fov, a.intrinsics) == (False, 1.0, None, 1, None, None)
    with pytest.raises(SystemExit):
        inference.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--point_cloud" in text and "_Base.ply" in text and "5.4" in text


# ---------------------------------------------------------------------------------------------- evaluate_depth.py
def _parse(*argv):
    return MonodepthOptions().parse(["--eval_mono"] + [str(a) for a in argv])


def test_options_carry_the_cloud_flags(capsys):
    d = _parse()
    assert (d.save_clouds, d.cloud_count, d.cloud_stride, d.cloud_rays) == (None, 8, 1, "pixel")
    o = _parse("--save_clouds", "dir", "--cloud_count", 3, "--cloud_stride", 2, "--cloud_rays", "reference")
    assert (o.save_clouds, o.cloud_count, o.cloud_stride, o.cloud_rays) == ("dir", 3, 2, "reference")
    with pytest.raises(SystemExit):
        _parse("--save_clouds", "dir", "--no_eval")
    assert "--no_eval produces no metrics rows" in capsys.readouterr().err
    for bad in (("--cloud_rays", "other"), ("--save_clouds", "d", "--cloud_count", 0), ("--save_clouds", "d", "--cloud_stride", 0)):
        with pytest.raises(SystemExit):
            _parse(*bad)


def test_save_clouds_with_no_eval_is_refused_before_anything_is_touched():
    import types

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("nothing may be used before the refusal")

    opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, eval_split="eigen", splits_dir="nowhere",
                                save_clouds="somewhere", no_eval=True)
    with pytest.raises(ValueError, match="no_eval produces no metrics rows"):
        evaluation.evaluate(opt, dataloader=Untouchable(), models=(Untouchable(), Untouchable()))


def _valid(gt, lo, hi, window=None, stride=1):
    r0, r1, c0, c1 = window or (0, gt.shape[0], 0, gt.shape[1])
    g = gt[r0:r1:stride, c0:c1:stride]
    return int(((g > np.float32(lo)) & (g < np.float32(hi))).sum())


@pytest.mark.parametrize("stride", [1, 2])
def test_save_clouds_on_a_kitti_split(tmp_path, port, stride, capsys):
    rng = np.random.default_rng(6)
    n, N = 5, 2
    shapes = [(40, 120), (38, 124), (40, 120), (40, 120), (36, 118)]
    gts = np.empty(n, dtype=object)
    for i, (gh, gw) in enumerate(shapes):
        g = (3.0 + 60.0 * rng.random((gh, gw))).astype(np.float32)
        g[rng.random((gh, gw)) < 0.7] = 0.0                       # sparse, as LiDAR
        g[rng.random((gh, gw)) < 0.02] = 95.0                     # beyond 80 m
        gts[i] = g
    split = tmp_path / "splits" / "eigen"
    split.mkdir(parents=True)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    disps = (1.0 / (2.0 + 50.0 * rng.random((n, 12, 40)))).astype(np.float32)
    np.save(tmp_path / "disps.npy", disps)
    out = tmp_path / "clouds"
    opt = _parse("--eval_split", "eigen", "--splits_dir", tmp_path / "splits", "--ext_disp_to_eval", tmp_path / "disps.npy",
                 "--save_clouds", out, "--cloud_count", N, "--cloud_stride", stride)
    mean_errors, ratios = evaluation.evaluate(opt, batch_size=3, backend=port, device="cpu")
    assert mean_errors.shape == (7,) and ratios.shape == (n,) and "Saved 4 point clouds" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["0000_gt.ply", "0000_pred.ply", "0001_gt.ply", "0001_pred.ply"]
    for i in range(N):
        pred, gt = pointcloud.read_ply(str(out / ("%04d_pred.ply" % i))), pointcloud.read_ply(str(out / ("%04d_gt.ply" % i)))
        want = _valid(gts[i], 1e-3, 80.0, evaluation.garg_window(*shapes[i]), stride)
        assert len(pred) == len(gt) == want > 0
        # both clouds hold the same pixels in the same order: the same rays, scaled by the two depths
        inv_K = pointcloud.intrinsics(*shapes[i])
        for c in (pred, gt):
            d = c["z"] / inv_K[2, 2]
            assert (d >= 1e-3 * 0.999).all() and (d <= 80.0 * 1.001).all()
        np.testing.assert_allclose(pred["x"] * gt["z"], gt["x"] * pred["z"], rtol=1e-4, atol=1e-3)
    # the scores are what they are without the flag
    plain = _parse("--eval_split", "eigen", "--splits_dir", tmp_path / "splits", "--ext_disp_to_eval", tmp_path / "disps.npy")
    again, _ = evaluation.evaluate(plain, batch_size=3, backend=port, device="cpu")
    assert np.array_equal(mean_errors, again)


@pytest.mark.parametrize("rays", ["pixel", "reference"])
def test_save_clouds_on_a_syns_split(tmp_path, port, rays):
    n, N, gh, gw = 3, 2, 30, 52
    gts, edges = np.empty(n, dtype=object), np.empty(n, dtype=object)
    for i in range(n):
        gts[i], edges[i] = syns_checks.make_gt(60 + i, gh - (i % 2), gw)
    split = tmp_path / "splits" / "SYNS"
    split.mkdir(parents=True)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    np.savez_compressed(split / "gt_edges.npz", data=edges)
    disps = np.stack([1.0 / syns_checks.make_depth(7 + i, 16, 24) for i in range(n)]).astype(np.float32)
    np.save(tmp_path / "disps.npy", disps)
    out = tmp_path / "clouds"
    opt = _parse("--eval_split", "SYNS", "--splits_dir", tmp_path / "splits", "--ext_disp_to_eval", tmp_path / "disps.npy",
                 "--save_clouds", out, "--cloud_count", N, "--cloud_rays", rays, "--chamfer")
    mean_errors, ratios = evaluation.evaluate(opt, batch_size=2, backend=port, device="cpu")
    assert mean_errors.shape == (9,) and ratios.shape == (n,)
    assert sorted(os.listdir(out)) == ["0000_gt.ply", "0000_pred.ply", "0001_gt.ply", "0001_pred.ply"]
    for i in range(N):
        pred, gt = pointcloud.read_ply(str(out / ("%04d_pred.ply" % i))), pointcloud.read_ply(str(out / ("%04d_gt.ply" % i)))
        assert len(pred) == len(gt) == _valid(gts[i], 1e-3, 125.0) > 0
        assert len(pred) < gts[i].size                                   # the mask mattered
