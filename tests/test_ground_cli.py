"""CPU tier of the ground-scale command lines: the options, `test_simple.py --point_cloud --camera_height` with a real
`DepthPredictor` around a network that returns a synthetic road, and `evaluate_depth.py --scale_recovery ground` on a
synthetic KITTI split, the kernels replaced by their host ports (tests/ports.py)."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ground_ref  # noqa: E402
from baseboostdepth_amd import evaluation, inference, ops, pointcloud  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

HEIGHT = 1.65


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


# ---------------------------------------------------------------------------------------------- options
def _argv(src, dst, *extra):
    return ["--image_path", str(src), "--save_path", str(dst), "--ext", "png", "--weights", "w"] + list(extra)


def test_test_simple_options(capsys):
    a = inference.parse_args(_argv("x", "y"))
    assert (a.camera_height, a.ground_angle, a.ground_mask) == (None, 5.0, False)
    a = inference.parse_args(_argv("x", "y", "--point_cloud", "--camera_height", "1.65", "--ground_angle", "7.5",
                                   "--ground_mask", "--cloud_scale", "1.0"))
    assert (a.camera_height, a.ground_angle, a.ground_mask, a.cloud_scale) == (1.65, 7.5, True, 1.0)
    for bad, word in ((["--camera_height", "1.65"], "needs --point_cloud"),
                      (["--point_cloud", "--camera_height", "1.65", "--cloud_scale", "5.4"], "--cloud_scale"),
                      (["--point_cloud", "--camera_height", "0"], "positive"),
                      (["--point_cloud", "--ground_mask"], "needs --camera_height"),
                      (["--point_cloud", "--camera_height", "1.65", "--ground_angle", "90"], "--ground_angle")):
        with pytest.raises(SystemExit):
            inference.parse_args(_argv("x", "y", *bad))
        assert word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        inference.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--camera_height METRES" in text and "_Base_ground.png" in text


def _parse(*argv):
    return MonodepthOptions().parse(["--eval_mono"] + [str(a) for a in argv])


def test_evaluate_depth_options(capsys):
    d = _parse()
    assert (d.scale_recovery, d.camera_height, d.ground_angle) == ("median", 1.65, 5.0)
    g = _parse("--scale_recovery", "ground", "--camera_height", 1.7, "--ground_angle", 3)
    assert (g.scale_recovery, g.camera_height, g.ground_angle) == ("ground", 1.7, 3.0)
    for bad, word in ((("--scale_recovery", "ground", "--disable_median_scaling"), "--disable_median_scaling"),
                      (("--scale_recovery", "ground", "--eval_split", "SYNS"), "--eval_split SYNS"),
                      (("--scale_recovery", "ground", "--camera_height", 0), "--camera_height"),
                      (("--scale_recovery", "other"), "invalid choice")):
        with pytest.raises(SystemExit):
            _parse(*bad)
        assert word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        MonodepthOptions().parse(["--eval_stereo", "--scale_recovery", "ground"])
    assert "--eval_stereo" in capsys.readouterr().err
    _parse("--disable_median_scaling")                                   # as before without the new flag
    import types
    opt = types.SimpleNamespace(eval_mono=False, eval_stereo=True, cuda=0, eval_split="eigen", splits_dir="nowhere",
                                scale_recovery="ground", disable_median_scaling=False)
    with pytest.raises(ValueError, match="excludes eval_stereo"):        # refused before anything is touched
        evaluation.evaluate(opt, dataloader=object(), models=(object(), object()))


# ---------------------------------------------------------------------------------------------- test_simple.py
FEED, SIZE, SCALE = (33, 130), (66, 260), 7.3


class SceneEncoder(torch.nn.Module):
    def forward(self, x):
        return [x]


class SceneDecoder(torch.nn.Module):
    """Returns the raw disparities whose scaled disparity (min_disp + (max_disp - min_disp) * raw) is `scaled`."""

    def __init__(self, scaled, min_depth=0.1, max_depth=80.0):
        super().__init__()
        lo, hi = 1.0 / max_depth, 1.0 / min_depth
        self.raw = torch.from_numpy(((scaled.astype(np.float64) - lo) / (hi - lo)).astype(np.float32))[:, None]

    def forward(self, feats):
        assert tuple(feats[0].shape[-2:]) == tuple(self.raw.shape[-2:])
        return {("disp", 0): self.raw[:feats[0].shape[0]]}


def _map_inv_K():
    return pointcloud.intrinsics_at(pointcloud.intrinsics(*SIZE), SIZE, FEED)


def _scene_predictor(port, planes):
    depth = np.stack([ground_ref.scene(*FEED, scale=SCALE, plane=p, inv_K=_map_inv_K()) for p in planes])
    assert depth.min() > 0.1 and depth.max() < 80.0                     # inside the sigmoid's range
    return inference.DepthPredictor(SceneEncoder(), SceneDecoder(np.float32(1) / depth), *FEED, "cpu", backend=port), depth


def _write(path, seed):
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, SIZE + (3,), dtype=np.uint8)).save(path)


def test_camera_height_writes_a_metric_cloud_a_mask_and_a_line(tmp_path, port, capsys):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _write(src / "road.png", 1)
    _write(src / "wall.png", 2)
    predictor, depth = _scene_predictor(port, (True, False))             # sorted names: road, wall
    args = inference.parse_args(_argv(src, dst, "--point_cloud", "--camera_height", str(HEIGHT), "--ground_mask"))
    inference.run_cli(args, predictor=predictor)
    out = capsys.readouterr().out
    assert sorted(os.listdir(dst)) == ["road_Base.jpg", "road_Base.ply", "road_Base_ground.png",
                                       "wall_Base.jpg", "wall_Base.ply", "wall_Base_ground.png"]
    # what the line says is what ops.ground_scale gives for the scaled disparity the predictor saw
    rows, masks = ops.ground_scale(torch.from_numpy(np.float32(1) / depth), _map_inv_K(), camera_height=HEIGHT,
                                   pred_is_disp=True, want_mask=True, backend=port)
    rows, masks = rows.numpy(), masks.numpy()
    assert abs(rows[0, 7] / SCALE - 1.0) < 1e-4 and np.isnan(rows[1, 7])
    assert "   road.png: scale {:.4f} | median ground height {:.4f} | ground {:.1f}% of {:d} candidates".format(
        rows[0, 7], rows[0, 0], 100.0 * rows[0, 1] / rows[0, 2], int(rows[0, 2])) in out
    assert "WARNING: wall.png: no ground found (0 ground pixels of {:d} candidates)".format(int(rows[1, 2])) in out
    road_mask = np.asarray(Image.open(dst / "road_Base_ground.png"))
    assert road_mask.shape == FEED and road_mask.dtype == np.uint8 and set(np.unique(road_mask)) == {0, 255}
    # (the decoder's float32 raw disparity moves the scaled one by an ulp or so: the mask may differ at single pixels)
    assert (road_mask != masks[0] * 255).mean() < 0.01
    assert not np.asarray(Image.open(dst / "wall_Base_ground.png")).any()
    # the cloud is in metres: every pixel is exported (the wall stands 20 m away), the road lies a camera height below
    assert len(pointcloud.read_ply(str(dst / "wall_Base.ply"))) == 0
    cloud = pointcloud.read_ply(str(dst / "road_Base.ply"))
    assert len(cloud) == SIZE[0] * SIZE[1]
    z = cloud["z"].reshape(SIZE)
    assert abs(z.max() / ground_ref.WALL - 1.0) < 1e-3
    # image pixels whose map neighbourhood is all ground: a plane's disparity is linear in the pixel, so the resampling
    # to the image's size is exact up to rounding
    inner = road_mask == 255
    inner[1:-1, 1:-1] &= (road_mask[:-2, 1:-1] == 255) & (road_mask[2:, 1:-1] == 255) & (road_mask[1:-1, :-2] == 255) \
        & (road_mask[1:-1, 2:] == 255)
    y = cloud["y"].reshape(SIZE)[np.repeat(np.repeat(inner, 2, 0), 2, 1)]
    assert len(y) > 1000 and (np.abs(y / HEIGHT - 1.0) < 1e-3).all()
    image = np.asarray(Image.open(src / "road.png").convert("RGB"))
    assert np.array_equal(np.stack([cloud["red"], cloud["green"], cloud["blue"]], 1), image.reshape(-1, 3))


def test_predictor_ground_scale_and_the_keyword_of_predict_cloud(port):
    predictor, depth = _scene_predictor(port, (True, False))
    images = [np.zeros(SIZE + (3,), np.uint8)] * 2
    rows, masks = predictor.ground_scale(images, camera_height=HEIGHT, want_mask=True)
    assert rows.shape == (2, 12) and rows.dtype == np.float32 and masks.shape == (2,) + FEED and masks.dtype == np.uint8
    assert abs(rows[0, 7] / SCALE - 1.0) < 1e-4 and np.isnan(rows[1, 7]) and masks[0].sum() == rows[0, 1]
    assert np.array_equal(predictor.ground_scale(images, camera_height=HEIGHT)[0], rows[0])
    plain = predictor.predict_cloud(images)                              # as before: a list, arbitrary units
    assert isinstance(plain, list) and abs(plain[0]["z"].max() * SCALE / ground_ref.WALL - 1.0) < 1e-3
    clouds, ground = predictor.predict_cloud(images, camera_height=HEIGHT)
    assert np.array_equal(ground["rows"].view(np.uint32), rows.view(np.uint32)) and ground["masks"] is None
    assert len(clouds[1]) == 0 and abs(clouds[0]["z"].max() / ground_ref.WALL - 1.0) < 1e-3
    assert len(predictor.predict_cloud(images, camera_height=HEIGHT, max_depth=10.0)[0][0]) < len(clouds[0])
    with pytest.raises(ValueError, match="scale must be 1.0"):
        predictor.predict_cloud(images, camera_height=HEIGHT, scale=5.4)


def test_old_predictors_meet_no_new_keyword(tmp_path, port):
    """Without --camera_height the predictor is called as before this feature."""
    src = tmp_path / "in"
    src.mkdir()
    _write(src / "a.png", 1)
    seen = []

    class Old:
        def predict(self, images, want_float=False):
            return [inference.DepthPrediction(np.zeros(im.shape, np.uint8), 1.0, 2.0) for im in images]

        def predict_cloud(self, images, inv_K=None, scale=1.0, max_depth=None, stride=1, post_process=False):
            seen.append(scale)
            return [np.zeros(0, pointcloud.VERTEX_DTYPE) for _ in images]

    inference.run_cli(inference.parse_args(_argv(src, tmp_path / "o", "--point_cloud", "--cloud_scale", "5.4")), predictor=Old())
    assert seen == [5.4] and sorted(os.listdir(tmp_path / "o")) == ["a_Base.jpg", "a_Base.ply"]


# ---------------------------------------------------------------------------------------------- evaluate_depth.py
def _split(tmp_path):
    rng = np.random.default_rng(8)
    h, w = 33, 130
    shapes = [(40, 120), (38, 124), (40, 120), (36, 118)]
    depth = np.stack([ground_ref.scene(h, w, scale=7.3), ground_ref.scene(h, w, pitch_deg=2.0, scale=3.1),
                      ground_ref.scene(h, w, plane=False), ground_ref.scene(h, w, pitch_deg=-3.0, noise=0.002, seed=9)])
    gts = np.empty(len(shapes), dtype=object)
    for i, (gh, gw) in enumerate(shapes):
        g = (3.0 + 60.0 * rng.random((gh, gw))).astype(np.float32)
        g[rng.random((gh, gw)) < 0.7] = 0.0
        gts[i] = g
    split = tmp_path / "splits" / "eigen"
    split.mkdir(parents=True)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    np.save(tmp_path / "disps.npy", np.float32(1) / depth)
    return np.float32(1) / depth, gts, ("--eval_split", "eigen", "--splits_dir", tmp_path / "splits",
                                         "--ext_disp_to_eval", tmp_path / "disps.npy")


def test_scale_recovery_ground_on_a_kitti_split(tmp_path, port, capsys):
    disps, gts, argv = _split(tmp_path)
    n, (h, w) = len(gts), disps.shape[1:]
    opt = _parse(*argv, "--scale_recovery", "ground", "--save_clouds", tmp_path / "clouds", "--cloud_count", 2)
    before = len(port.calls)
    mean_errors, ratios = evaluation.evaluate(opt, batch_size=3, backend=port, device="cpu")
    out = capsys.readouterr().out
    assert port.calls[before:].count("bbd_ground_scale") == 2 and port.calls[before:].count("bbd_depth_metrics") == 2
    # by hand: the ground rows, the disparities divided by their scale, depth_metrics without any other scaling
    ground = ops.ground_scale(torch.from_numpy(disps), pointcloud.intrinsics(h, w), camera_height=1.65, angle_deg=5.0,
                              pred_is_disp=True, backend=port)[0]
    scaled = torch.from_numpy(disps) / ground[:, 7].view(n, 1, 1)
    truth = evaluation.GroundTruthSet(gts, "cpu")
    rows = evaluation.depth_metrics(scaled, truth, list(range(n)), min_depth=1e-3, max_depth=80.0, pred_is_disp=True,
                                    median="numpy", median_scaling=False, scale_factor=1, backend=port)
    rows, ground = rows.numpy().astype(np.float64), ground.numpy().astype(np.float64)
    found = np.array([True, True, False, True])
    assert np.array_equal(np.isfinite(ground[:, 7]), found)
    assert np.array_equal(ratios, ground[:, 7], equal_nan=True) and ratios.dtype == np.float64
    assert np.array_equal(mean_errors, rows[found, :7].mean(0)) and np.isfinite(mean_errors).all()
    assert abs(ratios[0] / 7.3 - 1.0) < 1e-5 and abs(ratios[1] / 3.1 - 1.0) < 1e-5 and abs(ratios[3] - 1.0) < 2e-2
    med = np.median(ground[found, 7])
    assert " Scaling ratios | med: {:0.3f} | std: {:0.3f}\n".format(med, np.std(ground[found, 7] / med)) in out
    assert "WARNING: no ground found in 1 of 4 images, left out of the mean: 2\n" in out
    assert ("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\" in out
    # the clouds are those of the scaled disparities
    assert sorted(os.listdir(tmp_path / "clouds")) == ["0000_gt.ply", "0000_pred.ply", "0001_gt.ply", "0001_pred.ply"]
    want = ops.point_cloud(scaled[:2], truth.desc_host[[0, 1]],
                           np.stack([pointcloud.intrinsics(*truth.shapes[i]) for i in (0, 1)]), gt=truth.buffer,
                           min_depth=1e-3, max_depth=80.0, mask_gt=True, pred_is_disp=True, clamp_depth=True, backend=port)
    for i, arr in enumerate(pointcloud.cloud_arrays(*want)):
        got = pointcloud.read_ply(str(tmp_path / "clouds" / ("%04d_pred.ply" % i)))
        assert len(got) > 0 and np.array_equal(got.view(np.uint8), arr.view(np.uint8))


def test_scale_recovery_median_prints_what_it_printed_before(tmp_path, port, capsys):
    disps, gts, argv = _split(tmp_path)
    n = len(gts)
    plain_errors, plain_ratios = evaluation.evaluate(_parse(*argv), batch_size=3, backend=port, device="cpu")
    plain = capsys.readouterr().out
    before = len(port.calls)
    errors, ratios = evaluation.evaluate(_parse(*argv, "--scale_recovery", "median", "--camera_height", 2.0),
                                         batch_size=3, backend=port, device="cpu")
    assert "bbd_ground_scale" not in port.calls[before:]
    assert capsys.readouterr().out == plain and np.array_equal(errors, plain_errors) and np.array_equal(ratios, plain_ratios)
    # the text of the evaluation as it stood before the option, restated from the metrics rows
    rows = evaluation.depth_metrics(torch.from_numpy(disps), evaluation.GroundTruthSet(gts, "cpu"), list(range(n)),
                                    min_depth=1e-3, max_depth=80.0, pred_is_disp=True, median="numpy", backend=port)
    rows = rows.numpy().astype(np.float64)
    med = np.median(rows[:, 7])
    want = "-> Loading predictions from {}\n".format(tmp_path / "disps.npy") \
        + " Scaling ratios | med: {:0.3f} | std: {:0.3f}\n".format(med, np.std(rows[:, 7] / med)) \
        + "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3") + "\n" \
        + ("&{: 8.3f}  " * 7).format(*rows[:, :7].mean(0).tolist()) + "\\\\\n"
    assert plain == want
