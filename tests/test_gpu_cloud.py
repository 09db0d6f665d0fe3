"""GPU tier of the point-cloud export (bbd_cloud.hip through the C ABI): the checks of tests/cloud_checks.py - bit for bit
against tests/cloud_ref.py - then one call at the workload's own size against the host port,
`DepthPredictor.predict_cloud` on a randomly initialised network and `evaluate(..., save_clouds=)` on a synthetic split."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_checks as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.mark.parametrize("check", C.ALL_CHECKS, ids=lambda f: f.__name__)
def test_kernels(hip, check):
    check(hip, DEV)


@pytest.fixture(scope="module")
def workload():
    """4 images of 375 x 1242 from a 192 x 640 disparity, ground truth with holes, colours: inputs, and the port's
    answer at stride 1 and 3 (computed once)."""
    from ports import PortBackend
    rng = np.random.default_rng(40)
    shapes = [(375, 1242)] * 4
    gts = [C.depth_like(rng, 375, 1242, 2.0, 90.0) for _ in shapes]
    for g in gts:
        g[rng.random(g.shape) < 0.5] = 0.0
    case = dict(pred=1.0 / np.stack([C.depth_like(rng, 192, 640, 1.0, 100.0) for _ in shapes]), shapes=shapes, gts=gts,
                ratios=[1.1, 0.9, 1.0, 1.3], rgbs=C.colours(rng, shapes))
    port = PortBackend()
    want = {}
    for stride in (1, 3):
        case["kw"] = dict(stride=stride, pred_is_disp=True, mask_gt=stride == 1, min_depth=1e-3, max_depth=80.0)
        want[stride] = C.run_case(port, "cpu", case)
    return case, want


@pytest.mark.parametrize("stride", [1, 3])
def test_workload_size_equals_the_port(hip, workload, stride):
    case, want = workload
    case = dict(case, kw=dict(stride=stride, pred_is_disp=True, mask_gt=stride == 1, min_depth=1e-3, max_depth=80.0))
    got = C.run_case(hip, DEV, case)
    print("stride %d: capacities %s, counts %s" % (stride, got[3], got[1].tolist()))
    assert got[3] == [len(range(0, 375, stride)) * len(range(0, 1242, stride))] * 4
    assert np.array_equal(got[1], want[stride][1]) and (0 < got[1]).all() and (got[1] < got[3]).all()
    assert np.array_equal(got[0], want[stride][0])


def test_predict_cloud_equals_point_cloud_on_last_disp(hip):
    from baseboostdepth_amd import inference, networks, ops, pointcloud, tuning
    # as DepthPredictor.from_weights, Trainer and evaluate do before their first convolution: MIOpen fixes its database
    # when the process first uses it, and this may be the first GPU test of the process to run a network
    tuning.use_shipped_db()
    torch.manual_seed(3)
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    pred = inference.DepthPredictor(enc, dec, 64, 128, DEV, batch_size=4)
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (37, 91, 3), dtype=np.uint8), rng.integers(0, 256, (50, 64, 3), dtype=np.uint8)]
    clouds = pred.predict_cloud(images, scale=5.4, stride=2)
    disp = pred.last_disp
    again = pred.predict_cloud(images, scale=5.4, stride=2)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(clouds, again))
    sizes = [(37, 91), (50, 64)]
    scaled = 1.0 / pred.max_depth + (1.0 / pred.min_depth - 1.0 / pred.max_depth) * disp
    rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    inv_K = np.stack([pointcloud.intrinsics(h, w) for h, w in sizes])
    want = pointcloud.cloud_arrays(*ops.point_cloud(scaled, ops.cloud_rows(sizes), inv_K, rgb=rgb, stride=2, min_depth=0.0,
                                                    max_depth=pred.max_depth * 5.4, pred_is_disp=True, scale_factor=5.4))
    for c, w, im, (h, wd) in zip(clouds, want, images, sizes):
        assert c.dtype == pointcloud.VERTEX_DTYPE and len(c) == len(range(0, h, 2)) * len(range(0, wd, 2))
        assert np.array_equal(c.view(np.uint8), w.view(np.uint8))
        assert np.array_equal(np.stack([c["red"], c["green"], c["blue"]], 1), im[::2, ::2].reshape(-1, 3))
        assert (c["z"] > 0).all() and (c["z"] <= np.float32(pred.max_depth * 5.4)).all() and (c["alpha"] == 255).all()


def test_evaluate_save_clouds_on_the_device(tmp_path, hip):
    """`evaluate(..., save_clouds=DIR)` on a synthetic KITTI split of saved disparities: the ground-truth files equal the
    host port's byte for byte, the prediction files equal a direct `ops.point_cloud` call on the device's own metrics
    rows (the ratio is read on the device), and the scores are those of a run without the flag."""
    from ports import PortBackend
    from baseboostdepth_amd import evaluation, ops, pointcloud
    from baseboostdepth_amd.options import MonodepthOptions
    rng = np.random.default_rng(6)
    shapes = [(40, 120), (38, 124), (40, 120), (36, 118)]
    gts = np.empty(len(shapes), dtype=object)
    for i, (gh, gw) in enumerate(shapes):
        g = C.depth_like(rng, gh, gw, 3.0, 63.0)
        g[rng.random((gh, gw)) < 0.7] = 0.0
        g[rng.random((gh, gw)) < 0.02] = 95.0
        gts[i] = g
    split = tmp_path / "splits" / "eigen"
    split.mkdir(parents=True)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    disps = (1.0 / np.stack([C.depth_like(rng, 12, 40, 2.0, 52.0) for _ in shapes])).astype(np.float32)
    np.save(tmp_path / "disps.npy", disps)
    base = ["--eval_mono", "--eval_split", "eigen", "--splits_dir", str(tmp_path / "splits"), "--ext_disp_to_eval",
            str(tmp_path / "disps.npy")]
    mean_plain, _ = evaluation.evaluate(MonodepthOptions().parse(base), batch_size=3)
    for where, kw in (("dev", {}), ("port", dict(backend=PortBackend(), device="cpu"))):
        opt = MonodepthOptions().parse(base + ["--save_clouds", str(tmp_path / where), "--cloud_count", "4", "--cloud_stride", "2"])
        mean, _ = evaluation.evaluate(opt, batch_size=3, **kw)
        if where == "dev":
            assert np.array_equal(mean, mean_plain)
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(os.listdir(tmp_path / "port")) and len(os.listdir(tmp_path / "dev")) == 8
    gset = evaluation.GroundTruthSet(list(gts), torch.device(DEV))
    pred = torch.from_numpy(disps).to(DEV)
    rows = evaluation.depth_metrics(pred, gset, [0, 1, 2, 3], min_depth=1e-3, max_depth=80.0, pred_is_disp=True, median="numpy")
    inv_K = np.stack([pointcloud.intrinsics(*s) for s in shapes])
    want = pointcloud.cloud_arrays(*ops.point_cloud(pred, gset.desc_host, inv_K, gt=gset.buffer, rows=rows, stride=2,
                                                    min_depth=1e-3, max_depth=80.0, pred_is_disp=True, clamp_depth=True,
                                                    mask_gt=True))
    for i in range(4):
        gt_dev = (tmp_path / "dev" / ("%04d_gt.ply" % i)).read_bytes()
        assert gt_dev == (tmp_path / "port" / ("%04d_gt.ply" % i)).read_bytes()
        got = pointcloud.read_ply(str(tmp_path / "dev" / ("%04d_pred.ply" % i)))
        assert len(got) == len(pointcloud.read_ply(str(tmp_path / "dev" / ("%04d_gt.ply" % i)))) > 0
        assert np.array_equal(got.view(np.uint8), want[i].view(np.uint8))
