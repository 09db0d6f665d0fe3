"""CPU tier of the SYNS-Patches metrics: the product's Python layers (evaluation.pred_edges / distance_transform /
edge_metrics / pointcloud_metrics, ops.chamfer_nn) run through the host port of bbd_syns.hip (the same per-pixel
arithmetic, bbd_syns_math.h) and are compared with the numpy reference tests/syns_ref.py under the rules of
tests/syns_checks.py.  Also: the dataset's paths and camera, and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import syns_checks as C  # noqa: E402
import syns_ref  # noqa: E402


@pytest.fixture(scope="module")
def be():
    from ports import PortBackend
    return PortBackend()


def _set(gts, edges, crop=False):
    from baseboostdepth_amd.evaluation import GroundTruthSet
    return GroundTruthSet(gts, "cpu", crop=crop, edges=edges)


def _rows(ratios):
    rows = torch.zeros(len(ratios), 12)
    rows[:, 7] = torch.tensor([float(r) for r in ratios])
    return rows


# ------------------------------------------------------------------------------------------------ distance transform
def _edt_maps():
    rng = np.random.default_rng(11)
    maps = [rng.random((37, 53)) < p for p in (0.002, 0.05, 0.5)]
    line = np.zeros((40, 64), bool)
    line[7, :] = True
    corner = np.zeros((40, 64), bool)
    corner[0, 0] = corner[39, 63] = True
    col = np.zeros((33, 21), bool)
    col[:, 20] = True
    return maps + [line, corner, col, np.ones((5, 9), bool), np.zeros((6, 7), bool)]


def test_distance_transform_equals_scipy_exactly(be):
    ndimage = pytest.importorskip("scipy.ndimage")
    from baseboostdepth_amd.evaluation import distance_transform, syns_strides, image_view
    maps = _edt_maps()
    gts = _set([np.ones(m.shape, np.float32) for m in maps], None)
    _, _, stride = syns_strides(gts)
    buf = torch.zeros(len(maps), stride, dtype=torch.uint8)
    for i, m in enumerate(maps):
        buf[i, :m.size] = torch.from_numpy(m.reshape(-1).astype(np.uint8))
    out = distance_transform(buf, gts, list(range(len(maps))), backend=be)
    for i, m in enumerate(maps):
        got = image_view(out, gts, i, i).numpy()
        assert np.array_equal(got, syns_ref.edt_sq(m)), i
        if m.any():
            assert np.array_equal(np.sqrt(got.astype(np.float64)), ndimage.distance_transform_edt(1 - m)), i
        else:
            assert (got == 2 ** 30).all()


def test_distance_transform_refuses_sizes_that_would_overflow(be):
    import ctypes
    m, d, o = np.zeros(4, np.uint8), np.array([0, 0, 1, 4, 0, 1, 0, 4], np.int32), np.zeros(4, np.int32)
    pm, pd, po = (ctypes.c_void_p(x.ctypes.data) for x in (m, d, o))
    assert be.status("bbd_syns_edt", pm, pd, po, 1, 4, 1, 4) == 0
    # the launch bounds, not the image, are what is checked: 32768 rows or more, or more than 8192 columns
    assert be.status("bbd_syns_edt", pm, pd, po, 1, 40000 * 8192, 40000, 8192) == -2
    assert be.status("bbd_syns_edt", pm, pd, po, 1, 4 * 8196, 4, 8193) == -2
    assert be.lib.syns_scratch_ints(512, 376 * 1242) == -2 and be.lib.syns_scratch_ints(8, 376 * 1242) > 0


# ------------------------------------------------------------------------------------------------ nearest neighbour
def test_nearest_neighbour_port_equals_numpy_bit_for_bit(be):
    from baseboostdepth_amd import ops
    rng = np.random.default_rng(5)
    for na, nb in ((1, 1), (257, 130), (700, 1100)):
        a = (rng.standard_normal((na, 3)) * 5).astype(np.float32)
        b = (rng.standard_normal((nb, 3)) * 5).astype(np.float32)
        b[: min(na, nb) // 2] = a[: min(na, nb) // 2]                   # exact zeros
        nn_a, nn_b = ops.chamfer_nn(torch.from_numpy(a), torch.from_numpy(b), backend=be)
        assert np.array_equal(nn_a.numpy().view(np.uint32), syns_ref.nn_sq(a, b).view(np.uint32))
        assert np.array_equal(nn_b.numpy().view(np.uint32), syns_ref.nn_sq(b, a).view(np.uint32))
    nn_a, nn_b = ops.chamfer_nn(torch.from_numpy(a), torch.zeros(0, 3), backend=be)
    assert torch.isinf(nn_a).all() and nn_b.numel() == 0


# ------------------------------------------------------------------------------------------------ edges and metrics
@pytest.mark.parametrize("mode", ["evaluate", "trainer"])
def test_edge_maps_and_metrics_match_reference_ragged_batch(be, mode):
    """ramp_a and ramp_b share a prediction size and differ in ground-truth size: ONE call scores both."""
    from baseboostdepth_amd.evaluation import pred_edges, edge_metrics, image_view
    names = ["ramp_a", "ramp_b"]
    ins = [C.case_inputs(n) for n in names]
    gts = _set([i[1] for i in ins], [i[2] for i in ins])
    depth = np.stack([i[0] for i in ins])
    pred = torch.from_numpy(1.0 / depth if mode == "evaluate" else depth).float()
    ev = mode == "evaluate"
    edge, stats = pred_edges(pred, gts, [0, 1], pred_is_disp=ev, backend=be)
    at_gt = [C.resized(pred[i].numpy(), *ins[i][1].shape, mode) for i in range(2)]
    ratios = [C.scaled(at_gt[i], ins[i][1], mode)[1] for i in range(2)]
    lo, hi = C.depth_range(mode)
    rows = edge_metrics(pred, gts, [0, 1], edge, _rows(ratios), min_depth=float(lo), max_depth=float(hi),
                        pred_is_disp=ev, backend=be).numpy()
    for i, n in enumerate(names):
        e = image_view(edge, gts, i, i).numpy()
        C.check_edge_map(e, at_gt[i], n)
        assert int(stats[i, 1]) == int(e.sum())
        want, want_err = C.check_edge_metrics(rows[i], e, at_gt[i], ins[i][1], ins[i][2], mode, what=n)
        assert 0 < want["n_near"] < want["n_edge"] and want["edge_Acc"] < 10 and want["edge_comp"] > 0
        np.testing.assert_allclose(rows[i, 2], want_err, rtol=3e-5, atol=2e-6)
    # a batch gives the bits of one call per image
    for i in range(2):
        e1, s1 = pred_edges(pred[i:i + 1], gts, [i], pred_is_disp=ev, backend=be)
        assert torch.equal(e1[0], edge[i]) and torch.equal(s1[0], stats[i])


def test_noise_input_and_same_size(be):
    from baseboostdepth_amd.evaluation import pred_edges, image_view
    for n in ("noise", "same_size"):
        depth, gt, ge = C.case_inputs(n)
        gts = _set([gt], [ge])
        edge, _ = pred_edges(torch.from_numpy(1.0 / depth)[None], gts, [0], pred_is_disp=True, backend=be)
        C.check_edge_map(image_view(edge, gts, 0, 0).numpy(), C.resized(1.0 / depth, *gt.shape, "evaluate"), n)


def test_degenerate_edge_cases(be):
    from baseboostdepth_amd.evaluation import pred_edges, edge_metrics, image_view
    gh, gw = 40, 60
    gt = np.full((gh, gw), 10.0, np.float32)
    far_edge = np.zeros((gh, gw, 1), bool)
    far_edge[2, 2] = True
    no_edge = np.zeros((gh, gw, 1), bool)
    gts = _set([gt, gt, gt], [far_edge, far_edge, no_edge])
    flat = np.full((gh, gw), 5.0, np.float32)                       # constant depth: magnitude 0 everywhere, no edge
    step = flat.copy()
    step[30:, 40:] = 20.0                                            # an edge far (> 10 px) from the only target pixel
    pred = torch.from_numpy(np.stack([flat, step, step]))
    edge, stats = pred_edges(pred, gts, [0, 1, 2], backend=be)
    assert int(stats[0, 1]) == 0 and int(stats[1, 1]) > 0
    rows = edge_metrics(pred, gts, [0, 1, 2], edge, _rows([1, 1, 1]), min_depth=1e-3, max_depth=80.0, backend=be).numpy()
    assert rows[0, 0] == 10.0 and rows[0, 1] == 10.0 and rows[0, 3] == 0 and rows[0, 6] == 0     # no predicted edge
    assert rows[1, 0] == 10.0 and rows[1, 1] == 10.0 and rows[1, 3] == 0 and rows[1, 6] > 0      # none within 10 px
    assert np.isnan(rows[2, 0]) and np.isnan(rows[2, 1]) and rows[2, 4] == 0                     # empty target
    assert rows[2, 5] == gh * gw and np.isfinite(rows[2, 2])                                     # err is still defined
    for i in range(2):
        want = syns_ref.edge_metrics(image_view(edge, gts, i, i).numpy(), gt, far_edge, 1e-3, 80.0)
        assert want["edge_Acc"] == 10.0 and want["edge_comp"] == 10.0
    assert np.isnan(syns_ref.edge_metrics(image_view(edge, gts, 2, 2).numpy(), gt, no_edge, 1e-3, 80.0)["edge_Acc"])


# ------------------------------------------------------------------------------------------------ point clouds
@pytest.mark.parametrize("rays", ["reference", "pixel"])
def test_pointcloud_metrics_equal_numpy_float32(be, rays):
    from baseboostdepth_amd.evaluation import pointcloud_metrics
    from baseboostdepth_amd.datasets import SYNSRAWDataset
    inv_K = SYNSRAWDataset.load_intrinsic_syns()[1]
    rng = np.random.default_rng(2)
    gh, gw = 24, 40
    gt = (4.0 + 6.0 * rng.random((gh, gw))).astype(np.float32)
    gt[rng.random((gh, gw)) > 0.6] = 0.0
    close = (gt + 0.08 * rng.standard_normal((gh, gw))).astype(np.float32).clip(1.0, None)     # some within 0.1 m
    far = (gt * 3.0 + 20.0).astype(np.float32)                                                  # none: P = R = 0
    gts = _set([gt, gt], None)
    pred = torch.from_numpy(np.stack([1.0 / close, 1.0 / far])).float()
    at_gt = [C.resized(pred[i].numpy(), gh, gw, "evaluate") for i in range(2)]
    for scaling in (True, False):              # without median scaling the second cloud stays far from its target
        sc = [C.scaled(a, gt, "evaluate", scaling) for a in at_gt]
        got = pointcloud_metrics(pred, gts, [0, 1], _rows([s[1] for s in sc]), inv_K, pred_is_disp=True, rays=rays,
                                 median_scaling=scaling, backend=be).numpy()
        for i in range(2):
            f, iou, P, R, nn_p, nn_t = syns_ref.pointcloud_metrics(sc[i][0], gt, inv_K, np.float32(1e-3), np.float32(125), rays)
            print(rays, scaling, i, "got", got[i], "want", f, iou, P, R)
            assert got[i, 6] == len(nn_p)
            assert np.array_equal(got[i, :4].view(np.uint32), np.array([f, iou, P, R], np.float32).view(np.uint32))
        assert 1e-3 < got[0, 2] < 1 and got[0, 0] != got[0, 1]
    assert got[1, 2] < 1e-3 and got[1, 3] < 1e-3 and got[1, 0] == got[1, 2] == got[1, 1]       # the P, R < 1e-3 branch
    if rays == "reference":                     # the pairing itself: flat pixel k rides the ray of (k // GH, k % GH)
        pts = syns_ref.backproject(np.ones((gh, gw), np.float32), inv_K)
        k = 3 * gw + 7
        want = np.asarray(inv_K, np.float32)[:3, :3] @ np.array([k // gh, k % gh, 1], np.float32)
        np.testing.assert_allclose(pts[k], want, rtol=1e-6)


def test_f_score_and_iou_arithmetic():
    """evaluate_depth.py:49-55 on chosen counts, against torch's own float32 evaluation of the reference's lines."""
    for cp, ct, n in ((0, 0, 1000), (0, 5, 10000), (9, 9, 10000), (10, 3, 10000), (400, 900, 1000), (1000, 1000, 1000)):
        nn_p = np.where(np.arange(n) < cp, 0.0, 1.0).astype(np.float32)
        nn_t = np.where(np.arange(n) < ct, 0.0, 1.0).astype(np.float32)
        f, iou, P, R = syns_ref.f_iou(nn_p, nn_t)
        tp, tt = torch.from_numpy(nn_p).sqrt(), torch.from_numpy(nn_t).sqrt()
        Pt, Rt = (tp < 0.1).float().mean(), (tt < 0.1).float().mean()
        if (Pt < 1e-3) and (Rt < 1e-3):
            ft, it = Pt, Pt
        else:
            ft, it = 2 * Pt * Rt / (Pt + Rt), Pt * Rt / (Pt + Rt - (Pt * Rt))
        assert np.float32(f) == ft.numpy() or (np.isnan(f) and torch.isnan(ft)), (cp, ct, n)
        assert np.float32(iou) == it.numpy() or (np.isnan(iou) and torch.isnan(it)), (cp, ct, n)


# ------------------------------------------------------------------------------------------------ golden file
def test_golden_file_matches_port(be):
    """The committed expectations (tools/make_golden_syns.py: the float64 reference's edge maps, bit-packed, and its
    metrics) against the port on inputs regenerated from the seeds."""
    from baseboostdepth_amd.evaluation import pred_edges, image_view
    g = np.load(C.GOLDEN)
    for n in ("ramp_a", "ramp_b", "noise", "same_size"):
        depth, gt, ge = C.case_inputs(n)
        gts = _set([gt], [ge])
        edge, _ = pred_edges(torch.from_numpy(1.0 / depth)[None], gts, [0], pred_is_disp=True, backend=be)
        e = image_view(edge, gts, 0, 0).numpy().astype(bool)
        want = C.unpack_bits(g[n + "/edge_bits"], gt.shape)
        band = C.unpack_bits(g[n + "/band_bits"], gt.shape)
        assert band.mean() <= C.BAND_SHARE_CAP and not ((e != want) & ~band).any(), n


# ------------------------------------------------------------------------------------------------ dataset, options
def test_syns_dataset_paths_and_camera(tmp_path):
    from baseboostdepth_amd import datasets
    ds = datasets.SYNSRAWDataset(["01 5", "scene_b 0012"], 0, 192, 640, syns_path=str(tmp_path), is_train=False)
    assert ds.frame_paths(0) == {0: os.path.join(str(tmp_path), "images", "01", "5.png")}
    assert ds.frame_paths(1) == {0: os.path.join(str(tmp_path), "images", "scene_b", "0012.png")}
    K, inv_K = ds.K, ds.inv_K
    assert K.dtype == np.float32 and K.shape == (3, 3) and K[0, 2] == 621 and K[1, 2] == 188
    np.testing.assert_allclose(K[0, 0], 621 / np.tan(np.deg2rad(84.10) / 2), rtol=1e-6)
    np.testing.assert_allclose(K[1, 1], 188 / np.tan(np.deg2rad(25.46) / 2), rtol=1e-6)
    np.testing.assert_allclose(inv_K @ K, np.eye(3), atol=1e-5)
    Kr, iKr = syns_ref.syns_camera()
    assert np.array_equal(K, Kr) and np.array_equal(inv_K, iKr)
    with pytest.raises(ValueError):
        datasets.SYNSRAWDataset(["01 5"], 0, 192, 640, syns_path=str(tmp_path), is_train=True)


def test_syns_items_go_through_the_device_collate(tmp_path):
    """Evaluation items of the SYNS dataset have the form DeviceCollate / DeviceLoader take (host port of the image
    kernels): frame 0 at the network's size, one row per item, in split order."""
    from ports import PortBackend
    from baseboostdepth_amd import datasets
    lines = C.make_syns_tree(str(tmp_path), 3)
    ds = datasets.SYNSRAWDataset(lines, 0, 32, 64, syns_path=str(tmp_path), is_train=False, naive_mix=True)
    assert len(ds) == 3 and ds[1]["images"][0].shape == (94, 310, 3)
    loader = datasets.DeviceLoader(ds, 2, datasets.DeviceCollate(32, 64, [0], "cpu", PortBackend()), shuffle=False,
                                   drop_last=False, num_workers=2)
    shapes = [b[("color", 0, 0)].shape for b in loader]
    assert shapes == [(2, 3, 32, 64), (1, 3, 32, 64)]


def test_chamfer_parses_and_syns_eval_is_still_refused():
    from baseboostdepth_amd.options import MonodepthOptions
    o = MonodepthOptions().parse("--eval_mono --eval_split SYNS --chamfer --syns_path /data/syns".split())
    assert o.chamfer and o.eval_split == "SYNS" and o.syns_path == "/data/syns"
    assert not MonodepthOptions().parse([]).chamfer
    with pytest.raises(SystemExit):
        MonodepthOptions().parse(["--SYNS_eval"])


def test_ground_truth_set_without_edges_is_unchanged():
    from baseboostdepth_amd.evaluation import GroundTruthSet
    gt = [np.ones((4, 6), np.float32), np.ones((3, 5), np.float32)]
    a = GroundTruthSet(gt, "cpu")
    assert a.edges is None and a.desc.tolist()[1][:4] == [24, 0, 3, 5]
    b = GroundTruthSet(gt, "cpu", edges=[np.ones((4, 6, 1), bool), np.zeros((3, 5), np.uint8)])
    assert torch.equal(a.desc, b.desc) and b.edges.dtype == torch.uint8 and b.edges.tolist() == [1] * 24 + [0] * 15
