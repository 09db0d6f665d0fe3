"""GPU tier of the SYNS-Patches metrics (bbd_syns.hip through the C ABI): every kernel against the committed
expectations (tests/golden/syns_cases.npz) and against the numpy reference (tests/syns_ref.py) run live on fresh seeds,
under the rules of tests/syns_checks.py; ragged batches, a full-size 376x1242 image, repeatability, and the Trainer /
evaluate() plumbing on synthetic splits."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import syns_checks as C  # noqa: E402
import syns_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set(gts, edges):
    from baseboostdepth_amd.evaluation import GroundTruthSet
    return GroundTruthSet(gts, torch.device(DEV), crop=False, edges=edges)


def _close(got, want, rtol=3e-5):                  # the tolerance of tests/test_gpu_eval.py
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=rtol, atol=2e-6)


def _score(names, mode, chamfer_rays=None):
    """One ragged launch chain over the named cases (equal prediction size).  Returns per-case dicts."""
    from baseboostdepth_amd.evaluation import (depth_metrics, pred_edges, edge_metrics, pointcloud_metrics, image_view)
    ins = [C.case_inputs(n) for n in names]
    gts = _set([i[1] for i in ins], [i[2] for i in ins])
    depth = np.stack([i[0] for i in ins])
    ev = mode == "evaluate"
    pred = torch.from_numpy(1.0 / depth if ev else depth).float().to(DEV)
    idx = list(range(len(names)))
    lo, hi = C.depth_range(mode)
    rows = depth_metrics(pred, gts, idx, min_depth=float(lo), max_depth=float(hi), pred_is_disp=ev,
                         median="numpy" if ev else "torch")
    edge, stats = pred_edges(pred, gts, idx, pred_is_disp=ev)
    em = edge_metrics(pred, gts, idx, edge, rows, min_depth=float(lo), max_depth=float(hi), pred_is_disp=ev)
    pcs = {}
    for rays in chamfer_rays or ():
        pcs[rays] = pointcloud_metrics(pred, gts, idx, rows, syns_ref.syns_camera()[1], min_depth=float(lo),
                                       max_depth=float(hi), pred_is_disp=ev, rays=rays).cpu().numpy()
    out = []
    for i, n in enumerate(names):
        out.append(dict(name=n, depth=ins[i][0], gt=ins[i][1], gt_edge=ins[i][2], pred=pred[i].cpu().numpy(),
                        edge=image_view(edge, gts, i, i).cpu().numpy(), stats=stats[i].cpu().numpy(),
                        em=em[i].cpu().numpy(), rows=rows[i].cpu().numpy(), pc={r: v[i] for r, v in pcs.items()}))
    return out


@pytest.mark.parametrize("mode", ["evaluate", "trainer"])
@pytest.mark.parametrize("names", [["ramp_a", "ramp_b"], ["noise"], ["same_size"], ["full"]])
def test_edges_and_metrics_match_golden_and_live_reference(names, mode):
    """ramp_a + ramp_b: two ground-truth sizes in ONE launch.  full: 376x1242."""
    g = np.load(C.GOLDEN)
    for r in _score(names, mode):
        n, gt = r["name"], r["gt"]
        key = n if mode == "evaluate" else n + "/trainer"
        # golden: the float64 reference's map, outside its rounding band
        want, band = C.unpack_bits(g[key + "/edge_bits"], gt.shape), C.unpack_bits(g[key + "/band_bits"], gt.shape)
        e = r["edge"].astype(bool)
        assert band.mean() <= C.BAND_SHARE_CAP and not ((e != want) & ~band).any(), key
        assert int(r["stats"][1]) == int(e.sum())
        gm = g[key + "/metrics"]
        if np.array_equal(e, want):                   # same map: the golden metrics apply as they are
            assert [int(c) for c in r["em"][3:7]] == [int(c) for c in gm[3:7]], key
            np.testing.assert_allclose(r["em"][:2], gm[:2], rtol=C.METRIC_RTOL, atol=0)
        _close(r["em"][2], gm[2])
        _close(r["rows"][7], gm[7], rtol=2e-6)
        # live reference
        at_gt = C.resized(r["pred"], *gt.shape, mode)
        C.check_edge_map(r["edge"], at_gt, key)
        _, want_err = C.check_edge_metrics(r["em"], r["edge"], at_gt, gt, r["gt_edge"], mode, what=key)
        _close(r["em"][2], want_err)


def test_fresh_seeds_both_modes():
    from baseboostdepth_amd.evaluation import depth_metrics, pred_edges, edge_metrics, image_view
    for seed, (h, w, gh, gw) in ((101, (40, 120, 83, 251)), (102, (64, 64, 50, 70))):
        depth = np.stack([C.make_depth(seed, h, w), C.make_depth(seed + 50, h, w, "noise")])
        gt = [C.make_gt(seed, gh, gw), C.make_gt(seed + 1, gh - 3, gw + 5)]
        gts = _set([g[0] for g in gt], [g[1] for g in gt])
        for mode in ("evaluate", "trainer"):
            ev = mode == "evaluate"
            lo, hi = C.depth_range(mode)
            pred = torch.from_numpy(1.0 / depth if ev else depth).float().to(DEV)
            rows = depth_metrics(pred, gts, [0, 1], min_depth=float(lo), max_depth=float(hi), pred_is_disp=ev,
                                 median="numpy" if ev else "torch")
            edge, _ = pred_edges(pred, gts, [0, 1], pred_is_disp=ev)
            em = edge_metrics(pred, gts, [0, 1], edge, rows, min_depth=float(lo), max_depth=float(hi), pred_is_disp=ev).cpu().numpy()
            for i in range(2):
                at_gt = C.resized(pred[i].cpu().numpy(), *gt[i][0].shape, mode)
                e = image_view(edge, gts, i, i).cpu().numpy()
                C.check_edge_map(e, at_gt, "seed %d %s %d" % (seed, mode, i))
                _, want_err = C.check_edge_metrics(em[i], e, at_gt, gt[i][0], gt[i][1], mode, what="seed %d" % seed)
                _close(em[i, 2], want_err)


def test_distance_transform_bit_equal():
    from baseboostdepth_amd.evaluation import distance_transform, syns_strides, image_view
    g = np.load(C.GOLDEN)
    seed, hh, ww = (int(v) for v in g["edt/seed"])
    rng = np.random.default_rng(31)
    maps = [np.random.default_rng(seed).random((hh, ww)) < 0.004, rng.random((376, 1242)) < 2e-5,
            rng.random((61, 1030)) < 0.01, np.zeros((9, 300), bool), np.ones((3, 3), bool)]
    maps[2][:, :600] = False                           # distances beyond one 256-lane round of the row pass
    gts = _set([np.ones(m.shape, np.float32) for m in maps], None)
    _, _, stride = syns_strides(gts)
    buf = torch.zeros(len(maps), stride, dtype=torch.uint8)
    for i, m in enumerate(maps):
        buf[i, :m.size] = torch.from_numpy(m.reshape(-1).astype(np.uint8))
    out = distance_transform(buf.to(DEV), gts, list(range(len(maps))))
    again = distance_transform(buf.to(DEV), gts, list(range(len(maps))))
    assert torch.equal(out, again)
    assert np.array_equal(image_view(out, gts, 0, 0).cpu().numpy(), g["edt/sq"])
    for i, m in enumerate(maps):
        assert np.array_equal(image_view(out, gts, i, i).cpu().numpy(), syns_ref.edt_sq(m)), i
    one = distance_transform(buf[1:2].to(DEV), gts, [1])
    assert torch.equal(one[0], out[1])


def test_nearest_neighbour_bit_equal_golden_and_fresh():
    from baseboostdepth_amd import ops
    g = np.load(C.GOLDEN)
    seed, na, nb = (int(v) for v in g["nn/seed"])
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((na, 3)) * 4).astype(np.float32)
    b = (rng.standard_normal((nb, 3)) * 4).astype(np.float32)
    nn_a, nn_b = ops.chamfer_nn(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert np.array_equal(nn_a.cpu().numpy().view(np.uint32), g["nn/a"].view(np.uint32))
    assert np.array_equal(nn_b.cpu().numpy().view(np.uint32), g["nn/b"].view(np.uint32))
    rng = np.random.default_rng(5)
    for na, nb in ((1, 1), (2049, 1025), (5000, 9001)):          # partial query blocks, partial target tiles
        a = (rng.standard_normal((na, 3)) * 5).astype(np.float32)
        b = (rng.standard_normal((nb, 3)) * 5).astype(np.float32)
        b[: min(na, nb) // 2] = a[: min(na, nb) // 2]
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        nn_a, nn_b = ops.chamfer_nn(ta, tb)
        assert np.array_equal(nn_a.cpu().numpy().view(np.uint32), syns_ref.nn_sq(a, b).view(np.uint32))
        assert np.array_equal(nn_b.cpu().numpy().view(np.uint32), syns_ref.nn_sq(b, a).view(np.uint32))
        again = ops.chamfer_nn(ta, tb)
        assert torch.equal(again[0], nn_a) and torch.equal(again[1], nn_b)
    nn_a, nn_b = ops.chamfer_nn(ta, torch.zeros(0, 3, device=DEV))
    assert torch.isinf(nn_a).all() and nn_b.numel() == 0


def test_nearest_neighbour_full_size_subset():
    """Two clouds of 376 * 1242 points: about 2,000 seeded queries against numpy over ALL targets, both ways."""
    from baseboostdepth_amd import ops
    n = 376 * 1242
    rng = np.random.default_rng(9)
    a = (rng.random((n, 3)) * np.array([40, 10, 60]) - np.array([20, 5, 0])).astype(np.float32)
    b = (a + 0.05 * rng.standard_normal((n, 3))).astype(np.float32)[rng.permutation(n)]
    nn_a, nn_b = ops.chamfer_nn(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    pick = np.sort(rng.choice(n, 2000, replace=False))
    assert np.array_equal(nn_a.cpu().numpy()[pick].view(np.uint32), syns_ref.nn_sq(a[pick], b, chunk=64).view(np.uint32))
    assert np.array_equal(nn_b.cpu().numpy()[pick].view(np.uint32), syns_ref.nn_sq(b[pick], a, chunk=64).view(np.uint32))


def test_pointcloud_metrics_equal_float32_reference():
    g = np.load(C.GOLDEN)
    inv_K = syns_ref.syns_camera()[1]
    for names in (["ramp_a", "ramp_b"], ["noise"], ["same_size"]):
        for r in _score(names, "evaluate", chamfer_rays=("reference", "pixel")):
            at_gt = C.resized(r["pred"], *r["gt"].shape, "evaluate")
            # the device's own ratio (an ulp from numpy's at most, see test_gpu_eval.py) defines the clouds
            lo, hi = C.depth_range("evaluate")
            p = np.clip((at_gt * np.float32(r["rows"][7])).astype(np.float32), lo, hi)
            for rays in ("reference", "pixel"):
                f, iou, P, R, nn_p, nn_t = syns_ref.pointcloud_metrics(p, r["gt"], inv_K, lo, hi, rays)
                got = r["pc"][rays]
                print(r["name"], rays, "got", got, "want", f, iou, P, R, len(nn_p))
                assert got[6] == len(nn_p) and got[4] == (np.sqrt(nn_p) < np.float32(0.1)).sum()
                assert got[5] == (np.sqrt(nn_t) < np.float32(0.1)).sum()
                assert np.array_equal(got[:4].view(np.uint32), np.array([f, iou, P, R], np.float32).view(np.uint32))
                gold = g[r["name"] + "/cloud_" + rays]
                assert got[6] == gold[4]
                if np.float32(r["rows"][7]) == np.float32(g[r["name"] + "/metrics"][7]):   # same ratio: same clouds
                    assert np.array_equal(got[:4].view(np.uint32), gold[:4].view(np.uint32))


def test_pointcloud_small_precision_branch_and_empty_cloud():
    from baseboostdepth_amd.evaluation import depth_metrics, pointcloud_metrics
    rng = np.random.default_rng(2)
    gt = (4.0 + 6.0 * rng.random((24, 40))).astype(np.float32)
    gt[rng.random((24, 40)) > 0.6] = 0.0
    gts = _set([gt, np.zeros((24, 40), np.float32)], None)
    pred = torch.from_numpy(np.stack([1.0 / (gt * 3 + 20), np.full((24, 40), 0.1, np.float32)])).float().to(DEV)
    rows = depth_metrics(pred, gts, [0, 1], min_depth=1e-3, max_depth=125.0, pred_is_disp=True, median="numpy",
                         median_scaling=False)
    got = pointcloud_metrics(pred, gts, [0, 1], rows, syns_ref.syns_camera()[1], pred_is_disp=True,
                             median_scaling=False).cpu().numpy()
    assert got[0, 2] == 0 and got[0, 3] == 0 and got[0, 0] == 0 and got[0, 1] == 0 and got[0, 6] == (gt > 0).sum()
    assert got[1, 6] == 0 and np.isnan(got[1, :4]).all()             # the mean of nothing, as in the reference


def test_identical_calls_identical_bytes_and_batch_equals_single():
    from baseboostdepth_amd.evaluation import syns_metrics
    names = ["ramp_a", "ramp_b"]
    ins = [C.case_inputs(n) for n in names]
    gts = _set([i[1] for i in ins], [i[2] for i in ins])
    pred = torch.from_numpy(np.stack([1.0 / i[0] for i in ins])).float().to(DEV)
    inv_K = syns_ref.syns_camera()[1]
    a = syns_metrics(pred, gts, [0, 1], inv_K=inv_K, chamfer=True)
    b = syns_metrics(pred, gts, [0, 1], inv_K=inv_K, chamfer=True)
    assert a.shape == (2, 9) and a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.isfinite(a).all()
    for i in range(2):
        one = syns_metrics(pred[i:i + 1], gts, [i], inv_K=inv_K, chamfer=True)
        assert torch.equal(one[0].view(torch.int64), a[i].view(torch.int64)), i
    swapped = syns_metrics(pred.flip(0).contiguous(), gts, [1, 0], inv_K=inv_K, chamfer=True)
    assert torch.equal(swapped.flip(0).view(torch.int64), a.view(torch.int64))
    t = syns_metrics(1.0 / pred, gts, [0, 1], mode="trainer")
    assert torch.isnan(t[:, 7:]).all() and torch.isfinite(t[:, :7]).all()


def test_trainer_syns_losses_and_val_syns():
    """Trainer.compute_depth_losses(SYNS=True) with the reference's (outputs, losses, idx, accumulate) convention and
    val_syns on a synthetic split, against the reference on the depths the same networks produce."""
    from test_gpu_trainer import make_opt
    from baseboostdepth_amd.trainer import Trainer
    from baseboostdepth_amd.evaluation import pred_edges, image_view
    tr = Trainer(make_opt(64, 128, 2, [0, 1, 2, 3], False))
    gt = [C.make_gt(40 + i, 90, 200) for i in range(4)]
    with pytest.raises(RuntimeError):
        tr.compute_depth_losses({("depth", 0, 0): torch.ones(1, 1, 64, 128, device=DEV)}, {}, 0, SYNS=True)
    tr.set_ground_truth_syns([g[0] for g in gt], [g[1] for g in gt])
    g = torch.Generator().manual_seed(4)
    batches = [{("color", 0, 0): torch.rand(2, 3, 64, 128, generator=g)} for _ in range(2)]
    assert not hasattr(tr, "best_syns")
    result = tr.val_syns(batches)
    assert set(result) == {"edge_Acc", "edge_comp"} and tr.best_syns == result["edge_comp"]
    tr.set_eval()
    want = np.zeros(2)
    with torch.no_grad():
        for bi, b in enumerate(batches):
            out, _ = tr.process_batch(dict(b), is_train=False)
            edge, _ = pred_edges(out["depth", 0, 0], tr.gt_syns, [2 * bi, 2 * bi + 1])
            for r in range(2):
                i = 2 * bi + r
                at_gt = C.resized(out["depth", 0, 0][r, 0].cpu().numpy(), 90, 200, "trainer")
                e = image_view(edge, tr.gt_syns, i, r).cpu().numpy()
                C.check_edge_map(e, at_gt, "val image %d" % i, cap=None)
                m = syns_ref.edge_metrics(e, gt[i][0], gt[i][1], np.float32(1e-3), np.float32(80.0))
                want += [m["edge_Acc"], m["edge_comp"]]
    np.testing.assert_allclose([result["edge_Acc"], result["edge_comp"]], want / 4, rtol=C.METRIC_RTOL)
    losses = {}
    tr.compute_depth_losses(out, losses, [2, 3], SYNS=True)
    assert set(losses) == {"edge_Acc", "edge_comp"} and losses["edge_comp"].is_cuda and losses["edge_comp"].dim() == 0
    first = float(losses["edge_comp"])
    tr.compute_depth_losses(out, losses, [2, 3], SYNS=True, accumulate=True)
    assert float(losses["edge_comp"]) == 2 * first
    tr.best_syns = 0.0
    tr.val_syns(batches)
    assert tr.best_syns == 0.0                          # only an improvement replaces it


@pytest.mark.parametrize("chamfer", [False, True])
def test_evaluate_syns_split_end_to_end(tmp_path, capsys, chamfer):
    """evaluation.evaluate on a synthetic SYNS tree (PNGs written by Pillow, split lines `folder frame`,
    gt_depths.npz + gt_edges.npz in the split directory) == the reference per image on the same disparities."""
    from test_gpu_trainer import make_opt
    from baseboostdepth_amd import datasets, evaluation
    from baseboostdepth_amd.layers import disp_to_depth
    from baseboostdepth_amd.trainer import Trainer
    H, W, n, gh, gw = 64, 192, 5, 94, 310
    lines = C.make_syns_tree(str(tmp_path / "syns"), n, gh, gw)
    split = tmp_path / "splits" / "SYNS"
    split.mkdir(parents=True)
    (split / "test_files.txt").write_text("\n".join(lines) + "\n")
    gts, edges = np.empty(n, dtype=object), np.empty(n, dtype=object)
    for i in range(n):
        gts[i], edges[i] = C.make_gt(60 + i, gh - (i % 2), gw)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    np.savez_compressed(split / "gt_edges.npz", data=edges)
    opt = make_opt(H, W, 2, [0, 1, 2, 3], False)
    opt.log_dir, opt.model_name = str(tmp_path), "m"
    tr = Trainer(opt)
    tr.save_model("w")
    eopt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, num_layers=18, kt_path=None,
                                 syns_path=str(tmp_path / "syns"), chamfer=chamfer,
                                 load_weights_folder=str(tmp_path / "m" / "models" / "weights_w"),
                                 splits_dir=str(tmp_path / "splits"), eval_split="SYNS", disable_median_scaling=False,
                                 pred_depth_scale_factor=1, min_depth=0.1, max_depth=100.0, num_workers=2, height=H, width=W)
    mean_errors, ratios = evaluation.evaluate(eopt, batch_size=2)
    printed = capsys.readouterr().out
    ncol = 9 if chamfer else 7
    assert mean_errors.shape == (ncol,) and ratios.shape == (n,) and "edge_comp" in printed
    assert ("iou1" in printed) == chamfer
    ds = datasets.SYNSRAWDataset(lines, 0, H, W, syns_path=str(tmp_path / "syns"), is_train=False, naive_mix=True)
    coll = datasets.DeviceCollate(H, W, [0], DEV)
    gset = _set(list(gts), list(edges))
    lo, hi = C.depth_range("evaluate")
    inv_K = syns_ref.syns_camera()[1]

    def reference(disp_of, ratios_dev, strict_edges):
        """Per image on the disparity `disp_of(x)`: the KITTI-style columns from numpy alone; the edge columns from the
        reference's metrics on the device's own edge map; the clouds with the ratio the device found."""
        want, want_ratio = [], []
        with torch.no_grad():
            for i in range(n):
                disp = disp_of(coll([ds[i]])[("color", 0, 0)])
                at_gt = C.resized(disp[0, 0].cpu().numpy(), *gts[i].shape, "evaluate")
                p, ratio = C.scaled(at_gt, gts[i], "evaluate")
                m = (gts[i] > lo) & (gts[i] < hi)
                k = eval_errors(gts[i][m], p[m])
                edge, _ = evaluation.pred_edges(disp, gset, [i], pred_is_disp=True)
                e = evaluation.image_view(edge, gset, i, 0).cpu().numpy()
                C.check_edge_map(e, at_gt, "image %d" % i, cap=None)
                em = syns_ref.edge_metrics(e, gts[i], edges[i], lo, hi)
                row = [k[0], syns_ref.err(p, gts[i], lo, hi), k[1], k[2], k[3], em["edge_Acc"], em["edge_comp"]]
                if chamfer and strict_edges:
                    pd = np.clip((at_gt * np.float32(ratios_dev[i])).astype(np.float32), lo, hi)
                    row += [float(v) for v in syns_ref.pointcloud_metrics(pd, gts[i], inv_K, lo, hi)[:2]]
                want.append(row)
                want_ratio.append(ratio)
        return np.mean(np.asarray(want, np.float64), 0), want_ratio

    # (a) the weights folder: convolutions may round differently per batch size (as in test_gpu_eval.py), so the
    #     KITTI-style columns and ratios are compared with its tolerance and the edge columns for their range only
    tr.set_eval()
    want, want_ratio = reference(
        lambda x: disp_to_depth(tr.models["depth"](tr.models["encoder"](x))[("disp", 0)], 0.1, 100.0)[0], ratios, False)
    print("evaluate:", mean_errors, "reference:", want)
    _close(mean_errors[:5], want[:5], rtol=2e-4)
    _close(ratios, want_ratio, rtol=2e-4)
    assert np.isfinite(mean_errors).all() and (mean_errors[5:7] >= 0).all() and (mean_errors[5:7] <= 10).all()

    # (b) an injected pointwise "network": its disparity has the same bits whatever the batch, so every column is held
    #     to its rule - edge columns against the reference on the device's own map, F-score / IoU equal
    class Enc(torch.nn.Module):
        def forward(self, x):
            return x

    class Dec(torch.nn.Module):
        def forward(self, x):
            return {("disp", 0): torch.sigmoid(4.0 * (x.mean(1, keepdim=True) - 0.5))}

    mean_b, ratios_b = evaluation.evaluate(eopt, models=(Enc(), Dec()), batch_size=2)
    dec = Dec()
    want, want_ratio = reference(lambda x: disp_to_depth(dec(x)[("disp", 0)], 0.1, 100.0)[0], ratios_b, True)
    print("evaluate (pointwise):", mean_b, "reference:", want)
    _close(mean_b[:5], want[:5], rtol=2e-4)
    _close(ratios_b, want_ratio, rtol=2e-4)
    np.testing.assert_allclose(mean_b[5:7], want[5:7], rtol=C.METRIC_RTOL)
    if chamfer:                      # float32 values that are equal image by image: their float64 means agree
        np.testing.assert_allclose(mean_b[7:], want[7:], rtol=1e-12, atol=0)


def eval_errors(gt, pred):
    from oracle import eval_ref
    return eval_ref.compute_errors_ref(gt, pred)
