"""GPU tier of the depth evaluation's options: bbd_post_process_disp through `ops.post_process_disp`, and
`evaluation.evaluate` / `DepthPredictor.predict` with post_process, save_pred_disps, ext_disp_to_eval and no_eval on
synthetic KITTI and SYNS splits.  The reference of the blend is the literal numpy formulation (tests/postproc_ref.py,
computed live); the kernel's arithmetic is that float64 blend rounded once, so the tolerance is equality."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import postproc_ref  # noqa: E402
from oracle import eval_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N = 96, 320, 6
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0


def _close(got, want, rtol):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=rtol, atol=2e-6)


class Enc(torch.nn.Module):
    def forward(self, x):
        return x


class Dec(torch.nn.Module):
    """Pointwise, so a pixel's disparity has the same bits in any batch; the column ramp makes it differ from the
    prediction of the flipped image flipped back."""

    def forward(self, x):
        ramp = torch.linspace(0.35, 1.0, x.shape[3], device=x.device, dtype=x.dtype)
        mix = 0.6 * x[:, 0:1] - 0.3 * x[:, 1:2] + 0.5 * x[:, 2:3]
        return {("disp", 0): torch.sigmoid(3.0 * (mix - 0.4)) * ramp}


def _doubled(x):
    """The stub networks' scaled disparity for a batch and its flipped copy, [2n,h,w] float32 on the host."""
    from baseboostdepth_amd.layers import disp_to_depth
    with torch.no_grad():
        out = Dec()(Enc()(torch.cat((x, torch.flip(x, [3])), 0)))[("disp", 0)]
        return disp_to_depth(out, MIN_DEPTH, MAX_DEPTH)[0][:, 0].cpu().numpy()


# ---------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", postproc_ref.SHAPES + [(2, 192, 640)])
def test_kernel_equals_numpy_reference_and_repeats(shape):
    from baseboostdepth_amd import ops
    n, h, w = shape
    disp = postproc_ref.make_input(n, h, w, seed=100 + w)
    want = postproc_ref.reference(disp)
    x = torch.from_numpy(disp).to(DEV)
    got = ops.post_process_disp(x)
    again = ops.post_process_disp(x[:, None])                      # [2n,1,h,w], a second call on the same input
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, h, w)
    got, again = got.cpu().numpy(), again.cpu().numpy()
    print("%s: max |kernel - reference| = %.3g" % (shape, float(np.abs(got - want).max())))
    assert np.array_equal(got, want)
    assert got.tobytes() == again.tobytes()
    assert np.array_equal(x.cpu().numpy(), disp)                   # the input is left alone


# ---------------------------------------------------------------------------- evaluate, KITTI branch
@pytest.fixture(scope="module")
def kitti(tmp_path_factory):
    """A synthetic KITTI split of 6 images with ragged ground truth, scored once plain and once with post_process +
    save_pred_disps (batch_size 4: the last batch is short)."""
    import image_checks
    from baseboostdepth_amd import evaluation
    root = tmp_path_factory.mktemp("postprocess_kitti")
    lines = image_checks.make_kitti_tree(str(root / "kitti"), frames=18)
    test_files = [l.rsplit(" ", 2)[0] for l in lines][:N]
    assert len(test_files) == N
    split = root / "splits" / "eigen"
    split.mkdir(parents=True)
    (split / "test_files.txt").write_text("\n".join(test_files) + "\n")
    g = torch.Generator().manual_seed(16)
    gts = np.empty(N, dtype=object)
    for i in range(N):
        gh, gw = (375, 1242) if i % 2 else (370, 1226)
        gts[i] = (torch.rand(gh, gw, generator=g) * 85 * (torch.rand(gh, gw, generator=g) < 0.06)).numpy().astype(np.float32)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    weights = root / "weights"
    weights.mkdir()
    opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, num_layers=18, kt_path=str(root / "kitti"),
                                load_weights_folder=str(weights), splits_dir=str(root / "splits"), eval_split="eigen",
                                disable_median_scaling=False, pred_depth_scale_factor=1, min_depth=MIN_DEPTH,
                                max_depth=MAX_DEPTH, num_workers=2, height=H, width=W)
    plain = evaluation.evaluate(opt, models=(Enc(), Dec()), batch_size=4)
    saved = weights / "disps_eigen_split.npy"
    assert not saved.exists()                                      # nothing is written without the flag
    opt.post_process, opt.save_pred_disps = True, True
    post = evaluation.evaluate(opt, models=(Enc(), Dec()), batch_size=4)
    return types.SimpleNamespace(root=root, opt=opt, test_files=test_files, gts=gts, plain=plain, post=post, saved=saved,
                                 split=split)


def test_evaluate_post_process_saves_the_scored_disparities(kitti):
    from baseboostdepth_amd import datasets
    disps = np.load(kitti.saved)
    assert disps.dtype == np.float32 and disps.shape == (N, H, W)
    ds = datasets.KITTIRAWDataset(kitti.test_files, 0, H, W, kt_path=kitti.opt.kt_path, is_train=False, kt=True,
                                  naive_mix=True)
    coll = datasets.DeviceCollate(H, W, [0], DEV)
    for i in range(N):
        want = postproc_ref.reference(_doubled(coll([ds[i]])[("color", 0, 0)]))
        assert np.array_equal(disps[i], want[0]), "image %d" % i
    mean_errors, ratios = kitti.post
    want = [eval_ref.evaluate_image_ref(disps[i], kitti.gts[i]) for i in range(N)]
    print("evaluate:", mean_errors, "reference:", np.mean([w["metrics"] for w in want], 0))
    _close(mean_errors, np.mean([w["metrics"] for w in want], 0), rtol=2e-4)
    _close(ratios, [w["ratio"] for w in want], rtol=2e-4)
    plain_errors, plain_ratios = kitti.plain
    assert not np.array_equal(mean_errors, plain_errors) and not np.array_equal(ratios, plain_ratios)


def test_saved_file_round_trip_scores_identically(kitti, tmp_path):
    """ext_disp_to_eval on the file just written: no weights folder, no KITTI tree, the same numbers exactly."""
    from baseboostdepth_amd import evaluation
    opt = types.SimpleNamespace(**vars(kitti.opt))
    opt.ext_disp_to_eval, opt.load_weights_folder, opt.kt_path = str(kitti.saved), "None", str(tmp_path / "no_such_tree")
    assert not os.path.exists(opt.kt_path)
    mean_errors, ratios = evaluation.evaluate(opt, batch_size=4)
    assert np.array_equal(mean_errors, kitti.post[0]) and np.array_equal(ratios, kitti.post[1])
    other_batching = evaluation.evaluate(opt, batch_size=5)
    assert np.array_equal(other_batching[0], mean_errors) and np.array_equal(other_batching[1], ratios)
    short = tmp_path / "short.npy"
    np.save(short, np.load(kitti.saved)[:N - 1])
    opt.ext_disp_to_eval = str(short)
    with pytest.raises(ValueError):
        evaluation.evaluate(opt, batch_size=4)


def test_no_eval_predicts_saves_and_stops(kitti, tmp_path, capsys):
    from baseboostdepth_amd import evaluation
    split = tmp_path / "splits" / "eigen"
    split.mkdir(parents=True)
    (split / "test_files.txt").write_text("\n".join(kitti.test_files) + "\n")       # no gt_depths.npz here
    weights = tmp_path / "weights"
    weights.mkdir()
    opt = types.SimpleNamespace(**vars(kitti.opt))
    opt.splits_dir, opt.load_weights_folder, opt.no_eval = str(tmp_path / "splits"), str(weights), True
    capsys.readouterr()
    assert evaluation.evaluate(opt, models=(Enc(), Dec()), batch_size=4) == (None, None)
    printed = capsys.readouterr().out
    assert "abs_rel" not in printed and "Scaling ratios" not in printed
    assert np.array_equal(np.load(weights / "disps_eigen_split.npy"), np.load(kitti.saved))


# ---------------------------------------------------------------------------- evaluate, SYNS branch
def test_syns_branch_post_process_save_and_round_trip(tmp_path, capsys):
    import syns_checks
    from baseboostdepth_amd import datasets, evaluation
    h, w, n, gh, gw = 64, 192, 3, 94, 310
    lines = syns_checks.make_syns_tree(str(tmp_path / "syns"), n, gh, gw)
    split = tmp_path / "splits" / "SYNS"
    split.mkdir(parents=True)
    (split / "test_files.txt").write_text("\n".join(lines) + "\n")
    gts, edges = np.empty(n, dtype=object), np.empty(n, dtype=object)
    for i in range(n):
        gts[i], edges[i] = syns_checks.make_gt(80 + i, gh - (i % 2), gw)
    np.savez_compressed(split / "gt_depths.npz", data=gts)
    np.savez_compressed(split / "gt_edges.npz", data=edges)
    weights = tmp_path / "weights"
    weights.mkdir()
    opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, num_layers=18, kt_path=None,
                                syns_path=str(tmp_path / "syns"), chamfer=False, load_weights_folder=str(weights),
                                splits_dir=str(tmp_path / "splits"), eval_split="SYNS", disable_median_scaling=False,
                                pred_depth_scale_factor=1, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, num_workers=2,
                                height=h, width=w, post_process=True, save_pred_disps=True)
    mean_errors, ratios = evaluation.evaluate(opt, models=(Enc(), Dec()), batch_size=2)
    printed = capsys.readouterr().out
    assert mean_errors.shape == (7,) and ratios.shape == (n,) and "edge_comp" in printed
    assert np.isfinite(mean_errors).all()
    disps = np.load(weights / "disps_SYNS_split.npy")
    assert disps.dtype == np.float32 and disps.shape == (n, h, w)
    ds = datasets.SYNSRAWDataset(lines, 0, h, w, syns_path=str(tmp_path / "syns"), is_train=False, naive_mix=True)
    coll = datasets.DeviceCollate(h, w, [0], DEV)
    for i in range(n):
        assert np.array_equal(disps[i], postproc_ref.reference(_doubled(coll([ds[i]])[("color", 0, 0)]))[0])
    opt.post_process = opt.save_pred_disps = False
    plain_errors, _ = evaluation.evaluate(opt, models=(Enc(), Dec()), batch_size=2)
    assert not np.array_equal(plain_errors, mean_errors)
    ext = types.SimpleNamespace(**vars(opt))
    ext.ext_disp_to_eval, ext.load_weights_folder, ext.syns_path = str(weights / "disps_SYNS_split.npy"), "None", None
    again_errors, again_ratios = evaluation.evaluate(ext, batch_size=2)
    assert np.array_equal(again_errors, mean_errors) and np.array_equal(again_ratios, ratios)


# ---------------------------------------------------------------------------- the predictor
def test_predictor_post_process_blends_the_raw_disparities():
    from baseboostdepth_amd.inference import DepthPredictor

    def _synthetic_image(seed, h, w):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * 255 // (w - 1)), (yy * 255 // (h - 1)), ((xx + yy) % 256)], -1)
        return np.clip(base + rng.integers(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)

    pred = DepthPredictor(Enc(), Dec(), 64, 128, DEV, batch_size=3)       # 4 network rows: two network batches
    images = [_synthetic_image(1, 75, 230), _synthetic_image(2, 120, 161)]
    plain = pred.predict(images)
    assert tuple(pred.last_disp.shape) == (2, 1, 64, 128)
    post = pred.predict(images, post_process=True)
    blended = pred.last_disp
    assert blended.dtype == torch.float32 and tuple(blended.shape) == (2, 64, 128)
    x = pred.prepare(images)
    with torch.no_grad():
        raw = Dec()(Enc()(torch.cat((x, torch.flip(x, [3])), 0)))[("disp", 0)]
    assert np.array_equal(blended.cpu().numpy(), postproc_ref.reference(raw[:, 0].cpu().numpy()))
    for im, a, b in zip(images, plain, post):
        assert b.color.shape == im.shape and b.color.dtype == np.uint8
        assert not np.array_equal(a.color, b.color)
