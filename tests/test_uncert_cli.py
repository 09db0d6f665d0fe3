"""The uncertainty options end to end: `evaluation.evaluate(..., uncertainty="post")` against the by-hand
composition post_process_uncert -> depth_metrics -> sparsification -> mean; the printed table and the JSON file; the
saved maps fed back through ext_disp_to_eval + ext_uncert_to_eval; the launches of a run without the new options; every
refusal before anything is touched; `test_simple.py --uncertainty`.  CPU tier on the host port, with the stand-in
networks of tests/test_gpu_postprocess.py; ONE test of the GPU tier repeats the composition on the device."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ports import PortBackend  # noqa: E402
from test_gpu_postprocess import Dec, Enc  # noqa: E402
from baseboostdepth_amd import evaluation, inference, ops  # noqa: E402
from baseboostdepth_amd.layers import disp_to_depth  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

H, W, BATCHES = 24, 80, (2, 2, 1)
SHAPES = [(40, 120), (38, 124), (40, 120), (36, 118), (40, 120)]
MIN_DEPTH, MAX_DEPTH, K = 0.1, 100.0, 20


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def _loader(device="cpu"):
    g = torch.Generator().manual_seed(5)
    return [{("color", 0, 0): torch.rand(n, 3, H, W, generator=g).to(device)} for n in BATCHES]


def _gts():
    rng = np.random.default_rng(8)
    gts = np.empty(len(SHAPES), dtype=object)
    for i, (gh, gw) in enumerate(SHAPES):
        g = (3.0 + 60.0 * rng.random((gh, gw))).astype(np.float32)
        g[rng.random((gh, gw)) < 0.6] = 0.0
        gts[i] = g
    gts[3][:] = 0.0                                       # an image without a scored pixel: named, left out of the mean
    return gts


def _opt(tmp_path, **kw):
    weights = tmp_path / "weights"
    weights.mkdir(exist_ok=True)
    opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, num_layers=18, kt_path=None,
                                load_weights_folder=str(weights), splits_dir=str(tmp_path / "splits"), eval_split="eigen",
                                disable_median_scaling=False, pred_depth_scale_factor=1, min_depth=MIN_DEPTH,
                                max_depth=MAX_DEPTH, height=H, width=W)
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _by_hand(loader, gts, backend, device):
    """(metrics rows, sparsification rows) of the split, composed call by call."""
    truth = evaluation.GroundTruthSet(gts, device)
    rows, spars, first = [], [], 0
    with torch.no_grad():
        for data in loader:
            x = data[("color", 0, 0)]
            raw = Dec()(Enc()(torch.cat((x, torch.flip(x, [3])), 0)))[("disp", 0)]
            disp, uncert = ops.post_process_uncert(disp_to_depth(raw, MIN_DEPTH, MAX_DEPTH)[0], backend=backend)
            idx = list(range(first, first + x.shape[0]))
            rows.append(evaluation.depth_metrics(disp, truth, idx, min_depth=1e-3, max_depth=80.0, pred_is_disp=True,
                                                 median="numpy", backend=backend))
            spars.append(ops.sparsification(disp, uncert, truth, idx, rows[-1], intervals=K, backend=backend))
            first += x.shape[0]
    return torch.cat(rows).cpu().numpy().astype(np.float64), torch.cat(spars).cpu().numpy()


def _check_against_composition(out, scores, printed, rows, spars):
    mean_errors, ratios = out
    assert np.array_equal(mean_errors, rows[:, :7].mean(0), equal_nan=True) and np.array_equal(ratios, rows[:, 7], equal_nan=True)
    want = evaluation.sparsification_scores(spars, K)
    assert want["images"] == 4 and want["skipped"] == [3] and want["intervals"] == K
    assert all(np.isfinite(list(want[name].values())).all() for name in ("ause", "aurg"))
    assert json.dumps(scores) == json.dumps(want)                     # the same numbers, digit for digit
    has = spars[:, 6] > 0
    assert np.array_equal(np.array(list(want["ause"].values())), spars[has, :3].mean(0))
    assert "WARNING: no scored pixel in 1 of 5 images, left out of the uncertainty scores: 3\n" in printed
    for name in ("ause", "aurg"):
        line = "  " + "{:>8} | ".format(name.upper()) + ("{: 8.4f} | " * 3).format(*want[name].values())
        assert line + "\n" in printed
    assert printed.index("abs_rel |   sq_rel |") < printed.index("AUSE")                  # after the metrics table
    assert "post_process is implied" in printed


def test_evaluate_equals_the_composition_and_round_trips(tmp_path, port, capsys):
    gts = _gts()
    opt = _opt(tmp_path, uncertainty="post", sparsification_intervals=K, save_pred_uncerts=True, save_pred_disps=True,
               save_sparsification=str(tmp_path / "spars.json"))
    port.calls.clear()
    mean_errors, ratios, scores = evaluation.evaluate(opt, dataloader=_loader(), gt_depths=gts, models=(Enc(), Dec()),
                                                      backend=port, device="cpu")
    assert port.calls == ["bbd_post_process_uncert", "bbd_depth_metrics", "bbd_sparsification"] * len(BATCHES)
    printed = capsys.readouterr().out
    rows, spars = _by_hand(_loader(), gts, port, "cpu")
    _check_against_composition((mean_errors, ratios), scores, printed, rows, spars)
    with open(tmp_path / "spars.json") as f:
        assert json.dumps(json.load(f)) == json.dumps(scores)
    assert len(scores["curves"]["sparse"]["abs_rel"]) == K + 1 and scores["fractions"][-1] == 1.0
    # the saved maps: what the flip pass gave, and fed back they reproduce the scores exactly
    folder = opt.load_weights_folder
    disps, uncerts = np.load(os.path.join(folder, "disps_eigen_split.npy")), np.load(os.path.join(folder, "uncerts_eigen_split.npy"))
    assert disps.shape == uncerts.shape == (5, H, W) and uncerts.dtype == np.float32 and (uncerts > 0).any()
    ext = _opt(tmp_path, ext_disp_to_eval=os.path.join(folder, "disps_eigen_split.npy"),
               ext_uncert_to_eval=os.path.join(folder, "uncerts_eigen_split.npy"), sparsification_intervals=K)
    ext.load_weights_folder = "None"
    for batch_size in (2, 3):
        port.calls.clear()
        again = evaluation.evaluate(ext, gt_depths=gts, batch_size=batch_size, backend=port, device="cpu")
        assert port.calls == ["bbd_depth_metrics", "bbd_sparsification"] * -(-5 // batch_size)
        assert np.array_equal(again[0], mean_errors, equal_nan=True) and np.array_equal(again[1], ratios, equal_nan=True)
        assert json.dumps(again[2]) == json.dumps(scores)


def test_without_the_new_options_the_launches_and_the_result_are_todays(tmp_path, port, capsys):
    gts = _gts()
    port.calls.clear()
    out = evaluation.evaluate(_opt(tmp_path), dataloader=_loader(), gt_depths=gts, models=(Enc(), Dec()), backend=port,
                              device="cpu")
    assert port.calls == ["bbd_depth_metrics"] * len(BATCHES) and len(out) == 2
    printed = capsys.readouterr().out
    assert "AUSE" not in printed and "uncertaint" not in printed.lower() and "abs_rel" in printed
    port.calls.clear()
    post = evaluation.evaluate(_opt(tmp_path, post_process=True, uncertainty="none", ext_uncert_to_eval=None),
                               dataloader=_loader(), gt_depths=gts, models=(Enc(), Dec()), backend=port, device="cpu")
    assert port.calls == ["bbd_post_process_disp", "bbd_depth_metrics"] * len(BATCHES) and len(post) == 2
    assert not os.listdir(_opt(tmp_path).load_weights_folder)
    # the blended disparities of the plain flip pass are the ones the uncertainty run scores
    with_uncert = evaluation.evaluate(_opt(tmp_path, uncertainty="post"), dataloader=_loader(), gt_depths=gts,
                                      models=(Enc(), Dec()), backend=port, device="cpu")
    assert np.array_equal(with_uncert[0], post[0], equal_nan=True) and np.array_equal(with_uncert[1], post[1], equal_nan=True)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError("nothing may be used before the refusal")


@pytest.mark.parametrize("change, word", [
    (dict(uncertainty="post", eval_split="SYNS"), "excludes eval_split SYNS"),
    (dict(uncertainty="post", no_eval=True), "excludes no_eval"),
    (dict(uncertainty="post", scale_recovery="ground"), "excludes scale_recovery ground"),
    (dict(uncertainty="post", ext_disp_to_eval="d.npy", ext_uncert_to_eval="u.npy"), "choose one"),
    (dict(ext_uncert_to_eval="u.npy"), "ext_disp_to_eval, which is not set"),
    (dict(uncertainty="post", ext_disp_to_eval="d.npy"), "runs none"),
    (dict(uncertainty="post", sparsification_intervals=0), "sparsification_intervals"),
    (dict(uncertainty="post", sparsification_intervals=101), "sparsification_intervals"),
    (dict(uncertainty="other"), "none or post"),
    (dict(save_pred_uncerts=True), "needs an uncertainty"),
    (dict(save_sparsification="s.json"), "needs an uncertainty"),
])
def test_refusals_happen_before_anything_is_touched(tmp_path, change, word, capsys):
    opt = _opt(tmp_path, **change)
    with pytest.raises(ValueError, match=word):
        evaluation.evaluate(opt, dataloader=Untouchable(), gt_depths=Untouchable(), models=(Untouchable(), Untouchable()),
                            backend=Untouchable(), device="cpu")
    argv = ["--eval_mono"]
    for k, v in change.items():
        argv += ["--" + k] + ([] if v is True else [str(v)])
    with pytest.raises(SystemExit):
        MonodepthOptions().parse(argv)
    if word != "none or post":                                        # (argparse's own choice check words that one)
        assert word in capsys.readouterr().err


def test_options_carry_the_uncertainty_flags():
    d = MonodepthOptions().parse(["--eval_mono"])
    assert (d.uncertainty, d.ext_uncert_to_eval, d.save_pred_uncerts, d.sparsification_intervals, d.save_sparsification) == \
        ("none", None, False, 50, None)
    o = MonodepthOptions().parse(["--eval_mono", "--uncertainty", "post", "--save_pred_uncerts", "--sparsification_intervals",
                                  "25", "--save_sparsification", "s.json"])
    assert (o.uncertainty, o.save_pred_uncerts, o.sparsification_intervals, o.save_sparsification) == ("post", True, 25, "s.json")
    e = MonodepthOptions().parse(["--eval_mono", "--ext_disp_to_eval", "d.npy", "--ext_uncert_to_eval", "u.npy"])
    assert e.ext_uncert_to_eval == "u.npy"
    with pytest.raises(SystemExit):
        MonodepthOptions().parse(["--eval_mono", "--eval_eigen_to_benchmark"])


def test_external_uncertainties_are_checked_like_the_disparities(tmp_path):
    np.save(tmp_path / "d.npy", np.ones((5, H, W), np.float32))
    for name, arr in (("two_dim.npy", np.ones((4, 5), np.float32)), ("other_shape.npy", np.ones((5, H, W + 1), np.float32)),
                      ("strings.npy", np.array([[["a"]]]))):
        np.save(tmp_path / name, arr)
        opt = _opt(tmp_path, ext_disp_to_eval=str(tmp_path / "d.npy"), ext_uncert_to_eval=str(tmp_path / name))
        with pytest.raises(ValueError, match="ext_uncert_to_eval"):
            evaluation.evaluate(opt, gt_depths=Untouchable(), backend=Untouchable(), device="cpu")


# ---------------------------------------------------------------------------------------------- test_simple.py
def _argv(src, dst, *more):
    return ["--image_path", str(src), "--save_path", str(dst), "--ext", "png", "--weights", "unused"] + list(more)


def test_test_simple_writes_the_uncertainty_at_the_pictures_size(tmp_path, port):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    sizes = {"a": (30, 100), "b": (41, 77)}
    for i, (name, size) in enumerate(sizes.items()):
        Image.fromarray(np.random.default_rng(i).integers(0, 256, size + (3,), dtype=np.uint8)).save(src / (name + ".png"))
    predictor = inference.DepthPredictor(Enc(), Dec(), H, W, "cpu", backend=port)
    port.calls.clear()
    inference.run_cli(inference.parse_args(_argv(src, dst, "--uncertainty", "--save_npy")), predictor=predictor)
    assert port.calls.count("bbd_post_process_uncert") == 1 and "bbd_post_process_disp" not in port.calls
    assert sorted(os.listdir(dst)) == ["a_Base.jpg", "a_Base_uncert.jpg", "a_disp.npy", "a_uncert.npy",
                                       "b_Base.jpg", "b_Base_uncert.jpg", "b_disp.npy", "b_uncert.npy"]
    want, _, _ = ops.disp_viz(predictor.last_uncert, list(sizes.values()), want_float=False, backend=port, raw=True)
    _, floats, _ = ops.disp_viz(predictor.last_uncert, list(sizes.values()), want_float=True, backend=port, raw=True)
    for i, (name, size) in enumerate(sizes.items()):
        picture = np.asarray(Image.open(dst / (name + "_Base_uncert.jpg")))
        assert picture.shape == size + (3,) and np.asarray(Image.open(dst / (name + "_Base.jpg"))).shape == size + (3,)
        assert np.abs(picture.astype(int) - want[i].numpy().astype(int)).mean() < 12          # the JPEG of that picture
        assert np.array_equal(np.load(dst / (name + "_uncert.npy")), floats[i].numpy()) and floats[i].max() > 0
    # the disparity beside it is the flip-blended one
    blended = predictor.predict([np.asarray(Image.open(src / "a.png"))], want_float=True, post_process=True)[0]
    assert np.array_equal(np.load(dst / "a_disp.npy"), blended.scaled_disp)
    assert inference.find_inputs(str(dst), "x", "jpg")[0] == []                # a second run skips its own outputs


def test_an_old_predictor_works_without_the_flag(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(src / "a.png")

    class Old:                                # the interface before this feature
        def predict(self, images, want_float=False):
            return [inference.DepthPrediction(np.zeros(im.shape, np.uint8), 1.0, 2.0) for im in images]

    inference.run_cli(inference.parse_args(_argv(src, tmp_path / "o")), predictor=Old())
    assert sorted(os.listdir(tmp_path / "o")) == ["a_Base.jpg"]
    assert inference.parse_args(_argv(src, "o")).uncertainty is False


# ---------------------------------------------------------------------------------------------- the device
@pytest.mark.gpu
def test_evaluate_equals_the_composition_on_the_device(tmp_path, capsys):
    dev, gts = "cuda:0", _gts()
    opt = _opt(tmp_path, uncertainty="post", sparsification_intervals=K)
    mean_errors, ratios, scores = evaluation.evaluate(opt, dataloader=_loader(dev), gt_depths=gts, models=(Enc(), Dec()),
                                                      device=dev)
    printed = capsys.readouterr().out
    rows, spars = _by_hand(_loader(dev), gts, None, dev)
    _check_against_composition((mean_errors, ratios), scores, printed, rows, spars)
