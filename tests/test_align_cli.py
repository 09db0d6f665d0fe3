"""CPU tier of `evaluate_depth.py --scale_recovery lsq`: the options and what they refuse, and the
evaluation of a synthetic KITTI split whose disparities are another affine gauge of the truth, the kernels replaced by
their host ports (tests/ports.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_checks as A  # noqa: E402
from baseboostdepth_amd import evaluation, options  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


def _parse(*argv):
    return MonodepthOptions().parse(["--eval_mono"] + [str(a) for a in argv])


REFUSED = [(("--disable_median_scaling",), dict(disable_median_scaling=True), "disable_median_scaling"),
           (("--pred_depth_scale_factor", 2), dict(pred_depth_scale_factor=2.0), "pred_depth_scale_factor"),
           (("--eval_split", "SYNS"), dict(eval_split="SYNS"), "eval_split SYNS"),
           (("--save_clouds", "somewhere"), dict(save_clouds="somewhere"), "save_clouds"),
           (("--uncertainty", "post"), dict(uncertainty="post"), "uncertainty"),
           (("--ext_disp_to_eval", "d.npy", "--ext_uncert_to_eval", "u.npy"),
            dict(ext_disp_to_eval="d.npy", ext_uncert_to_eval="u.npy"), "ext_uncert_to_eval")]


def test_options(capsys):
    assert _parse().scale_recovery == "median"
    assert _parse("--scale_recovery", "lsq").scale_recovery == "lsq"
    _parse("--scale_recovery", "lsq", "--pred_depth_scale_factor", 1, "--post_process", "--save_pred_disps")
    for argv, _, word in REFUSED:
        with pytest.raises(SystemExit):
            _parse("--scale_recovery", "lsq", *argv)
        assert word in capsys.readouterr().err, argv
        _parse("--scale_recovery", "median", *argv)                      # the other modes take them as before
    with pytest.raises(SystemExit):
        MonodepthOptions().parse(["--eval_stereo", "--scale_recovery", "lsq"])
    assert "eval_stereo" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse("--scale_recovery", "affine")
    assert "invalid choice" in capsys.readouterr().err


def _bare(**fields):
    return types.SimpleNamespace(**dict(dict(eval_mono=True, eval_stereo=False, cuda=0, eval_split="eigen",
                                             splits_dir="nowhere", disable_median_scaling=False,
                                             pred_depth_scale_factor=1), **fields))


def test_evaluate_refuses_what_the_parser_refuses():
    for _, fields, word in REFUSED:
        assert options.alignment_conflict(_bare(**fields)) is None       # an opt without the field behaves as median
        assert word in options.alignment_conflict(_bare(scale_recovery="lsq", **fields))
        with pytest.raises(ValueError, match=word):                      # refused before anything is touched
            evaluation.evaluate(_bare(scale_recovery="lsq", **fields), dataloader=object(), models=(object(), object()))
    with pytest.raises(ValueError, match="eval_stereo"):
        evaluation.evaluate(_bare(scale_recovery="lsq", eval_mono=False, eval_stereo=True), dataloader=object(),
                            models=(object(), object()))
    assert options.alignment_conflict(_bare(scale_recovery="lsq")) is None
    assert options.alignment_conflict(types.SimpleNamespace()) is None
    # the names the ground options know, and the wording for one they do not
    assert evaluation._ground_options(_bare(scale_recovery="lsq")) is None
    assert evaluation._ground_options(_bare()) is None
    with pytest.raises(ValueError, match="scale_recovery is median or ground"):
        evaluation._ground_options(_bare(scale_recovery="affine"))


def test_scale_recovery_lsq_on_a_kitti_split(tmp_path, port, capsys):
    disps, gts, argv = A.write_split(tmp_path)
    n = len(gts)
    before = len(port.calls)
    mean_errors, alignment = evaluation.evaluate(_parse(*argv, "--scale_recovery", "lsq"), batch_size=4, backend=port,
                                                 device="cpu")
    out = capsys.readouterr().out
    assert port.calls[before:] == ["bbd_depth_metrics_affine"] * 2       # one launch per batch, nothing else
    truth = evaluation.GroundTruthSet(gts, "cpu")
    rows = evaluation.depth_metrics_affine(torch.from_numpy(disps), truth, list(range(n)), backend=port).numpy()
    assert np.array_equal(mean_errors, rows[:, :7].mean(0)) and mean_errors[0] < 1e-3
    assert alignment.shape == (n, 2) and alignment.dtype == np.float64 and np.array_equal(alignment, rows[:, 7:9])
    for (s0, o0), (scale, shift) in zip(A.SPLIT_GAUGES, alignment):
        assert abs(scale / s0 - 1.0) < 1e-2 and abs(shift - o0) < 1e-3
    want = "-> Loading predictions from {}\n".format(tmp_path / "disps.npy") \
        + " Alignment | scale med: {:0.4g} | shift med: {:0.4g}\n".format(np.median(rows[:, 7]), np.median(rows[:, 8])) \
        + "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3") + "\n" \
        + ("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\\n" \
        + "  " + ("{:>8} | " * 2).format("silog", "irmse") + "\n" \
        + ("&{: 8.3f}  " * 2).format(rows[:, 9].mean(), rows[:, 11].mean()) + "\\\\\n"
    assert out == want
    # the same file under median scaling: no shift is known there
    median_errors, ratios = evaluation.evaluate(_parse(*argv), batch_size=4, backend=port, device="cpu")
    assert median_errors[0] >= 10.0 * mean_errors[0] and len(ratios) == n


def test_scale_recovery_median_prints_what_it_printed_before(tmp_path, port, capsys):
    disps, gts, argv = A.write_split(tmp_path)
    n = len(gts)
    before = len(port.calls)
    errors, ratios = evaluation.evaluate(_parse(*argv, "--scale_recovery", "median"), batch_size=4, backend=port,
                                         device="cpu")
    printed = capsys.readouterr().out
    assert port.calls[before:] == ["bbd_depth_metrics"] * 2
    # the text of the evaluation as it stood before the option value, restated from the metrics rows
    rows = evaluation.depth_metrics(torch.from_numpy(disps), evaluation.GroundTruthSet(gts, "cpu"), list(range(n)),
                                    min_depth=1e-3, max_depth=80.0, pred_is_disp=True, median="numpy", backend=port)
    rows = rows.numpy().astype(np.float64)
    med = np.median(rows[:, 7])
    want = "-> Loading predictions from {}\n".format(tmp_path / "disps.npy") \
        + " Scaling ratios | med: {:0.3f} | std: {:0.3f}\n".format(med, np.std(rows[:, 7] / med)) \
        + "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3") + "\n" \
        + ("&{: 8.3f}  " * 7).format(*rows[:, :7].mean(0).tolist()) + "\\\\\n"
    assert printed == want
    assert np.array_equal(errors, rows[:, :7].mean(0)) and np.array_equal(ratios, rows[:, 7])


def test_lsq_names_what_it_cannot_align_and_what_it_flips(tmp_path, port, capsys):
    disps, gts, argv = A.write_split(tmp_path)
    disps = disps.copy()
    disps[1] = 0.5                                                       # constant: no line to fit
    disps[4] = -disps[4]                                                 # anti-correlated with the truth
    np.save(tmp_path / "disps.npy", disps)
    mean_errors, alignment = evaluation.evaluate(_parse(*argv, "--scale_recovery", "lsq", "--save_pred_disps"),
                                                 batch_size=4, backend=port, device="cpu")
    out = capsys.readouterr().out
    assert "WARNING: no alignment for 1 of 6 images" in out and "left out of the means: 1\n" in out
    assert "WARNING: scale <= 0 in 1 of 6 images" in out and "stay in the means: 4\n" in out
    assert np.isnan(alignment[1]).all() and np.isfinite(np.delete(alignment, 1, 0)).all() and alignment[4, 0] < 0
    rows = evaluation.depth_metrics_affine(torch.from_numpy(disps), evaluation.GroundTruthSet(gts, "cpu"),
                                           list(range(len(gts))), backend=port).numpy()
    assert np.array_equal(mean_errors, np.delete(rows, 1, 0)[:, :7].mean(0)) and mean_errors[0] < 1e-3
