"""CPU tier of the training log (`--train_log`): `trainlog.TrainLog`'s lines and files, `Trainer.log` on a golden case
through the host port of the panel kernels, and the wiring in `Trainer.run_epoch`."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panel_checks as pc  # noqa: E402
import panel_ref  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import Trainer, ops, synthetic  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402
from baseboostdepth_amd.trainlog import ARGMIN_KEYS, TrainLog, argmin_fractions, sec_to_hm_str  # noqa: E402

H, W, B = 64, 128, 2
# the reference's line (trainer.py:673-674), restated
REFERENCE_LINE = ("epoch {:>3} | batch {:>6} | examples/s: {:5.1f}" +
                  " | loss: {:.5f} | time elapsed: {} | time left: {}")


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def _hm(t):
    t = int(t)
    return "{:02d}h{:02d}m{:02d}s".format(t // 3600, t // 60 % 60, t % 60)


def test_log_time_line(capsys, tmp_path):
    tl = TrainLog(str(tmp_path), batch_size=12)
    line = tl.log_time(epoch=3, batch_idx=1250, step=12000, num_total_steps=66000, duration=0.25, loss=0.1234567,
                       start_time=1000.0, now=1000.0 + 10239.0)
    left = (66000 / 12000 - 1.0) * 10239.0
    want = REFERENCE_LINE.format(3, 1250, 12 / 0.25, 0.1234567, _hm(10239.0), _hm(left))
    assert line == want == capsys.readouterr().out.rstrip("\n")
    assert "02h50m39s" in line and sec_to_hm_str(10239) == "02h50m39s"
    assert tl.log_time(0, 0, 0, 10, 1.0, 1.0, 5.0, now=6.0).endswith("time left: 00h00m00s")


def test_context_lines(capsys, tmp_path):
    TrainLog(str(tmp_path), 2).context(4, 1e-4, [[0, 1, -1], [0, "s"]], [0, 1, 2, 3], [1, -1, "s"], 0.26, 1)
    out = capsys.readouterr().out.splitlines()
    assert out == ["Starting from epoch 4 and current learning rate is 0.0001", "Ordering: [[0, 1, -1], [0, 's']]",
                   "Scales: [0, 1, 2, 3]", "Valid Frames: [1, -1, 's']", "Current Boosting Weight: 0.26", "Omega: 1"]


def test_scalars_and_argmin_fractions(tmp_path):
    tl = TrainLog(str(tmp_path), 2)
    names = [[("T", 1), ("T", -1), ("E", 1), ("E", -1), ("I", 1), ("I", -1)], [("T", "s"), ("I", "s")]]
    counts = [[10, 20, 5, 5, 30, 30] + [0] * 14, [60, 40] + [0] * 18]
    frac = argmin_fractions(counts, names)
    assert frac == {"argmin/true_pose": 90 / 200, "argmin/error_induced": 10 / 200, "argmin/identity": 100 / 200}
    assert abs(sum(frac.values()) - 1.0) < 1e-12
    rec = {"step": 7, "epoch": 1, "batch": 6, "loss": torch.tensor(0.5), "loss/0": np.float32(0.25), "lr": 1e-4, **frac}
    tl.scalars("train", rec)
    tl.scalars("train", dict(rec, step=8))
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path), "train", "scalars.jsonl"))]
    assert [r["step"] for r in rows] == [7, 8]
    assert rows[0] == {"step": 7, "epoch": 1, "batch": 6, "loss": 0.5, "loss/0": 0.25, "lr": 1e-4, **frac}


def test_png_round_trip(tmp_path):
    from PIL import Image
    img = torch.randint(0, 256, (10, 14, 3), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    path = TrainLog(str(tmp_path), 2).panel("val", 123, img)
    assert path == os.path.join(str(tmp_path), "val", "panels", "step_00000123.png")
    assert np.array_equal(np.asarray(Image.open(path)), img.numpy())


def test_trainer_log_on_a_golden_case(port, tmp_path):
    from PIL import Image
    case, tr, inputs, outputs = pc.run_case("tri_7765_32x64", port, "cpu")
    losses = tr.compute_losses(inputs, outputs)
    tr.opt.train_log, tr.opt.log_samples = "panels", 1
    tr.log_path, tr.step, tr.epoch, tr.batch_idx = str(tmp_path), 41, 2, 40
    row = tr.log("train", inputs, outputs, losses)
    Hc, Wc = case.H, case.W
    names = tr.plan.cand_names[0]
    true = [f for k, f in names if k == "T"]
    assert len(true) == 6 and all(("E", f) in names for f in true)
    panel = np.asarray(Image.open(os.path.join(str(tmp_path), "train", "panels", "step_00000041.png")))
    assert panel.shape == ((1 + len(true)) * Hc, 4 * Wc, 3)
    cell = lambda r, c: panel_ref.cell(panel, r, c, Hc, Wc)
    plasma, magma, palette = pc.luts()
    # header row: target | plasma disparity | magma minimum-loss map | arg-min map
    assert np.array_equal(cell(0, 0), case.z["in/color/0/0"][0].transpose(1, 2, 0))
    assert np.array_equal(cell(0, 1), panel_ref.scalar_tile(outputs[("disp", 0)][0, 0].detach().numpy(), plasma)[0])
    assert np.array_equal(cell(0, 2), panel_ref.scalar_tile(outputs[("bbd", "to_optimise")][0][0].detach().numpy(), magma)[0])
    assert np.array_equal(cell(0, 3), panel_ref.argmin_tile(outputs[("bbd", "argmin")][0][0].numpy(), palette, 6, 6))
    # one row per true-pose candidate: source | warp | error-induced warp | empty
    for r, f in enumerate(true, start=1):
        j = tr.plan.jobs[f].index(0)
        assert np.array_equal(cell(r, 0), pc.quantised(inputs[("color", f, 0)])[tr.plan.source_row(f, 0)])
        assert np.array_equal(cell(r, 1), pc.quantised(outputs[("color", f, 0)])[j])
        assert np.array_equal(cell(r, 2), pc.quantised(outputs[("color_D", f, 0)])[j])
        assert not cell(r, 3).any()
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path), "train", "scalars.jsonl"))]
    assert rows == [row] and row["step"] == 41 and row["epoch"] == 2 and row["batch"] == 40
    assert row["loss"] == float(losses["loss"].detach()) and row["loss/0"] == float(losses["loss/0"].detach())
    assert abs(sum(row[k] for k in ARGMIN_KEYS) - 1.0) < 1e-12
    arg = outputs[("bbd", "argmin")][0]
    norm, guide = tr.argmin_masks(outputs)
    assert row["argmin/true_pose"] == float(norm.sum()) / arg.numel()
    assert row["argmin/error_induced"] == float(guide.sum()) / arg.numel()
    # two samples: the second block starts right under the first
    tr.opt.log_samples, tr.step = 2, 42
    tr.log("train", inputs, outputs, losses)
    two = np.asarray(Image.open(os.path.join(str(tmp_path), "train", "panels", "step_00000042.png")))
    n1 = sum(1 for k, _ in tr.plan.cand_names[1] if k == "T")
    assert two.shape[0] == (2 + len(true) + n1) * Hc and np.array_equal(two[:panel.shape[0]], panel)
    assert np.array_equal(panel_ref.cell(two, 1 + len(true), 0, Hc, Wc), case.z["in/color/0/0"][1].transpose(1, 2, 0))
    # off: nothing happens
    tr.opt.train_log = "off"
    assert tr.log("train", inputs, outputs, losses) is None and len(os.listdir(os.path.join(str(tmp_path), "train", "panels"))) == 2


def _opts(tmp, extra=""):
    return MonodepthOptions().parse(("--no_cuda --synthetic --weights_init scratch --height %d --width %d --batch_size %d "
                                     "--log_dir %s --model_name t --num_epochs 1 %s" % (H, W, B, tmp, extra)).split())


def _loader(opts, steps):
    return synthetic.synthetic_loader(B, steps, H, W, opts.scales, device="cpu", seed=5, epoch=0)


def _files_under(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs)


def test_run_epoch_text_log_prints_and_records(port, tmp_path, capsys):
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts(str(tmp_path), "--train_log text --log_frequency 2")
    assert opts.train_log == "text" and opts.log_samples == 1
    tr = Trainer(opts, backend=port)
    tr.num_total_steps = 5
    tr.run_epoch(_loader(opts, 5))
    out = capsys.readouterr().out.splitlines()
    lines = [l for l in out if l.startswith("epoch")]
    assert len(lines) == 2 and "| batch      2 |" in lines[0] and "| batch      4 |" in lines[1]
    assert sum(l.startswith("Ordering: ") for l in out) == 2 and sum(l.startswith("Omega: ") for l in out) == 2
    assert sum(l.startswith("Starting from epoch 0 and current learning rate is ") for l in out) == 2
    rows = [json.loads(l) for l in open(os.path.join(tr.log_path, "train", "scalars.jsonl"))]
    assert [r["batch"] for r in rows] == [2, 4] and [r["step"] for r in rows] == [3, 5]
    for r in rows:
        assert set(r) == {"step", "epoch", "batch", "lr", "loss", "loss/0", "loss/1", "loss/2", "loss/3", *ARGMIN_KEYS}
        assert abs(sum(r[k] for k in ARGMIN_KEYS) - 1.0) < 1e-12 and np.isfinite(r["loss"])
        assert ("loss: %.5f" % r["loss"]) in lines[rows.index(r)]
    assert _files_under(tr.log_path) == ["train/scalars.jsonl"]          # text: no picture, no validation files


def test_run_epoch_without_the_flag_is_silent(port, tmp_path, capsys):
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts(str(tmp_path), "--log_frequency 2")
    assert opts.train_log == "off"
    tr = Trainer(opts, backend=port)
    outputs, losses = tr.run_epoch(_loader(opts, 3))
    assert capsys.readouterr().out == ""
    assert not os.path.exists(tr.log_path)
    assert not any(k[0] == "bbd" and k[1] not in ("loss_sum", "to_optimise", "argmin", "identity") for k in outputs
                   if isinstance(k, tuple))
    assert not hasattr(tr, "trainlog") and not hasattr(tr, "start_time")


def test_weights_best_follows_the_validation_result(port, tmp_path, capsys):
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts(str(tmp_path), "--train_log text --log_frequency 1")
    tr = Trainer(opts, backend=port)
    metric = lambda a: dict({n: 0.5 for n in tr.depth_metric_names}, **{"de/abs_rel": a})
    results = [metric(0.30), metric(0.35), metric(0.20)]
    saved = []
    tr.kitti_val_loader = lambda: object()
    tr.val = lambda loader: results.pop(0)
    tr.save_model = lambda name=None: saved.append(name)
    tr.run_epoch(_loader(opts, 4))                      # validations after batches 1, 2, 3
    assert saved == ["best", "best"] and tr.best_logged == 0.20
    rows = [json.loads(l) for l in open(os.path.join(tr.log_path, "val", "scalars.jsonl"))]
    assert [r["de/abs_rel"] for r in rows] == [0.30, 0.35, 0.20]
    assert all(set(tr.depth_metric_names) <= set(r) for r in rows)
    # a real save lands where resume_epoch looks for it
    del tr.save_model
    tr._log_val(metric(0.10))
    assert os.path.isfile(os.path.join(tr.log_path, "models", "weights_best", "encoder.pth"))
    tr._log_val(metric(0.15))
    assert tr.best_logged == 0.10


def test_panels_without_the_library_or_a_backend_is_refused(tmp_path):
    opts = _opts(str(tmp_path), "--train_log panels")
    with pytest.raises(ValueError, match="--train_log"):
        Trainer(opts)
