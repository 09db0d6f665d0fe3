"""bench.py --dump-outputs, host side: file names, dtypes, the fixed sample of a large array and the size cap."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _result():
    g = torch.Generator().manual_seed(0)
    outputs = {("disp", 0): torch.rand(2, 1, 600, 300, generator=g),            # 360 000 elements: sampled
               ("bbd", "argmin"): torch.randint(0, 18, (2, 8, 16), generator=g),
               ("cam_T_cam", 0, -1): torch.rand(2, 4, 4, generator=g), "frames": [0, -1, 1]}
    losses = {"loss": torch.tensor(0.25), "loss/0": torch.tensor(0.5, dtype=torch.float64)}
    return outputs, losses


def test_dump_names_dtypes_and_fixed_sample(tmp_path):
    outputs, losses = _result()
    a = bench.dump_outputs(str(tmp_path / "a"), (outputs, losses))
    b = bench.dump_outputs(str(tmp_path / "b"), (outputs, losses))
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["loss.loss.npy", "loss.loss_0.npy", "out.bbd_argmin.npy", "out.cam_T_cam_0_-1.npy", "out.disp_0.npy"]
    assert a["files"] == 5 and a["sampled"] == ["out.disp_0"] and a["omitted"] == []
    load = lambda run, n: np.load(str(tmp_path / run / n))
    assert load("a", "loss.loss.npy").dtype == np.float32 and float(load("a", "loss.loss.npy")) == 0.25
    assert load("a", "loss.loss_0.npy").dtype == np.float64
    assert load("a", "out.bbd_argmin.npy").dtype == np.float64
    np.testing.assert_array_equal(load("a", "out.bbd_argmin.npy"), outputs[("bbd", "argmin")].numpy())
    np.testing.assert_array_equal(load("a", "out.cam_T_cam_0_-1.npy"), outputs[("cam_T_cam", 0, -1)].numpy())
    disp = load("a", "out.disp_0.npy")
    assert disp.shape == (bench.DUMP_SAMPLE,) and disp.dtype == np.float32
    np.testing.assert_array_equal(disp, load("b", "out.disp_0.npy"))               # the same indices every run
    assert np.isin(disp, outputs[("disp", 0)].numpy().reshape(-1)).all()
    assert a["bytes"] == b["bytes"] == sum(load("a", n).nbytes for n in names)


def test_dump_stays_within_its_byte_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * bench.DUMP_SAMPLE)
    outputs, losses = _result()
    got = bench.dump_outputs(str(tmp_path), (outputs, losses))
    assert got["bytes"] <= bench.DUMP_BYTES and "out.disp_0" in got["omitted"]
    assert sum(os.path.getsize(str(tmp_path / n)) - 128 for n in os.listdir(str(tmp_path))) == got["bytes"]
