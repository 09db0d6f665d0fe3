"""CPU tier of the prediction command line (test_simple.py / baseboostdepth_amd.inference.run_cli) with a stub
predictor injected: argument parsing, file and folder discovery, the skip rules, output names and directories, the
size of the written JPEGs and --save_npy."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from baseboostdepth_amd import inference  # noqa: E402


class StubPredictor:
    """Colours every image with a ramp of its own size and remembers what it was asked."""

    def __init__(self):
        self.calls = []

    def predict(self, images, want_float=False):
        self.calls.append(([im.shape for im in images], want_float))
        out = []
        for im in images:
            assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3
            H, W = im.shape[:2]
            col = np.zeros((H, W, 3), np.uint8)
            col[..., 0] = np.linspace(0, 255, W).astype(np.uint8)[None, :]
            col[..., 1] = im[..., 1]
            sd = (np.arange(H * W, dtype=np.float32).reshape(H, W) + 1) if want_float else None
            out.append(inference.DepthPrediction(col, 1.0, 2.0, sd))
        return out


def _write(path, h, w, mode="RGB", seed=0):
    rng = np.random.default_rng(seed)
    arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im = Image.fromarray(arr)
    if mode != "RGB":
        im = im.convert(mode)
    im.save(path)


def test_arguments_are_the_references_plus_save_npy():
    a = inference.parse_args(["--image_path", "x", "--save_path", "y", "--weights", "w"])
    assert (a.image_path, a.save_path, a.weights, a.ext, a.vit, a.save_npy) == ("x", "y", "w", "jpg", False, False)
    a = inference.parse_args(["--image_path", "x", "--save_path", "y", "--weights", "w", "--ext", "png", "--vit",
                              "--save_npy"])
    assert a.ext == "png" and a.vit and a.save_npy
    for missing in ("--image_path", "--save_path", "--weights"):
        argv = ["--image_path", "x", "--save_path", "y", "--weights", "w"]
        i = argv.index(missing)
        with pytest.raises(SystemExit):
            inference.parse_args(argv[:i] + argv[i + 2:])


def test_help_documents_the_two_additions(capsys):
    with pytest.raises(SystemExit):
        inference.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--save_npy" in text and "_disp.npy" in text and "_Base.jpg" in text and "skipped" in text


def test_folder_run_writes_named_jpegs_of_original_size(tmp_path):
    src, dst = tmp_path / "in", tmp_path / "out" / "deeper"
    src.mkdir()
    _write(src / "a.png", 37, 91, seed=1)
    _write(src / "b.png", 50, 64, "L", seed=2)              # greyscale input: opened with convert('RGB')
    _write(src / "c.jpg", 20, 30)                          # other extension: not found by --ext png
    stub = StubPredictor()
    args = inference.parse_args(["--image_path", str(src), "--save_path", str(dst), "--ext", "png", "--weights", "w"])
    written = inference.run_cli(args, predictor=stub)
    assert sorted(os.listdir(dst)) == ["a_Base.jpg", "b_Base.jpg"]
    assert sorted(os.path.basename(p) for p in written) == ["a_Base.jpg", "b_Base.jpg"]
    assert Image.open(dst / "a_Base.jpg").size == (91, 37) and Image.open(dst / "b_Base.jpg").size == (64, 50)
    assert stub.calls == [([(37, 91, 3), (50, 64, 3)], False)]          # the whole folder is ONE predict call
    assert sorted(os.listdir(src)) == ["a.png", "b.png", "c.jpg"]       # nothing written next to the inputs


def test_single_file_writes_next_to_the_file(tmp_path):
    _write(tmp_path / "photo.png", 33, 47)
    unused = tmp_path / "unused"
    args = inference.parse_args(["--image_path", str(tmp_path / "photo.png"), "--save_path", str(unused),
                                 "--weights", "w"])
    inference.run_cli(args, predictor=StubPredictor())
    assert Image.open(tmp_path / "photo_Base.jpg").size == (47, 33)
    assert not unused.exists()


def test_outputs_of_an_earlier_run_are_skipped(tmp_path):
    for name in ("x.jpg", "x_Base.jpg", "y_disp.jpg"):
        _write(tmp_path / name, 16, 24)
    stub = StubPredictor()
    args = inference.parse_args(["--image_path", str(tmp_path), "--save_path", str(tmp_path), "--weights", "w"])
    inference.run_cli(args, predictor=stub)
    assert stub.calls == [([(16, 24, 3)], False)]
    before = sorted(os.listdir(tmp_path))
    inference.run_cli(args, predictor=stub)                          # second run over its own outputs
    assert sorted(os.listdir(tmp_path)) == before == ["x.jpg", "x_Base.jpg", "y_disp.jpg"]
    assert stub.calls[1] == ([(16, 24, 3)], False)


def test_save_npy_writes_the_scaled_disparity(tmp_path):
    _write(tmp_path / "k.png", 12, 18)
    stub = StubPredictor()
    args = inference.parse_args(["--image_path", str(tmp_path), "--save_path", str(tmp_path / "o"), "--ext", "png",
                                 "--weights", "w", "--save_npy"])
    inference.run_cli(args, predictor=stub)
    sd = np.load(tmp_path / "o" / "k_disp.npy")
    assert sd.dtype == np.float32 and sd.shape == (12, 18) and sd[0, 0] == 1 and sd[-1, -1] == 12 * 18
    assert stub.calls == [([(12, 18, 3)], True)]


def test_batches_follow_batch_size_and_keep_order(tmp_path):
    for k in range(5):
        _write(tmp_path / ("im%d.png" % k), 10 + k, 20 + k, seed=k)
    stub = StubPredictor()
    args = inference.parse_args(["--image_path", str(tmp_path), "--save_path", str(tmp_path / "o"), "--ext", "png",
                                 "--weights", "w", "--batch_size", "2"])
    inference.run_cli(args, predictor=stub)
    assert [len(c[0]) for c in stub.calls] == [2, 2, 1]
    for k in range(5):
        assert Image.open(tmp_path / "o" / ("im%d_Base.jpg" % k)).size == (20 + k, 10 + k)


def test_missing_path_raises_and_pool_is_small(tmp_path):
    args = inference.parse_args(["--image_path", str(tmp_path / "nope"), "--save_path", "y", "--weights", "w"])
    with pytest.raises(Exception, match="Can not find"):
        inference.run_cli(args, predictor=StubPredictor())
    assert inference.HOST_THREADS <= 8


def test_root_script_is_the_same_command_line():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_simple.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--image_path" in r.stdout and "--save_npy" in r.stdout
