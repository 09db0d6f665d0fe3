"""CPU tier of the comparison command line (validation.py / baseboostdepth_amd.compare.run_cli): option parsing, the
refusals, frame tokens, the sheet-layout arithmetic, abs_rel.csv, labelling, and the whole pipeline on a synthetic
KITTI-shaped tree with predictors injected (tiny networks on the host port)."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compare_checks as C  # noqa: E402
from baseboostdepth_amd import compare, inference  # noqa: E402

BASE = ["--model_name", "a", "b", "--kt_path", "k"]


def test_arguments_and_defaults():
    a = compare.parse_args(BASE)
    assert a.model_name == ["a", "b"] and a.ext == "jpg" and a.format == "jpg" and not a.ViT and a.num_layers == 18
    assert a.split_dir == os.path.join("splits", "eigen_zhou") and a.files == "val_files.txt"
    assert a.output == "validation_vis" and a.cell_size == [621, 188] and not a.error_maps and a.err_max == 0.5
    assert a.dot_radius == 2 and not a.no_labels and a.batch_size == 16 and a.limit is None
    a = compare.parse_args(BASE + ["--ViT", "--format", "png", "--cell_size", "64", "24", "--error_maps", "--limit", "3",
                                   "--ext", "png", "--dot_radius", "0", "--no_labels"])
    assert a.ViT and a.format == "png" and a.cell_size == [64, 24] and a.error_maps and a.limit == 3 and a.dot_radius == 0


@pytest.mark.parametrize("flag", ["--SQL", "--pred_metric_depth"])
def test_other_zoos_are_refused_in_the_options_wording(flag, capsys):
    with pytest.raises(SystemExit):
        compare.parse_args(BASE + [flag])
    assert "%s select parts of the reference that are outside this build's scope" % flag in capsys.readouterr().err


def test_bad_values_are_refused():
    for extra in (["--dot_radius", "5"], ["--format", "bmp"], ["--cell_size", "0", "10"]):
        with pytest.raises(SystemExit):
            compare.parse_args(BASE + extra)
    with pytest.raises(SystemExit):
        compare.parse_args(["--kt_path", "k"])


def test_frame_tokens_are_padded_to_ten_digits(tmp_path):
    assert compare.frame_token("5") == "0000000005" and compare.frame_token("0000000123") == "0000000123"
    assert compare.frame_token("12345678901") == "12345678901" and compare.frame_token("img_7") == "img_7"
    (tmp_path / "val_files.txt").write_text("d/x 7 l\n\nd/y 0000000012 r\nd/z name l\n")
    frames = compare.read_frames(str(tmp_path), "val_files.txt", "/kt", "jpg")
    assert frames[0] == ("d/x", "0000000007", os.path.join("/kt", "d/x", "image_02", "data", "0000000007.jpg"))
    assert frames[1][2].endswith(os.path.join("d/y", "image_02", "data", "0000000012.jpg"))       # always image_02
    assert frames[2][1] == "name" and len(compare.read_frames(str(tmp_path), "val_files.txt", "/kt", limit=2)) == 2


def test_sheet_layout_arithmetic():
    for M in range(1, 8):
        assert compare.sheet_rows(M) == 1 + (M + 1) // 2 and compare.sheet_rows(M, True) == 1 + M
        cells = compare.sheet_cells(M)
        assert cells[(0, 0)] == ("image", None) and cells[(0, 1)] == ("gt", None)
        assert [cells[(1 + m // 2, m % 2)] for m in range(M)] == [("disp", m) for m in range(M)]
        assert len(cells) == 2 + M and ((compare.sheet_rows(M) - 1, 1) in cells) == (M % 2 == 0)
        cells = compare.sheet_cells(M, True)
        assert all(cells[(1 + m, 0)] == ("disp", m) and cells[(1 + m, 1)] == ("error", m) for m in range(M))
    assert compare.cell_rect(0, 0) == (0, 188, 0, 621) and compare.cell_rect(2, 1) == (376, 564, 621, 1242)
    assert compare.cell_rect(1, 1, (24, 64)) == (24, 48, 64, 128)


def test_labels_touch_only_their_boxes():
    rng = np.random.default_rng(0)
    cell = (40, 120)
    sheet = rng.integers(0, 200, (3 * 40, 2 * 120, 3), dtype=np.uint8)
    labels = compare.sheet_labels(["md2_row1", "rand", "x"], [0.1234, 0.0871, 0.5])
    assert labels == {(0, 0): "Images", (0, 1): "Depth", (1, 0): "MD2_ROW1 0.123", (1, 1): "RAND 0.087", (2, 0): "X 0.500"}
    out = compare.label_sheet(sheet, labels, cell)
    assert out is not sheet and out.shape == sheet.shape
    mask = np.zeros(sheet.shape[:2], bool)
    for (y0, y1, x0, x1) in compare.label_boxes(labels, cell).values():
        mask[y0:y1, x0:x1] = True
    assert np.array_equal(out[~mask], sheet[~mask])
    changed = (out != sheet).any(-1)
    assert changed.any() and (out[changed] == 255).all()
    for (row, col) in labels:                                   # every label drew something inside its own cell
        y0, y1, x0, x1 = compare.cell_rect(row, col, cell)
        assert changed[y0:y1, x0:x1].any()
    assert not changed[80:120, 120:240].any()                   # the unused cell has no label
    assert compare.sheet_labels(["a"], [0.25], error_maps=True) == {(0, 0): "Images", (0, 1): "Depth", (1, 0): "A 0.250"}


def test_csv_format(tmp_path):
    frames = [("d/x", "0000000007", "p"), ("d/y", "0000000012", "q")]
    compare.write_csv(str(tmp_path / "abs_rel.csv"), ["a", "b"], frames, [[0.1, 0.25], [0.3, 0.35]])
    text = (tmp_path / "abs_rel.csv").read_text().splitlines()
    assert text == ["index,frame,a,b", "0000000000,d/x/0000000007,0.100000,0.250000",
                    "0000000001,d/y/0000000012,0.300000,0.350000", "mean,,0.200000,0.300000"]


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


def _predictors(port):
    return C.tiny_predictors(port, [(32, 64), (24, 48), (32, 64)])


@pytest.mark.parametrize("error_maps", [False, True])
def test_pipeline_on_a_synthetic_tree(tmp_path, port, error_maps, capsys):
    images, maps = C.synth_frames()
    kt, split = C.write_tree(str(tmp_path), images, maps)
    out = str(tmp_path / "out")
    argv = ["--model_name", "m0", "m1", "m2", "--kt_path", kt, "--split_dir", split, "--output", out, "--ext", "png",
            "--format", "png", "--cell_size", "64", "24", "--batch_size", "2"] + (["--error_maps"] if error_maps else [])
    args = compare.parse_args(argv)
    predictors = _predictors(port)
    abs_rel, ratios = compare.run_cli(args, predictors=predictors)
    assert abs_rel.shape == (3, 3) and (abs_rel > 0).all() and (ratios > 0).all()
    names = ["%010d.png" % i for i in range(3)]
    want = {"depth", "sheets", "m0", "m1", "m2", "abs_rel.csv"} | ({"errors"} if error_maps else set())
    assert set(os.listdir(out)) == want
    for d in ("depth", "sheets", "m0", "m1", "m2") + (("errors/m0", "errors/m2") if error_maps else ()):
        assert sorted(os.listdir(os.path.join(out, d))) == names
    R = compare.sheet_rows(3, error_maps)
    assert Image.open(os.path.join(out, "sheets", names[0])).size == (128, R * 24)
    # what was written is what compare_batch returns (the batches of the run: frames 0-1, then frame 2)
    from baseboostdepth_amd import evaluation
    gts = evaluation.GroundTruthSet(maps, "cpu")
    for chunk in ([0, 1], [2]):
        res = compare.compare_batch([images[i] for i in chunk], gts, chunk, predictors, cell=(24, 64),
                                    error_maps=error_maps).host()
        for j, i in enumerate(chunk):
            assert Image.open(os.path.join(out, "m1", names[i])).size == C.FRAME_SIZES[i][::-1]
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, "m1", names[i]))), res.disps[1][j])
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, "depth", names[i]))), res.gt[j])
            if error_maps:
                assert np.array_equal(np.asarray(Image.open(os.path.join(out, "errors", "m2", names[i]))), res.errors[2][j])
            labels = compare.sheet_labels(["m0", "m1", "m2"], res.rows[:, j, 0], error_maps)
            sheet = np.asarray(Image.open(os.path.join(out, "sheets", names[i])))
            assert np.array_equal(sheet, compare.label_sheet(res.sheets[j], labels, (24, 64)))
            assert np.allclose(abs_rel[i], res.rows[:, j, 0], rtol=0, atol=0)
    header, body, mean = C.read_csv(os.path.join(out, "abs_rel.csv"))
    assert header == ["index", "frame", "m0", "m1", "m2"] and [r[0] for r in body] == [n[:10] for n in names]
    assert body[1][1] == "2011_09_26/2011_09_26_drive_0001_sync/0000000001"
    assert [r[2:] for r in body] == [["%.6f" % v for v in row] for row in abs_rel]
    assert mean[:2] == ["mean", ""] and mean[2:] == ["%.6f" % v for v in abs_rel.mean(0)]
    printed = capsys.readouterr().out
    for m in range(3):
        assert "abs_rel %0.4f | scaling ratio %0.4f" % (abs_rel[:, m].mean(), ratios[:, m].mean()) in printed


def test_count_mismatch_names_both_numbers(tmp_path, port):
    images, maps = C.synth_frames()
    kt, split = C.write_tree(str(tmp_path), images, maps[:2])
    args = compare.parse_args(["--model_name", "m0", "--kt_path", kt, "--split_dir", split, "--ext", "png",
                               "--output", str(tmp_path / "o")])
    with pytest.raises(ValueError, match="3 frames.*2 maps"):
        compare.run_cli(args, predictors=_predictors(port)[:1])


def test_no_labels_leaves_the_device_sheet(tmp_path, port):
    images, maps = C.synth_frames()
    kt, split = C.write_tree(str(tmp_path), images, maps)
    out = str(tmp_path / "o")
    args = compare.parse_args(["--model_name", "m0", "--kt_path", kt, "--split_dir", split, "--ext", "png", "--format",
                               "png", "--output", out, "--cell_size", "64", "24", "--no_labels", "--limit", "1"])
    predictors = _predictors(port)[:1]
    compare.run_cli(args, predictors=predictors)
    from baseboostdepth_amd import evaluation
    res = compare.compare_batch(images[:1], evaluation.GroundTruthSet(maps, "cpu"), [0], predictors, cell=(24, 64)).host()
    assert sorted(os.listdir(os.path.join(out, "sheets"))) == ["0000000000.png"]
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "sheets", "0000000000.png"))), res.sheets[0])
    assert inference.HOST_THREADS <= 8


def test_root_script_is_the_same_command_line():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "validation.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--model_name" in r.stdout and "--error_maps" in r.stdout
