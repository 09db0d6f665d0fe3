"""`export_depth_hints.py` end to end on the CPU tier (host port): the synthetic KITTI-shaped tree of the loader tests
(`synthetic.synthetic_kitti_tree`: the right camera's frame is the left one's shifted by 9 pixels at full size), the
hint file, `--as_disps`, and `evaluate_depth.py --eval_stereo --ext_disp_to_eval` on what was written.  There are no
real KITTI data here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import evaluation, hints, synthetic  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

FULL_H, FULL_W, SHIFT = 120, 400, 9          # the tree's image size and its stereo shift in pixels of that size
H, W = 48, 160                               # the export size: the shift is 9 * 160 / 400 = 3.6 pixels there


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    root = tmp_path_factory.mktemp("hints")
    folder = "2011_09_26/2011_09_26_drive_0001_sync"
    synthetic.synthetic_kitti_tree(str(root / "kitti"), drives=((folder, FULL_H, FULL_W),), frames=4)
    split = root / "splits" / "eigen"
    split.mkdir(parents=True)
    lines = ["%s %d %s" % (folder, t, side) for t, side in ((0, "l"), (1, "r"), (2, "l"), (3, "l"), (3, "r"))]
    (split / "test_files.txt").write_text("\n".join(lines) + "\n")
    argv = ["--data_path", str(root / "kitti"), "--split", "eigen", "--splits_dir", str(root / "splits"), "--height", str(H),
            "--width", str(W), "--hint_disparities", "64", "--as_disps", str(root / "sgm_disps.npy"), "--batch_size", "2",
            "--device", "cpu"]
    path, density = hints.export_main(argv, backend=PortBackend())
    return root, path, density, len(lines)


def test_the_hint_file_holds_the_tree_s_shift(exported, capsys):
    root, path, density, n = exported
    assert path == str(root / "splits" / "eigen" / "depth_hints.npy")
    disp16 = np.load(path)
    assert disp16.dtype == np.int16 and disp16.shape == (n, H, W)
    valid = disp16 != -16
    assert abs(density - valid.mean()) < 1e-12 and density > 0.5
    # the plane's disparity at the export size, to the matcher's half pixel and the resize's blur
    assert abs(np.median(disp16[valid]) / 16.0 - SHIFT * W / FULL_W) <= 0.5
    # line 1 and line 4 name the right camera: matched mirrored, the same scene, the same disparity
    assert abs(np.median(disp16[1][valid[1]]) / 16.0 - SHIFT * W / FULL_W) <= 0.5


def test_as_disps_scores_under_eval_stereo(exported, capsys):
    root, path, density, n = exported
    disps = np.load(root / "sgm_disps.npy")
    assert disps.dtype == np.float32 and disps.shape == (n, H, W) and (disps > 0).all()
    # metres = 5.4 / q: fx * 0.54 / d with fx = 0.58 w, for the median pixel
    metres = 5.4 / np.median(disps)
    want = 0.58 * FULL_W * 0.54 / SHIFT
    assert abs(metres - want) <= 0.15 * want
    gts = np.empty(n, dtype=object)
    for i in range(n):
        gts[i] = np.full((FULL_H, FULL_W), want, np.float32)
    np.savez_compressed(root / "splits" / "eigen" / "gt_depths.npz", data=gts)
    opt = MonodepthOptions().parse(["--eval_stereo", "--eval_split", "eigen", "--splits_dir", str(root / "splits"),
                                    "--ext_disp_to_eval", str(root / "sgm_disps.npy"), "--no_cuda"])
    mean_errors, ratios = evaluation.evaluate(opt, batch_size=2, backend=PortBackend(), device="cpu")
    capsys.readouterr()
    assert mean_errors.shape == (7,) and np.isfinite(mean_errors).all()
    assert mean_errors[0] < 0.2 and mean_errors[4] > 0.8            # abs_rel and a1 against the plane's true depth


def test_hints_as_disps_is_the_written_conversion():
    filled = np.array([[[-16, 0, 16, 58]]], np.int16)
    q = hints.hints_as_disps(filled, 100)
    assert q.dtype == np.float32
    np.testing.assert_allclose(q[0, 0], [1 / 16 / 5.8, 1 / 16 / 5.8, 1 / 5.8, 58 / 16 / 5.8], rtol=1e-6)
