"""CPU tier of the KITTI odometry evaluation: the host port of bbd_odom.hip (same bbd_odom_math.h) through the `backend=`
seam of `evaluation.pose_ate` against the reference's results (tools/make_golden_odom.py; acceptance rules:
tests/odom_checks.py), `datasets.KITTIOdomDataset` and its window tables on a small tree of JPEGs, the new options, and
the checks `evaluation.evaluate_pose` makes before it launches anything."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import odom_checks as oc  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, datasets, evaluation  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.fixture(scope="module")
def v():
    return oc.load()


def test_fixture_holds_what_the_tests_rely_on(v):
    for case in oc.CASES:
        M, N, S, Ls = oc.SHAPES[case]
        assert v[case + "/poses"].shape == (1 + S, N, 16) and v[case + "/poses"].dtype == np.float32
        assert int(v[case + "/S"]) == S and tuple(v[case + "/Ls"]) == Ls and len(str(v[case + "/text"]).splitlines()) == M
        assert v[case + "/gt_local"].shape == (M - S, 16) and v[case + "/chained"].shape == (N, 16)
    assert np.array_equal(v["skip1/chained"].view(np.uint32), v["skip1/poses"][0].view(np.uint32))
    assert v["no_track/L1/ates"].shape == (2, 0) and np.isnan(v["no_track/L1/summary"][:, :2]).all()
    nan = np.isnan(v["zero_pred/L1/ates"])
    assert nan.sum(1).tolist() == [2, 2] and np.isnan(v["zero_pred/L1/summary"][:, :2]).all()
    assert v["zero_pred/L1/summary"][:, 2].tolist() == [6.0, 6.0]
    rot = np.loadtxt(str(v["curve/text"]).splitlines()).reshape(-1, 3, 4)[:, :, :3]
    assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() > 1e-8         # printed to 7 digits: not orthonormal
    assert np.abs(np.loadtxt(str(v["curve/text"]).splitlines())).max() > 400


@pytest.mark.parametrize("case,L", oc.EVERY)
def test_host_port_matches_the_reference(port, v, tmp_path, case, L):
    res, gt = oc.run(v, case, L, port, "cpu", tmp_path)
    oc.check(v, case, L, res, gt)
    again, _ = oc.run(v, case, L, port, "cpu", tmp_path)
    a, b = oc.host(res), oc.host(again)
    assert all(oc.same_bytes(a[k], b[k]) for k in oc.FIELDS)


@pytest.mark.parametrize("case", ["no_track", "one_track", "big"])
def test_outputs_are_written_whole_and_nothing_else(port, v, tmp_path, case):
    M, N, S, _ = oc.SHAPES[case]
    gt = torch.from_numpy(oc.gt_global(v, case, tmp_path))
    poses = torch.from_numpy(v[case + "/poses"])
    sizes = {"chained": (N * 16, torch.float32), "gt_local": ((M - S) * 16, torch.float64),
             "ates": (2 * max(N - S, 0), torch.float64), "summary": (8, torch.float64)}
    bufs = {k: torch.full((n + 14,), float("nan"), dtype=dt) for k, (n, dt) in sizes.items()}
    views = {k: bufs[k][7:7 + n] for k, (n, _) in sizes.items()}
    evaluation.pose_ate_into(poses, gt, views["chained"], views["gt_local"], views["ates"], views["summary"], S, 1, port)
    for k, (n, _) in sizes.items():
        assert torch.isnan(bufs[k][:7]).all() and torch.isnan(bufs[k][7 + n:]).all(), k
    want, _ = oc.run(v, case, 1, port, "cpu", tmp_path)
    for k in ("chained", "gt_local", "ates", "summary"):
        assert oc.same_bytes(views[k].numpy(), getattr(want, k).numpy().reshape(-1)), k
    if case != "no_track":
        assert not any(torch.isnan(views[k]).any() for k in views)


def test_refusals(port, v, tmp_path):
    gt = oc.gt_global(v, "one_track", tmp_path)
    poses = torch.from_numpy(v["one_track/poses"])
    for kw in (dict(skip=0), dict(track_length=0), dict(skip=3)):                 # skip=3: poses has 1 + 2 sections
        with pytest.raises(ValueError):
            evaluation.pose_ate(poses, gt, backend=port, **kw)
    with pytest.raises(ValueError, match=r"N = 3 > M - S = 2"):
        evaluation.pose_ate(poses, gt[:4], backend=port)
    with pytest.raises(ValueError):
        evaluation.pose_ate(poses.double(), gt, backend=port)
    # the C entry point itself refuses what the binding would have caught
    out = [torch.empty(64, dtype=dt) for dt in (torch.float32, torch.float64, torch.float64, torch.float64)]
    g = torch.from_numpy(gt)
    for N, M, S, L in ((3, 6, 0, 1), (3, 6, 2, 0), (-1, 6, 2, 1), (3, 4, 2, 1), (0, 1, 2, 1)):
        rc = port.dll.hp_pose_ate(_lib.ptr(poses), _lib.ptr(g), *[_lib.ptr(t) for t in out], N, M, S, L)
        assert rc != 0, (N, M, S, L)


def test_hip_backend_refuses_cpu_tensors(v, tmp_path):
    from baseboostdepth_amd import ops
    from baseboostdepth_amd.csrc.build import build
    build()
    with pytest.raises(_lib.BbdError):
        oc.run(v, "one_track", 1, ops.HipBackend(), "cpu", tmp_path)


# ---------------------------------------------------------------------------- dataset
def _tree(tmp_path, frames=12, missing=(), seq=9):
    root = str(tmp_path / "data" / "odom")
    oc.write_sequence(root, seq, range(frames), missing=missing)
    return str(tmp_path / "data" / "kitti"), root


def _dataset(lines, kt_path, **kw):
    return datasets.KITTIOdomDataset(lines, 0, 32, 64, kt_path=kt_path, is_train=False, kt=True, naive_mix=True, **kw)


def test_dataset_paths_and_line_parsing(tmp_path):
    kt, root = _tree(tmp_path)
    ds = _dataset(["9 0 l", "9 7 r", "10"], kt)
    assert ds.odom_path == root and len(ds) == 3                              # dirname(kt_path)/odom, as the reference
    assert ds.index_to_folder_and_frame_idx(1) == ("9", 7, "r") and ds.index_to_folder_and_frame_idx(2) == ("10", 0, None)
    assert ds.get_image_path_odom(kt, "9", 7, "r") == os.path.join(root, "sequences/09", "image_3", "data", "000007.jpg")
    assert ds.get_image_path_odom(kt, "9", 123456, "l").endswith("sequences/09/image_2/data/123456.jpg")
    other = _dataset(["9 0 l"], kt, odom_path=str(tmp_path / "elsewhere"))
    assert other.get_image_path_odom(None, "0", 1, "l") == str(tmp_path / "elsewhere" / "sequences/00/image_2/data/000001.jpg")
    with pytest.raises(ValueError):
        datasets.KITTIOdomDataset(["9 0 l"], 0, 32, 64, kt_path=kt, is_train=True, kt=True, naive_mix=True)
    item = ds[0]                                                              # one item = one frame, the loader's form
    assert list(item["images"]) == [0] and item["images"][0].shape == (48, 160, 3) and item["images"][0].dtype == np.uint8
    assert item["paths"][0] == ds.get_image_path_odom(kt, "9", 0, "l") and item["flip"] is False and not item["jitter"]
    batch = datasets.DeviceCollate(32, 64, [0], "cpu", backend=_image_port())([ds[0], _dataset(["9 3 l"], kt)[0]])
    assert batch[("color", 0, 0)].shape == (2, 3, 32, 64)


def _image_port():
    from ports import PortBackend
    return PortBackend()


def test_windows_tables_and_trailing_drop(tmp_path):
    kt, _ = _tree(tmp_path, frames=12)
    lines = ["9 %d l" % t for t in range(11)]                    # one line fewer than frames, like test_files_09.txt
    ds = _dataset(lines, kt)
    frames, pairs, N = ds.windows(2)
    assert N == 10 and frames == ["9 %d l" % t for t in range(12)]            # line 10 needs frame 12: dropped
    assert pairs.dtype == np.int32 and pairs.shape == (3, 10, 2) and pairs.flags["C_CONTIGUOUS"]
    i = np.arange(10)
    assert np.array_equal(pairs[0], np.stack([i, i + 2], 1)) and np.array_equal(pairs[1], np.stack([i, i + 1], 1))
    assert np.array_equal(pairs[2], np.stack([i + 1, i + 2], 1))
    frames, pairs, N = ds.windows(1)
    assert N == 11 and pairs.shape == (2, 11, 2) and np.array_equal(pairs[0], pairs[1]) and len(frames) == 12
    frames, pairs, N = ds.windows(3)
    assert N == 9 and pairs.shape == (4, 9, 2) and np.array_equal(pairs[0, :, 1], np.arange(9) + 3)
    sub = _dataset(["9 %d l" % t for t in range(4, 8)], kt)                 # a pool that does not start at frame 0
    frames, pairs, N = sub.windows(2)
    assert N == 4 and frames == ["9 %d l" % t for t in range(4, 10)] and pairs[0, 0].tolist() == [0, 2]
    with pytest.raises(ValueError):
        ds.windows(0)
    with pytest.raises(ValueError):
        _dataset(["9"], kt).windows(2)


def test_a_frame_missing_in_the_middle_is_an_error(tmp_path):
    kt, root = _tree(tmp_path, frames=12, missing=(5,))
    ds = _dataset(["9 %d l" % t for t in range(11)], kt)
    with pytest.raises(FileNotFoundError, match="000005.jpg"):
        ds.windows(2)


# ---------------------------------------------------------------------------- options and the evaluator's host side
def test_options_parse_the_new_flags_and_select_the_split(tmp_path):
    o = MonodepthOptions().parse([])
    assert (o.skip_frame, o.track_length, o.odom_path) == (2, 1, None)
    o = MonodepthOptions().parse(["--eval_split", "odom_9", "--skip_frame", "3", "--track_length", "5", "--odom_path", "/x/odo",
                                  "--kt_path", "/data/kitti", "--splits_dir", "/s"])
    assert (o.skip_frame, o.track_length, o.odom_path) == (3, 5, "/x/odo")
    assert evaluation.odom_paths(o) == (9, "/s/odom/test_files_09.txt", "/x/odo", "/x/odo/poses/09.txt")
    for split, nn in (("odom_9", "09"), ("odom_10", "10"), ("odom_0", "00")):
        o = MonodepthOptions().parse(["--eval_split", split, "--kt_path", "/data/kitti", "--splits_dir", "/s"])
        seq, split_file, root, poses = evaluation.odom_paths(o)
        assert (seq, split_file) == (int(nn), "/s/odom/test_files_%s.txt" % nn)
        assert (root, poses) == ("/data/odom", "/data/odom/poses/%s.txt" % nn)
    for bad in ("eigen", "odom_11", "odom_x", "odom_-1", "odom"):
        with pytest.raises(ValueError):
            evaluation.odom_sequence(bad)


def _opt(tmp_path, kt, **kw):
    base = dict(eval_split="odom_9", splits_dir=str(tmp_path / "splits"), kt_path=kt, odom_path=None, height=32, width=64,
                skip_frame=2, track_length=1, cuda=0, num_layers=18, load_weights_folder="None", num_workers=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_evaluate_pose_checks_frames_and_ground_truth_before_any_launch(tmp_path):
    """`evaluate_pose` itself cannot run on the CPU tier: between the loader and `pose_ate` it calls `ops.gather_pairs`
    and `ops.pose_matrix`, which have no host port, and it places the frame pool on `cuda:<opt.cuda>`.  Its end-to-end
    runs are in the GPU tier (tests/test_gpu_odom.py).  What runs before the first launch is checked here, on a machine
    without a GPU: a frame missing in the middle, and more windows than the ground truth covers."""
    kt, root = _tree(tmp_path, frames=12, missing=(6,))
    oc.write_split(str(tmp_path / "splits"), 9, ["9 %d l" % t for t in range(11)])
    with pytest.raises(FileNotFoundError, match="000006.jpg"):
        evaluation.evaluate_pose(_opt(tmp_path, kt), gt_poses=np.zeros((12, 12)))
    oc.write_sequence(root, 9, [6])
    with pytest.raises(ValueError, match=r"N = 10 .* 11 poses \(M - S = 9\)"):
        evaluation.evaluate_pose(_opt(tmp_path, kt), gt_poses=np.zeros((11, 12)))
    os.makedirs(os.path.join(root, "poses"))
    with open(os.path.join(root, "poses", "09.txt"), "w") as f:               # the default ground truth: <odom>/poses/09.txt
        f.write("1 0 0 0 0 1 0 0 0 0 1 0\n" * 5)
    with pytest.raises(ValueError, match=r"N = 10 .* 5 poses \(M - S = 3\)"):
        evaluation.evaluate_pose(_opt(tmp_path, kt))


def test_root_script_is_the_command_line(tmp_path):
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_pose.py"), "--eval_split", "eigen"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "odom_0 ... odom_10" in r.stderr
