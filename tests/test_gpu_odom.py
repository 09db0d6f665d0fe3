"""GPU tier of the KITTI odometry evaluation: bbd_pose_ate through `evaluation.pose_ate` against the reference's results
(acceptance rules: tests/odom_checks.py) and against the host port bit for bit, and `evaluation.evaluate_pose` end to end:
with element-wise stand-ins for the pose network (whose results do not depend on the batch size, to the bit) against a
window-by-window loop, and with the real ResNet-18 pose network through the root evaluate_pose.py as a child process
under `timeout`."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import odom_checks as oc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def v():
    return oc.load()


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.mark.parametrize("case,L", oc.EVERY)
def test_device_matches_the_reference_the_host_port_and_itself(v, port, tmp_path, case, L):
    from baseboostdepth_amd import ops
    res, gt = oc.run(v, case, L, ops.default_backend(), DEV, tmp_path)
    assert all(getattr(res, k).is_cuda for k in oc.FIELDS)
    oc.check(v, case, L, res, gt)
    got = oc.host(res)
    again, _ = oc.run(v, case, L, ops.default_backend(), DEV, tmp_path)
    again = oc.host(again)
    on_host, _ = oc.run(v, case, L, port, "cpu", tmp_path)
    on_host = oc.host(on_host)
    for k in oc.FIELDS:
        assert oc.same_bytes(got[k], again[k]), "%s: two identical calls differ" % k
        assert oc.same_bytes(got[k], on_host[k]), "%s: device and host port differ" % k


@pytest.mark.parametrize("case", ["no_track", "one_track", "big"])
def test_outputs_are_written_whole_and_nothing_else(v, tmp_path, case):
    from baseboostdepth_amd import evaluation, ops
    M, N, S, _ = oc.SHAPES[case]
    gt = torch.from_numpy(oc.gt_global(v, case, tmp_path)).to(DEV)
    poses = torch.from_numpy(v[case + "/poses"]).to(DEV)
    sizes = {"chained": (N * 16, torch.float32), "gt_local": ((M - S) * 16, torch.float64),
             "ates": (2 * max(N - S, 0), torch.float64), "summary": (8, torch.float64)}
    bufs = {k: torch.full((n + 14,), float("nan"), dtype=dt, device=DEV) for k, (n, dt) in sizes.items()}
    views = {k: bufs[k][7:7 + n] for k, (n, _) in sizes.items()}
    evaluation.pose_ate_into(poses, gt, views["chained"], views["gt_local"], views["ates"], views["summary"], S, 1)
    for k, (n, _) in sizes.items():
        assert bool(torch.isnan(bufs[k][:7]).all()) and bool(torch.isnan(bufs[k][7 + n:]).all()), k
    want, _ = oc.run(v, case, 1, ops.default_backend(), DEV, tmp_path)
    for k in ("chained", "gt_local", "ates", "summary"):
        assert oc.same_bytes(views[k].cpu().numpy(), getattr(want, k).cpu().numpy().reshape(-1)), k
    if case != "no_track":
        assert not any(bool(torch.isnan(views[k]).any()) for k in views)


def test_the_entry_point_refuses_bad_sizes_without_launching(v, tmp_path):
    from baseboostdepth_amd import _lib, evaluation
    gt = torch.from_numpy(oc.gt_global(v, "one_track", tmp_path)).to(DEV)
    poses = torch.from_numpy(v["one_track/poses"]).to(DEV)
    out = [torch.empty(64, dtype=dt, device=DEV) for dt in (torch.float32, torch.float64, torch.float64, torch.float64)]
    lib = _lib.get_lib()
    for N, M, S, L in ((3, 6, 0, 1), (3, 6, 2, 0), (-1, 6, 2, 1), (3, 4, 2, 1)):
        with pytest.raises(_lib.BbdError):
            lib.call("bbd_pose_ate", _lib.ptr(poses), _lib.ptr(gt), *[_lib.ptr(t) for t in out], N, M, S, L,
                     lib.stream_for(poses))
    with pytest.raises(ValueError, match=r"N = 3 > M - S = 2"):
        evaluation.pose_ate(poses, gt[:4])


# ---------------------------------------------------------------------------- evaluate_pose end to end
H, W = 32, 64


class PixelEncoder(torch.nn.Module):
    """Stands in for ResnetEncoder: hands the pair through."""
    num_ch_enc = np.array([6])

    def forward(self, x):
        return [x]


class PixelDecoder(torch.nn.Module):
    """Stands in for PoseDecoder(num_ch_enc, 1, 2): fixed pixels of the two frames times constants - element-wise only, so a
    row's result does not depend on the rows batched with it.  Output shapes [n, 2, 1, 3] like PoseDecoder's."""
    SPOTS = ((0, 3, 5), (1, 10, 20), (2, 7, 40), (1, 20, 33), (2, 28, 9), (0, 15, 60))

    def forward(self, input_features):
        x = input_features[0][-1]
        first = torch.stack([x[:, c, r, col] for c, r, col in self.SPOTS], 1)                  # [n, 6] of frame a
        second = torch.stack([x[:, 3 + c, r, col] for c, r, col in self.SPOTS], 1)             # [n, 6] of frame b
        diff = second - first
        axisangle = (diff[:, :3] * 0.11).view(-1, 1, 1, 3)
        translation = (diff[:, 3:] * 0.4 + second[:, :3] * 0.05).view(-1, 1, 1, 3)
        return torch.cat([axisangle, axisangle * 0.5], 1), torch.cat([translation, translation * 0.5], 1)


def _sequence(v, tmp_path, frames=14, missing=()):
    """A 14-frame sequence 9 with the first 14 poses of the `curve` case as its ground truth, and the options for it."""
    root = str(tmp_path / "data" / "odom")
    oc.write_sequence(root, 9, range(frames), missing=missing)
    oc.write_split(str(tmp_path / "splits"), 9, ["9 %d l" % t for t in range(frames - 1)])
    os.makedirs(os.path.join(root, "poses"), exist_ok=True)
    with open(os.path.join(root, "poses", "09.txt"), "w") as f:
        f.write("".join(l + "\n" for l in str(v["curve/text"]).splitlines()[:frames]))
    return types.SimpleNamespace(eval_split="odom_9", splits_dir=str(tmp_path / "splits"), kt_path=str(tmp_path / "data" / "kitti"),
                                 odom_path=None, height=H, width=W, skip_frame=2, track_length=1, cuda=0, num_layers=18,
                                 load_weights_folder="None", num_workers=2)


def test_evaluate_pose_equals_a_window_by_window_loop_for_any_chunking(v, port, tmp_path, capsys):
    from baseboostdepth_amd import datasets, evaluation, layers
    opt = _sequence(v, tmp_path)
    models = (PixelEncoder(), PixelDecoder())
    small = evaluation.evaluate_pose(opt, models=models, batch_windows=4)
    said = capsys.readouterr().out
    large = evaluation.evaluate_pose(opt, models=models, batch_windows=64)
    assert said.count("Trajectory error: ") == 2 and "std: " in said
    assert "Trajectory error: {:0.3f}, std: {:0.3f}".format(small["ate_mean"], small["ate_std"]) in said
    assert "Trajectory error: {:0.3f}, std: {:0.3f}".format(small["ate_chained_mean"], small["ate_chained_std"]) in said
    keys = ("ate_mean", "ate_std", "ate_chained_mean", "ate_chained_std", "ates", "pred_poses", "pred_poses_chained")
    assert sorted(small) == sorted(keys)
    S, N = 2, 12
    assert small["ates"].shape == (2, N - S) and small["pred_poses"].shape == (N, 4, 4) and small["pred_poses"].dtype == np.float32
    assert np.isfinite(small["ates"]).all() and small["ate_mean"] > 0
    # ---- the test's own loop: the same frames, one window and one network call at a time
    lines = datasets.KITTIOdomDataset(datasets.readlines(os.path.join(opt.splits_dir, "odom", "test_files_09.txt")), 0, H, W,
                                      kt_path=opt.kt_path, is_train=False, kt=True, naive_mix=True)
    frames, pairs, n_windows = lines.windows(S)
    assert n_windows == N and len(frames) == 14
    pool_set = datasets.KITTIOdomDataset(frames, 0, H, W, kt_path=opt.kt_path, is_train=False, kt=True, naive_mix=True)
    pool = datasets.DeviceCollate(H, W, [0], DEV)([pool_set[i] for i in range(len(pool_set))])[("color", 0, 0)]
    encoder, decoder = models
    poses = torch.empty(1 + S, N, 4, 4, device=DEV)
    with torch.no_grad():
        for i in range(N):
            for section, (a, b) in enumerate([(i, i + S)] + [(i + k, i + k + 1) for k in range(S)]):
                x = torch.cat([pool[a:a + 1], pool[b:b + 1]], 1)
                axisangle, translation = decoder([encoder(x)])
                poses[section, i] = layers.transformation_from_parameters(axisangle[:, 0], translation[:, 0])[0]
    gt = evaluation.read_poses_file(os.path.join(os.path.dirname(opt.kt_path), "odom", "poses", "09.txt"))
    loop = oc.host(evaluation.pose_ate(poses, gt, skip=S, track_length=1))
    on_host = oc.host(evaluation.pose_ate(poses.cpu(), gt, skip=S, track_length=1, backend=port))
    for k in oc.FIELDS:
        assert oc.same_bytes(loop[k], on_host[k]), "%s: device and host port differ on the same matrices" % k
    for out in (small, large):
        assert oc.same_bytes(out["pred_poses"], loop["direct"]) and oc.same_bytes(out["pred_poses_chained"], loop["chained"])
        assert oc.same_bytes(out["ates"], loop["ates"])
        got = np.array([[out["ate_mean"], out["ate_std"]], [out["ate_chained_mean"], out["ate_chained_std"]]])
        assert oc.same_bytes(got, np.ascontiguousarray(loop["summary"][:, :2]))


def test_root_script_with_the_real_pose_network_as_a_child_process(v, tmp_path):
    import re
    from fake_nets import fill_deterministic
    from baseboostdepth_amd import networks
    opt = _sequence(v, tmp_path)
    weights = str(tmp_path / "weights")
    os.makedirs(weights)
    encoder = fill_deterministic(networks.ResnetEncoder(18, False, 2))
    torch.save(encoder.state_dict(), os.path.join(weights, "pose_encoder.pth"))
    torch.save(fill_deterministic(networks.PoseDecoder(encoder.num_ch_enc, 1, 2), phase=0.3).state_dict(),
               os.path.join(weights, "pose.pth"))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "evaluate_pose.py"),
                        "--eval_split", "odom_9", "--load_weights_folder", weights, "--kt_path", opt.kt_path,
                        "--splits_dir", opt.splits_dir, "--height", str(H), "--width", str(W), "--num_workers", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    found = re.findall(r"Trajectory error: (\S+), std: (\S+)", r.stdout)
    print(r.stdout)
    assert len(found) == 2 and all(np.isfinite(float(a)) and np.isfinite(float(b)) for a, b in found), r.stdout


def test_gather_pairs_takes_strided_index_views():
    """Both index arguments as stride-2 views of one table: each is made contiguous inside `ops.gather_pairs` and has
    to stay alive until the launch (a temporary's memory is handed to the next allocation at once)."""
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(2)
    pool = torch.rand(9, 3, 4, 8, generator=gen).to(DEV)
    table = torch.randint(0, 9, (37, 2), generator=gen, dtype=torch.int32).to(DEV)
    a, b = table[:, 0], table[:, 1]
    assert not a.is_contiguous() and not b.is_contiguous()
    got = ops.gather_pairs(pool, a, b)
    want = torch.cat([pool[a.long()], pool[b.long()]], 1)
    assert torch.equal(got, want)


class _NeverMoved(torch.nn.Module):
    def to(self, *a, **k):
        raise AssertionError("the models were touched before the inputs were checked")


def test_missing_frame_and_short_ground_truth_are_errors_before_any_launch(v, tmp_path):
    from baseboostdepth_amd import evaluation
    opt = _sequence(v, tmp_path, missing=(6,))
    models = (_NeverMoved(), _NeverMoved())
    with pytest.raises(FileNotFoundError, match="000006.jpg"):
        evaluation.evaluate_pose(opt, models=models)
    oc.write_sequence(os.path.join(str(tmp_path), "data", "odom"), 9, [6])
    with pytest.raises(ValueError, match=r"N = 12 .* 13 poses \(M - S = 11\)"):
        evaluation.evaluate_pose(opt, models=models, gt_poses=np.zeros((13, 12)))
