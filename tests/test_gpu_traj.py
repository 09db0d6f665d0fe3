"""GPU tier of the full-trajectory odometry scores: bbd_pose_trajectory through `evaluation.pose_trajectory` against the
numpy reference (acceptance rules: tests/traj_checks.py) and against the host port - bit for bit on every output that is
not behind acos, within the r_err bound on those that are - and `evaluation.evaluate_pose --trajectory` with the real
ResNet-18 pose network: in process against the by-hand path, and once through the root script as a child process under
`timeout`."""
import ctypes
import os
import re
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
import traj_checks as tc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 12345.678


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.mark.parametrize("name,mode", tc.EVERY)
def test_device_matches_the_reference_the_host_port_and_itself(port, name, mode):
    from baseboostdepth_amd import ops
    res = tc.run(name, mode, ops.default_backend(), DEV)
    assert all(getattr(res, k).is_cuda for k in tc.FIELDS)
    got = tc.host(res)
    tol = tc.check(name, mode, got)
    again = tc.host(tc.run(name, mode, ops.default_backend(), DEV))
    for k in tc.FIELDS:
        assert tc.same_bytes(got[k], again[k]), "%s: two identical calls differ" % k
    on_host = tc.host(tc.run(name, mode, port, "cpu"))
    exact, angles = tc.behind_acos(got)
    exact_h, angles_h = tc.behind_acos(on_host)
    for k in exact:
        assert tc.same_bytes(exact[k], exact_h[k]), "%s: device and host port differ" % k
    for k in angles:
        tc._within(angles[k], angles_h[k], tol["r"], "r_err L", "%s/%s device / port %s" % (name, mode, k))
    print("worst / bound so far:", {k: round(v, 4) for k, v in tc.WORST.items()})


def _guarded(F, n_first, n_len):
    sizes = {"traj": F * 16, "gt_traj": F * 16, "aligned": F * 16, "transform": 16, "dist": F,
             "pairs": n_first * n_len * 4, "per_length": n_len * 3, "summary": 8}
    bufs = {k: torch.full((n + 14,), GUARD, dtype=torch.float64, device=DEV) for k, n in sizes.items()}
    return sizes, bufs, [bufs[k][7:7 + sizes[k]] for k in tc.FIELDS]


@pytest.mark.parametrize("name,mode", [("noisy257", "sim3"), ("no_pair", "se3"), ("zero", "scale"), ("single", "none")])
def test_outputs_are_written_whole_and_nothing_else(name, mode):
    from baseboostdepth_amd import evaluation, ops
    case = tc.make(name)
    F = case["J"] + 1
    sizes, bufs, views = _guarded(F, -(-F // tc.STEP), len(tc.LENGTHS))
    steps, gt = torch.from_numpy(case["steps"]).to(DEV), torch.from_numpy(case["gt"]).to(DEV)
    evaluation.pose_trajectory_into(steps, gt, tc.LENGTHS, views, tc.STEP, mode)
    want = tc.host(tc.run(name, mode, ops.default_backend(), DEV))
    for k, view in zip(tc.FIELDS, views):
        n = sizes[k]
        assert bool((bufs[k][:7] == GUARD).all()) and bool((bufs[k][7 + n:] == GUARD).all()), k
        assert tc.same_bytes(view.cpu().numpy(), want[k].reshape(-1)), k
        assert not bool((view == GUARD).any()), k


def test_the_entry_point_refuses_without_launching():
    from baseboostdepth_amd import _lib, evaluation
    case = tc.make("noisy63")
    steps, gt = torch.from_numpy(case["steps"]).to(DEV), torch.from_numpy(case["gt"]).to(DEV)
    outs = [torch.full((64 * 16,), GUARD, dtype=torch.float64, device=DEV) for _ in range(8)]
    lib = _lib.get_lib()
    for J, M, lengths, n_len, step, mode in tc.BAD:
        lens = (ctypes.c_double * len(lengths))(*lengths)
        with pytest.raises(_lib.BbdError):
            lib.call("bbd_pose_trajectory", _lib.ptr(steps), _lib.ptr(gt), ctypes.cast(lens, ctypes.c_void_p),
                     *[_lib.ptr(t) for t in outs], J, M, len(lengths) if n_len is None else n_len, step, mode,
                     lib.stream_for(steps))
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in outs)
    with pytest.raises(ValueError, match=r"M = 63 < J \+ 1 = 64"):
        evaluation.pose_trajectory(steps, gt[:63])


# ---------------------------------------------------------------------------- evaluate_pose end to end
H, W, FRAMES = 32, 64, 40


def _sequence(tmp_path, **flags):
    """A 40-frame sequence 9 with the first 40 poses of the `noisy63` case as its ground truth, and the options for it."""
    root = str(tmp_path / "data" / "odom")
    oc.write_sequence(root, 9, range(FRAMES))
    oc.write_split(str(tmp_path / "splits"), 9, ["9 %d l" % t for t in range(FRAMES - 1)])
    os.makedirs(os.path.join(root, "poses"), exist_ok=True)
    with open(os.path.join(root, "poses", "09.txt"), "w") as f:
        f.write("".join(l + "\n" for l in tc.make("noisy63")["text"].splitlines()[:FRAMES]))
    return types.SimpleNamespace(eval_split="odom_9", splits_dir=str(tmp_path / "splits"), kt_path=str(tmp_path / "data" / "kitti"),
                                 odom_path=None, height=H, width=W, skip_frame=2, track_length=1, cuda=0, num_layers=18,
                                 load_weights_folder="None", num_workers=2, **flags)


def _pose_network():
    from fake_nets import fill_deterministic
    from baseboostdepth_amd import networks
    encoder = fill_deterministic(networks.ResnetEncoder(18, False, 2))
    return encoder, fill_deterministic(networks.PoseDecoder(encoder.num_ch_enc, 1, 2), phase=0.3)


def test_evaluate_pose_trajectory_with_the_real_pose_network_equals_the_by_hand_path(port, tmp_path, capsys, monkeypatch):
    """The by-hand path: the matrices the network gave, chunk by chunk as `ops.pose_matrix` returned them, put in frame
    order by the test and handed to `pose_trajectory` - on the device, and on the host port bit for bit."""
    from baseboostdepth_amd import evaluation, ops
    opt = _sequence(tmp_path, trajectory=True, trajectory_align="sim3", save_trajectory=str(tmp_path / "aligned.txt"))
    chunks, real = [], ops.pose_matrix

    def spy(*a, **k):
        chunks.append(real(*a, **k))
        return chunks[-1]

    monkeypatch.setattr(ops, "pose_matrix", spy)
    out = evaluation.evaluate_pose(opt, models=_pose_network(), batch_windows=16)
    monkeypatch.undo()
    said = capsys.readouterr().out
    S, N = 2, FRAMES - 2
    assert len(chunks) == 3 and sum(c.shape[0] for c in chunks) == (1 + S) * N
    single = torch.cat([c.view(1 + S, -1, 16)[1] for c in chunks])                # frame pairs (i, i+1), i < N
    tail = chunks[-1].view(1 + S, -1, 16)[2, -1:]                                 # (N, N+1)
    steps = torch.cat([single, tail])
    assert steps.shape == (FRAMES - 1, 16)
    gt = evaluation.read_poses_file(os.path.join(str(tmp_path), "data", "odom", "poses", "09.txt"))
    want = tc.host(evaluation.pose_trajectory(steps, gt, align="sim3"))
    on_host = tc.host(evaluation.pose_trajectory(steps.cpu(), gt, align="sim3", backend=port))
    exact, _ = tc.behind_acos(want, evaluation.KITTI_LENGTHS)
    exact_h, _ = tc.behind_acos(on_host, evaluation.KITTI_LENGTHS)
    for k in exact:
        assert tc.same_bytes(exact[k], exact_h[k]), "%s: device and host port differ on the network's matrices" % k
    assert tc.same_bytes(out["traj_aligned"], want["aligned"]) and tc.same_bytes(out["traj_gt"], want["gt_traj"])
    assert tc.same_bytes(out["per_length"], want["per_length"])
    got = np.array([out["t_rel"], out["r_rel"], out["traj_ate_rmse"], out["traj_scale"]])
    assert tc.same_bytes(got, want["summary"][[0, 1, 3, 6]]) and np.isfinite(got[2:]).all()
    assert want["summary"][7] == FRAMES and np.isfinite(out["traj_aligned"]).all()
    assert said.count("Trajectory error: ") == 2 and said.count("Full trajectory (sim3, 40 frames): t_rel ") == 1
    saved = evaluation.read_poses_file(str(tmp_path / "aligned.txt"))
    assert saved.shape == (FRAMES, 12)
    assert np.abs(saved - want["aligned"].reshape(FRAMES, 16)[:, :12]).max() <= 1e-6 * max(1, np.abs(saved).max())


def test_root_script_with_trajectory_as_a_child_process(tmp_path):
    opt = _sequence(tmp_path)
    weights = str(tmp_path / "weights")
    os.makedirs(weights)
    encoder, decoder = _pose_network()
    torch.save(encoder.state_dict(), os.path.join(weights, "pose_encoder.pth"))
    torch.save(decoder.state_dict(), os.path.join(weights, "pose.pth"))
    saved = str(tmp_path / "aligned.txt")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "evaluate_pose.py"),
                        "--eval_split", "odom_9", "--load_weights_folder", weights, "--kt_path", opt.kt_path,
                        "--splits_dir", opt.splits_dir, "--height", str(H), "--width", str(W), "--num_workers", "2",
                        "--trajectory", "--trajectory_align", "se3", "--save_trajectory", saved],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert len(re.findall(r"Trajectory error: (\S+), std: (\S+)", r.stdout)) == 2
    found = re.findall(r"Full trajectory \(se3, 40 frames\): t_rel (\S+) %, r_rel (\S+) deg/100m, ATE (\S+) m, scale (\S+)",
                       r.stdout)
    assert len(found) == 1 and np.isfinite(float(found[0][2])) and float(found[0][3]) == 1.0, r.stdout
    assert np.loadtxt(saved).shape == (FRAMES, 12)
