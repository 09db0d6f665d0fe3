#!/usr/bin/env python3
"""Golden vectors for the KITTI odometry evaluation, recorded from the reference's own `evaluate_pose.dump_xyz`,
`evaluate_pose.compute_ate` and `layers.transformation_from_parameters` (imported unmodified from the reference tree)
and a replay of evaluate_pose.py:101-116 (chained pose) and :125-162 (ground truth, tracks, mean / std) on CPU tensors.
Output: tests/golden/odom_cases.npz - data only.  Per case: the poses-file TEXT (so that parsing is under test), the
float32 matrices [1+S, N, 16] a pose network would have produced (section 0 direct, section 1+k the k-th single step), S,
the track lengths, and the reference's chained matrices, local ground truth, both ATE rows and their mean / std / count.

    python tools/make_golden_odom.py

Cases (M poses, N windows, skip S, track length L), each the smallest that still reaches its hazard
  straight    12 10 2 1      plain path; one row has a zero axis-angle
  curve       40 38 2 1, 5   car-like path offset to about (300, -20, 450) m: cancellation in inv(G_a) . G_b, rotations
                             that are not orthonormal after printing as %.6e, truncated tracks at the end for L = 5
  skip1       20 19 1 5      Monodepth2's protocol; chained == direct bit for bit
  skip3       16 13 3 1      three-factor chain order
  one_track    6  3 2 1      a single track
  no_track     6  2 2 1      count 0: NaN summary
  zero_pred   10  8 2 1      two windows with an exactly zero predicted translation: NaN ATE, NaN mean
  big        702 700 2 1     the summary's partial sums take several elements each, unevenly
  short_list  30 20 2 1      N < M - S

Asserted here, so that the reference alone stays inside what the tests demand (tests/odom_checks.py): outside zero_pred
every track has sum(pred^2) > 1e-6 and a finite ATE, and a second, independent float64 evaluation - Gauss-Jordan inverse
with partial pivoting, explicit sequential sums, plain Python floats - agrees with the reference within tol / 8, where
tol = 64 * 2^-52 * max(1, max|G|) is the tests' bound (derivation: DESIGN.md 6d).
"""
import io
import math
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

refshim.install_stubs()
sys.path.insert(0, refshim.REFERENCE_ROOT)
import evaluate_pose as ref  # noqa: E402
from layers import transformation_from_parameters  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "odom_cases.npz")

#        name        M    N   S  Ls      path      origin
CASES = [("straight", 12, 10, 2, (1,), "straight", (0.0, 0.0, 0.0)),
         ("curve", 40, 38, 2, (1, 5), "curve", (300.0, -20.0, 450.0)),
         ("skip1", 20, 19, 1, (5,), "curve", (12.0, -1.0, 30.0)),
         ("skip3", 16, 13, 3, (1,), "curve", (-40.0, 2.0, 75.0)),
         ("one_track", 6, 3, 2, (1,), "curve", (5.0, 0.0, 9.0)),
         ("no_track", 6, 2, 2, (1,), "curve", (5.0, 0.0, 9.0)),
         ("zero_pred", 10, 8, 2, (1,), "curve", (20.0, -3.0, 60.0)),
         ("big", 702, 700, 2, (1,), "curve", (150.0, -8.0, 220.0)),
         ("short_list", 30, 20, 2, (1,), "curve", (-75.0, 4.0, 110.0))]
ZERO_WINDOWS = (1, 4)


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def trajectory(rng, M, path, origin):
    """Camera-to-world poses [M,3,4] of a car: z forward, yaw about y, a little pitch; about 0.8 m per frame."""
    poses, yaw, pos = [], 0.0, np.array(origin, np.float64)
    rate = 0.0
    for k in range(M):
        R = rot_y(yaw) @ rot_x(0.004 * math.sin(0.3 * k) if path == "curve" else 0.0)
        poses.append(np.concatenate([R, pos[:, None]], 1))
        if path == "curve":
            rate = 0.85 * rate + 0.15 * rng.uniform(-0.06, 0.08)
            yaw += rate
        pos = pos + R @ np.array([rng.normal(0, 0.004), rng.normal(0, 0.003), 0.8 + rng.normal(0, 0.05)])
    return np.stack(poses)


def poses_text(G):
    return "".join(" ".join("%.6e" % v for v in row.reshape(-1)) + "\n" for row in G)


def network_outputs(rng, G4, a, b):
    """(axisangle, translation) float32 [1,1,3] a monocular pose network could give for frames (a, b): the true relative
    motion at an arbitrary scale, with noise."""
    rel = np.linalg.inv(np.linalg.inv(G4[a]) @ G4[b])
    yaw = math.atan2(rel[0, 2], rel[2, 2])
    aa = np.array([rng.normal(0, 0.002), yaw + rng.normal(0, 0.003), rng.normal(0, 0.002)])
    tr = 0.031 * rel[:3, 3] + rng.normal(0, 0.0015, 3)
    return (torch.tensor(aa, dtype=torch.float32).view(1, 1, 3), torch.tensor(tr, dtype=torch.float32).view(1, 1, 3))


# ---- the second, independent evaluation: plain Python floats (IEEE double, no FMA), sequential sums
def py_matmul(a, b):
    out = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            acc = a[i][0] * b[0][j]
            for k in range(1, 4):
                acc = acc + a[i][k] * b[k][j]
            out[i][j] = acc
    return out


def py_inverse(a):
    m = [list(map(float, a[i])) + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for col in range(4):
        p = max(range(col, 4), key=lambda r: (abs(m[r][col]), -r))
        m[col], m[p] = m[p], m[col]
        pivot = m[col][col]
        m[col] = [v / pivot for v in m[col]]
        for r in range(4):
            if r != col:
                f = m[r][col]
                m[r] = [v - f * w for v, w in zip(m[r], m[col])]
    return [row[4:] for row in m]


def py_ate(pred, gt):
    eye = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    P, G, ps, gs = eye, eye, [[0.0] * 3], [[0.0] * 3]
    for p, g in zip(pred, gt):
        P, G = py_matmul(P, [[float(v) for v in row] for row in p]), py_matmul(G, g)
        ps.append([P[c][3] for c in range(3)])
        gs.append([G[c][3] for c in range(3)])
    sgp = spp = 0.0
    for p, g in zip(ps, gs):
        for c in range(3):
            sgp, spp = sgp + g[c] * p[c], spp + p[c] * p[c]
    if spp == 0.0:
        return float("nan"), spp
    scale, se = sgp / spp, 0.0
    for p, g in zip(ps, gs):
        for c in range(3):
            se = se + (p[c] * scale - g[c]) ** 2
    return math.sqrt(se) / len(ps), spp


def py_mean_std(x):
    if not len(x):
        return float("nan"), float("nan")
    s = 0.0
    for v in x:
        s = s + v
    mean, q = s / len(x), 0.0
    for v in x:
        q = q + (v - mean) * (v - mean)
    return mean, math.sqrt(q / len(x))


def close(a, b, bound):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and (a.size == 0 or nan.all() or float(np.abs(a - b)[~nan].max()) <= bound)


def main():
    out = {}
    for number, (name, M, N, S, Ls, path, origin) in enumerate(CASES):
        rng = np.random.default_rng(1000 + number)
        text = poses_text(trajectory(rng, M, path, origin))
        # ---- evaluate_pose.py:125-128
        gt_global_poses = np.loadtxt(io.StringIO(text)).reshape(-1, 3, 4)
        tol = 64 * 2.0 ** -52 * max(1.0, float(np.abs(gt_global_poses).max()))
        gt_global_poses = np.concatenate((gt_global_poses, np.zeros((gt_global_poses.shape[0], 1, 4))), 1)
        gt_global_poses[:, 3, 3] = 1
        assert gt_global_poses.shape == (M, 4, 4)
        # ---- the pose network's outputs through the reference's transformation_from_parameters, :87-116
        skip_frame = S
        pred_poses, pred_poses_multi, sections = [], [], [[] for _ in range(1 + S)]
        for i in range(N):
            steps_in = [network_outputs(rng, gt_global_poses, i + k, i + k + 1) for k in range(S)]
            direct_in = steps_in[0] if S == 1 else network_outputs(rng, gt_global_poses, i, i + S)
            if name == "straight" and i == 3:
                direct_in = (torch.zeros(1, 1, 3), direct_in[1])
                steps_in[1] = (torch.zeros(1, 1, 3), steps_in[1][1])
            if name == "zero_pred" and i in ZERO_WINDOWS:
                direct_in = (direct_in[0], torch.zeros(1, 1, 3))
                steps_in = [(aa, torch.zeros(1, 1, 3)) for aa, _ in steps_in]
            direct = transformation_from_parameters(*direct_in)
            pred_poses.append(direct.cpu().numpy())
            pred_poses_multi_step = [transformation_from_parameters(*s) for s in steps_in]
            T_rel_cumulative = torch.eye(4)
            for pose_step in pred_poses_multi_step[::-1]:
                T_rel_cumulative = torch.matmul(T_rel_cumulative, pose_step)
            pred_poses_multi.append(T_rel_cumulative.cpu().numpy())
            sections[0].append(direct.numpy().reshape(16))
            for k, s in enumerate(pred_poses_multi_step):
                sections[1 + k].append(s.numpy().reshape(16))
        pred_poses = np.concatenate(pred_poses)
        pred_poses_multi = np.concatenate(pred_poses_multi)
        poses = np.asarray(sections, np.float32).reshape(1 + S, N, 16)
        assert pred_poses.dtype == np.float32 and pred_poses_multi.shape == (N, 4, 4)
        if S == 1:
            assert np.array_equal(pred_poses.view(np.uint32), pred_poses_multi.view(np.uint32))
        # ---- :130-146
        gt_local_poses = []
        for i in range(skip_frame, len(gt_global_poses)):
            gt_local_poses.append(
                np.linalg.inv(np.dot(np.linalg.inv(gt_global_poses[i - skip_frame]), gt_global_poses[i])))
        py_local = [py_inverse(py_matmul(py_inverse(gt_global_poses[j].tolist()), gt_global_poses[j + S].tolist()))
                    for j in range(M - S)]
        assert close(gt_local_poses, py_local, tol / 8), (name, np.abs(np.array(gt_local_poses) - np.array(py_local)).max())
        out[name + "/text"] = np.array(text)
        out[name + "/poses"] = poses
        out[name + "/S"] = np.int32(S)
        out[name + "/Ls"] = np.asarray(Ls, np.int32)
        out[name + "/chained"] = pred_poses_multi.reshape(N, 16)
        out[name + "/gt_local"] = np.asarray(gt_local_poses, np.float64).reshape(M - S, 16)
        for track_length in Ls:
            assert track_length == 1 or N == M - S        # the slices of :155-157 then have equal lengths
            # ---- :149-162
            ates, ates_2 = [], []
            num_frames = pred_poses.shape[0]
            for i in range(0, num_frames - skip_frame):
                local_xyzs = np.array(ref.dump_xyz(pred_poses[i:i + track_length]))
                local_xyzs_2 = np.array(ref.dump_xyz(pred_poses_multi[i:i + track_length]))
                gt_local_xyzs = np.array(ref.dump_xyz(gt_local_poses[i:i + track_length]))
                with np.errstate(invalid="ignore"):
                    ates.append(ref.compute_ate(gt_local_xyzs, local_xyzs))
                    ates_2.append(ref.compute_ate(gt_local_xyzs, local_xyzs_2))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                summary = np.array([[np.mean(a), np.std(a), len(a)] for a in (ates, ates_2)], np.float64)
            rows = np.asarray([ates, ates_2], np.float64).reshape(2, max(N - S, 0))
            # ---- conditions + the second evaluation
            for r, mats in enumerate((pred_poses, pred_poses_multi)):
                mine = [py_ate(mats[i:i + track_length], py_local[i:i + len(mats[i:i + track_length])])
                        for i in range(N - S)]
                for i, (ate, spp) in enumerate(mine):
                    if name == "zero_pred" and i in ZERO_WINDOWS:
                        assert spp == 0.0 and np.isnan(rows[r, i]), (name, r, i)
                    else:
                        assert spp > 1e-6 and np.isfinite(rows[r, i]), (name, r, i, spp, rows[r, i])
                assert close(rows[r], [a for a, _ in mine], tol / 8), (name, track_length, r)
                assert close(summary[r, :2], py_mean_std([a for a, _ in mine]), tol / 8), (name, track_length, r)
            out["%s/L%d/ates" % (name, track_length)] = rows
            out["%s/L%d/summary" % (name, track_length)] = summary
            print("%-10s M %3d N %3d S %d L %d: tol %.2e, direct %s, chained %s"
                  % (name, M, N, S, track_length, tol, summary[0, :2], summary[1, :2]))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size // 1024, "KB")
    assert size < 1 << 20, "a committed file must stay under 1 MiB"


if __name__ == "__main__":
    main()
