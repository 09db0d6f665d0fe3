#!/usr/bin/env python3
"""Measurements of the KITTI odometry evaluation on the GPU (profiles/odom/README.md).

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/odom_bench.py --kernel
        20 `bbd_pose_ate` calls on the `big` golden case (702 poses, 700 windows): the kernel times are in the trace
    python tools/odom_bench.py --e2e [--frames 1591] [--out profiles/odom/odom_bench.json]
        wall time of `evaluation.evaluate_pose` on a synthetic sequence (KITTI-sized JPEGs, 1590 split lines, a poses file)
        at 192 x 640 with ResNet-18 + PoseDecoder on closed-form weights: first call (kernel selection included) and a
        second one
    python tools/odom_bench.py --trajectory [--out profiles/odom/odom_bench.json]
        kernel time of one `bbd_pose_trajectory` call (four launches, HIP events around 50 calls after 5 warm-up calls)
        for J = 1590 steps (sequence 09) and J = 4540 (sequence 00), sim3, the devkit's lengths; the result is added to
        `--out` under "trajectory"
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def kernel():
    import odom_checks as oc
    from baseboostdepth_amd import evaluation
    v = oc.load()
    with tempfile.TemporaryDirectory() as tmp:
        gt = torch.from_numpy(oc.gt_global(v, "big", tmp)).cuda()
    poses = torch.from_numpy(v["big/poses"]).cuda()
    for _ in range(20):
        res = evaluation.pose_ate(poses, gt, skip=2, track_length=1)
    torch.cuda.synchronize()
    print("summary", res.summary.cpu().numpy().tolist())


def e2e(frames, out):
    from PIL import Image
    from fake_nets import fill_deterministic
    from baseboostdepth_amd import evaluation, networks
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "data", "odom")
        d = os.path.join(root, "sequences", "09", "image_2", "data")
        os.makedirs(d)
        os.makedirs(os.path.join(root, "poses"))
        t0 = time.perf_counter()
        base = rng.integers(0, 256, (376 // 8 + 1, 1241 // 8 + 40, 3)).astype(np.uint8)
        big = np.asarray(Image.fromarray(base).resize((1241 + 8 * 39, 376), Image.BILINEAR))
        for t in range(frames):                                   # a window sliding over one picture: cheap, distinct frames
            shift = (t * 7) % (8 * 39)
            Image.fromarray(big[:, shift:shift + 1241]).save(os.path.join(d, "%06d.jpg" % t), quality=90)
        with open(os.path.join(root, "poses", "09.txt"), "w") as f:
            for t in range(frames):
                a = 0.002 * t
                row = [math.cos(a), 0, math.sin(a), 0.05 * t, 0, 1, 0, 0, -math.sin(a), 0, math.cos(a), 0.8 * t]
                f.write(" ".join("%.6e" % x for x in row) + "\n")
        splits = os.path.join(tmp, "splits", "odom")
        os.makedirs(splits)
        with open(os.path.join(splits, "test_files_09.txt"), "w") as f:
            f.write("".join("9 %d l\n" % t for t in range(frames - 1)))
        weights = os.path.join(tmp, "weights")
        os.makedirs(weights)
        enc = fill_deterministic(networks.ResnetEncoder(18, False, 2))
        torch.save(enc.state_dict(), os.path.join(weights, "pose_encoder.pth"))
        torch.save(fill_deterministic(networks.PoseDecoder(enc.num_ch_enc, 1, 2), phase=0.3).state_dict(),
                   os.path.join(weights, "pose.pth"))
        made = time.perf_counter() - t0
        opt = types.SimpleNamespace(eval_split="odom_9", splits_dir=os.path.join(tmp, "splits"), kt_path=os.path.join(tmp, "data", "kitti"),
                                    odom_path=None, height=192, width=640, skip_frame=2, track_length=1, cuda=0, num_layers=18,
                                    load_weights_folder=weights, num_workers=16)
        walls = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluation.evaluate_pose(opt)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
    result = {"frames": frames, "windows": int(res["pred_poses"].shape[0]), "size": [192, 640], "batch_windows": 64,
              "wall_s_first_call": walls[0], "wall_s_second_call": walls[1], "make_sequence_s": made,
              "ate_mean": res["ate_mean"], "ate_chained_mean": res["ate_chained_mean"],
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)


def trajectory(out, sizes=(1590, 4540), warmup=5, calls=50):
    from baseboostdepth_amd import evaluation
    rows = []
    for J in sizes:
        G = np.tile(np.eye(4), (J + 1, 1, 1))
        for t in range(J + 1):                                    # a wide arc, 0.8 m per frame
            a = 0.002 * t
            G[t, :3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
            G[t, :3, 3] = [400 * (1 - math.cos(a)), 0.01 * math.sin(0.05 * t), 400 * math.sin(a)]
        rel = np.linalg.inv(G[:-1]) @ G[1:]
        rel[:, :3, 3] *= 0.5                                      # a monocular network's scale
        steps = torch.from_numpy(np.linalg.inv(rel).astype(np.float32)).cuda().reshape(J, 16)
        gt = torch.from_numpy(G[:, :3].reshape(J + 1, 12)).cuda()
        res = evaluation.pose_trajectory(steps, gt)
        for _ in range(warmup):
            evaluation.pose_trajectory_into(steps, gt, evaluation.KITTI_LENGTHS, res, 10, "sim3")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            evaluation.pose_trajectory_into(steps, gt, evaluation.KITTI_LENGTHS, res, 10, "sim3")
        stop.record()
        torch.cuda.synchronize()
        summary = res.summary.cpu().numpy()
        rows.append({"J": J, "calls": calls, "us_per_call": start.elapsed_time(stop) * 1000.0 / calls,
                     "t_rel_percent": 100 * float(summary[0]), "pairs": int(summary[2]), "scale": float(summary[6])})
    result = {"align": "sim3", "lengths": list(evaluation.KITTI_LENGTHS), "step": 10, "timing": "HIP events, host launch "
              "overhead of 4 launches per call included when it exceeds the kernels", "sizes": rows,
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        whole = {}
        if os.path.isfile(out):
            with open(out) as f:
                whole = json.load(f)
        whole["trajectory"] = result
        with open(out, "w") as f:
            json.dump(whole, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--trajectory", action="store_true")
    ap.add_argument("--frames", type=int, default=1591)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "these are GPU measurements"
    if args.kernel:
        kernel()
    if args.e2e:
        e2e(args.frames, args.out)
    if args.trajectory:
        trajectory(args.out)
