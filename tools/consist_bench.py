#!/usr/bin/env python3
"""Measurements of depth-pose consistency on the GPU (profiles/consist/README.md).

    python tools/consist_bench.py --kernel [--frames 200] [--calls 20] [--out profiles/consist/consist_bench.json]
        HIP events around each of `--calls` `bbd_depth_consistency` calls after 2 warm-up calls (the mean), on buffers
        allocated beforehand: `--frames` frames of 192 x 640 of a synthetic street (a road 1.65 m below the camera, walls
        6 m to either side, a drive of 0.8 m per frame with a slow turn), V = 2 (the frame before and the frame after),
        all four per-pixel outputs.  A call is its two launches; the transform launch handles frames * 2 pairs.  The
        launches' own times come from a `rocprofv3 --kernel-trace --stats` run of this mode (a run of its own).
        The time is set against the byte model of DESIGN.md 6m at the 6 076 GB/s float4 copy rate of DESIGN.md 3: per
        pixel 4 B read and 10 B written, and the taps once per frame (4 B per pixel more).
    python tools/consist_bench.py --e2e [--frames 200] [--map_consistent] [--tree DIR] [--out FILE.json]
        wall time of `evaluation.evaluate_pose(..., trajectory, save_map)` - with `--map_consistent` also the consistency
        pass - on a synthetic sequence of `--frames` frames at 192 x 640 held in device memory, ResNet-18 pose and depth
        networks on closed-form weights (their outputs squashed to a plausible drive and depth ramp): a first call (kernel selection included) and the mean of three more.
        `--tree DIR` imports the package from another checkout of this repository (the parent commit, to compare with).
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
H, W = 192, 640
COPY_GBPS = 6076.0


def street(n, inv_K):
    """Disparity float32 [n,H,W] of the street seen from poses float64 [n,4,4]: 0.8 m per frame, 0.002 rad per frame."""
    iK = np.asarray(inv_K, np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([iK[j, 0] * u + iK[j, 1] * v + iK[j, 2] for j in range(3)], -1)
    rays = rays / rays[..., 2:3]
    disp, poses = np.empty((n, H, W), np.float32), np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        a = 0.002 * i
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        poses[i, :3, :3], poses[i, :3, 3] = R, (0.05 * math.sin(0.05 * i), 0.0, 0.8 * i)
        d = rays @ R.T
        x0 = poses[i, 0, 3]
        with np.errstate(all="ignore"):
            road = np.where(d[..., 1] > 1e-9, 1.65 / d[..., 1], np.inf)
            wall = np.where(d[..., 0] > 1e-9, (6.0 - x0) / d[..., 0],
                            np.where(d[..., 0] < -1e-9, (-6.0 - x0) / d[..., 0], np.inf))
        disp[i] = (1.0 / np.minimum(np.minimum(road, wall), 80.0)).astype(np.float32)
    return disp, poses


def timed(fn, calls):
    """Mean milliseconds of `fn` over `calls` calls after 2 warm-up calls (HIP events, a synchronise after each)."""
    total = 0.0
    for i in range(2 + calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        if i >= 2:
            total += start.elapsed_time(stop)
    return total / calls


def kernel(frames, calls, out):
    from baseboostdepth_amd import _lib, ops, pointcloud
    dev = torch.device("cuda:0")
    K, inv_K = pointcloud.camera_matrix(H, W)[:3, :3].copy(), pointcloud.intrinsics(H, W)
    disp, poses = street(frames, inv_K)
    disp, poses = torch.from_numpy(disp).to(dev), torch.from_numpy(poses).to(dev)
    sources = pointcloud.neighbour_sources(frames)
    res = ops.depth_consistency(disp, poses, K, inv_K, sources, want_err=True)          # the wrapper: allocations and all
    counters = res.counters.sum(0).cpu().tolist()
    lib, ptr = ops.default_backend().lib, _lib.ptr
    Kd, iKd, src = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (K, inv_K, sources))
    args = [ptr(disp), ptr(poses), ptr(None), ptr(Kd), ptr(iKd), ptr(src), ptr(res.transforms), ptr(res.seen), ptr(res.agree),
            ptr(res.err), ptr(res.filtered), ptr(res.counters), frames, H, W, 2, 0.05, 1, 0]
    call_ms = timed(lambda: lib.call("bbd_depth_consistency", *args, lib.stream_for(disp)), calls)
    again = res.counters.sum(0).cpu().tolist()
    wrapper_ms = timed(lambda: ops.depth_consistency(disp, poses, Kd, iKd, src, want_err=True), calls)
    px = frames * H * W
    stream_bytes, tap_bytes = px * (4 + 10), px * 4
    model_ms = (stream_bytes + tap_bytes) / (COPY_GBPS * 1e9) * 1e3
    result = {"frames": frames, "size": [H, W], "views": 2, "calls": calls, "call_ms": call_ms, "wrapper_ms": wrapper_ms,
              "stream_bytes": stream_bytes, "tap_bytes": tap_bytes, "copy_GBps": COPY_GBPS, "model_ms": model_ms,
              "ratio_to_model": call_ms / model_ms, "counters": counters, "counters_repeat": again == counters,
              "visible_share": counters[1] / (2.0 * counters[0] - 2 * H * W), "mean_err": counters[3] / 16777216.0 / counters[1],
              "device": torch.cuda.get_device_name(0)}
    return result


class CalmPose(torch.nn.Module):
    """A PoseDecoder on closed-form weights gives wild motions: its cost is kept, its output is squashed to a drive of
    0.8 m per frame along an arc with a little of the network's own signal on top."""

    def __init__(self, decoder):
        super().__init__()
        self.decoder = decoder

    def forward(self, features):
        axisangle, translation = self.decoder(features)
        ahead = torch.tensor([0.0, 0.0, -0.8], device=translation.device)
        turn = torch.tensor([0.0, -0.01, 0.0], device=translation.device)     # an arc: a straight line has no se3 alignment
        return (0.001 * torch.tanh(torch.nan_to_num(axisangle)) + turn,
                0.01 * torch.tanh(torch.nan_to_num(translation)) + ahead)


class CalmDepth(torch.nn.Module):
    """Likewise for the DepthDecoder: a ramp down the image (4 m at the bottom, 20 m at the top once scaled) plus a
    little of the network's output."""

    def __init__(self, decoder):
        super().__init__()
        self.decoder = decoder

    def forward(self, features):
        raw = torch.nan_to_num(self.decoder(features)[("disp", 0)]).clamp(0.0, 1.0)
        ramp = torch.linspace(0.0, 1.0, raw.shape[-2], device=raw.device).view(1, 1, -1, 1)
        return {("disp", 0): 0.004 + 0.02 * ramp + 0.001 * raw}


def e2e(frames, map_consistent, out, port=False):
    from fake_nets import fill_deterministic
    from baseboostdepth_amd import evaluation, networks
    dev = torch.device("cpu" if port else "cuda:0")
    backend = None
    if port:                                                       # a rehearsal without a GPU: no time means anything
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from ports import PortBackend
        backend = PortBackend()
    sync = (lambda: None) if port else torch.cuda.synchronize
    g = torch.Generator().manual_seed(0)
    base = torch.rand(3, H // 8, W // 8 + 40, generator=g)
    big = torch.nn.functional.interpolate(base[None], size=(H, W + 8 * 39), mode="bilinear", align_corners=False)[0]
    pool = torch.stack([big[:, :, (t * 7) % (8 * 39):(t * 7) % (8 * 39) + W] for t in range(frames)]).to(dev)
    gt = np.array([[math.cos(0.002 * t), 0, math.sin(0.002 * t), 0.05 * t, 0, 1, 0, 0, -math.sin(0.002 * t), 0,
                    math.cos(0.002 * t), 0.8 * t] for t in range(frames)])
    pose_enc = fill_deterministic(networks.ResnetEncoder(18, False, 2))
    pose_dec = CalmPose(fill_deterministic(networks.PoseDecoder(pose_enc.num_ch_enc, 1, 2), phase=0.3))
    enc = fill_deterministic(networks.ResnetEncoder(18, False), phase=0.6)
    dec = CalmDepth(fill_deterministic(networks.DepthDecoder(enc.num_ch_enc, [0]), phase=0.9))
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "odom", "sequences", "09", "image_2", "data")
        os.makedirs(d)
        for t in range(frames):                                    # the windows only ask whether the frames exist
            open(os.path.join(d, "%06d.jpg" % t), "wb").close()
        os.makedirs(os.path.join(tmp, "splits", "odom"))
        with open(os.path.join(tmp, "splits", "odom", "test_files_09.txt"), "w") as f:
            f.write("".join("9 %d l\n" % t for t in range(frames - 1)))
        flags = dict(map_consistent=True) if map_consistent else {}
        opt = types.SimpleNamespace(eval_split="odom_9", splits_dir=os.path.join(tmp, "splits"), kt_path=os.path.join(tmp, "kitti"),
                                    odom_path=None, height=H, width=W, skip_frame=2, track_length=1, cuda=0, num_layers=18,
                                    load_weights_folder="None", num_workers=0, trajectory=True, trajectory_align="se3",
                                    save_trajectory=None, save_map=os.path.join(tmp, "map.ply"), **flags)
        loader = [{("color", 0, 0): pool[lo:lo + 32]} for lo in range(0, frames, 32)]
        walls = []
        for _ in range(4):
            sync()
            t0 = time.perf_counter()
            res = evaluation.evaluate_pose(opt, dataloader=loader, gt_poses=gt, models=(pose_enc, pose_dec, enc, dec),
                                           backend=backend, device=dev)
            sync()
            walls.append(time.perf_counter() - t0)
    result = {"frames": frames, "size": [H, W], "map_consistent": bool(map_consistent), "wall_s_first_call": walls[0],
              "wall_s_later_calls": walls[1:], "wall_s_mean_later": sum(walls[1:]) / 3.0, "map_stats": res["map_stats"],
              "consistency": res.get("consistency"), "package": os.path.dirname(os.path.abspath(evaluation.__file__)),
              "traj_ate_rmse": res["traj_ate_rmse"], "step_z_mean": float(np.diff(res["traj_aligned"][:, 2, 3]).mean()),
              "device": "host port (rehearsal)" if port else torch.cuda.get_device_name(0)}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--map_consistent", action="store_true")
    ap.add_argument("--port", action="store_true", help="--e2e through the tests' host port on the CPU: a rehearsal")
    ap.add_argument("--tree", type=str, default=ROOT)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    for p in (os.path.join(ROOT, "tools"), os.path.abspath(a.tree)):
        sys.path.insert(0, p)
    if not torch.cuda.is_available() and not (a.e2e and a.port):
        raise SystemExit("consist_bench: no GPU - nothing is measured without one")
    result = kernel(a.frames, a.calls, a.out) if a.kernel else e2e(a.frames, a.map_consistent, a.out, a.port)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
