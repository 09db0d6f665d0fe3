#!/usr/bin/env python3
"""Measurements of the geometry-consistency loss on the GPU (profiles/geo_consistency/README.md).

    python tools/geo_bench.py --kernel [--batch 12] [--calls 20] [--out FILE.json]
        HIP events around each of `--calls` `bbd_geo_fwd` calls and as many `bbd_geo_bwd` calls after 2 warm-up calls
        (the means), on buffers allocated beforehand: `--batch` target frames of 192 x 640 of a synthetic street (a road
        1.65 m below the camera, walls 6 m to either side), V = 2 sources 0.8 m behind and ahead with a slight turn, the
        source depths 6 % larger, without the optional err and code outputs - the call the trainer makes.  A forward call
        is two launches, a backward call three.  The times are set against the byte model of DESIGN.md 6o at the
        6 076 GB/s float4 copy rate of DESIGN.md 3.
    python tools/geo_bench.py --step [--batch 12] [--steps 20] [--weight 0.5] [--out FILE.json]
        wall time per MD2 training step (ResNet-18, frames 0 -1 1, step graph) on one synthetic batch, with
        --geometry_consistency 0 and with `--weight`: the mean over `--steps` steps after the capture and 5 more steps.
"""
import argparse
import json
import math
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, V = 192, 640, 2
COPY_GBPS = 6076.0


def camera():
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    return K.astype(np.float32), np.linalg.inv(K).astype(np.float32)


def pose(tx, tz, yaw):
    P = np.eye(4)
    P[:3, :3] = [[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]]
    P[:3, 3] = (tx, 0.0, tz)
    return P


def depth_of(P, inv_K):
    """Depth float64 [H,W] of the street (road, two walls, nothing beyond 80 m) seen from camera-to-world pose P."""
    iK = np.asarray(inv_K, np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([iK[j, 0] * u + iK[j, 1] * v + iK[j, 2] for j in range(3)], -1)
    d = rays @ P[:3, :3].T
    x0 = P[0, 3]
    with np.errstate(all="ignore"):
        road = np.where(d[..., 1] > 1e-9, 1.65 / d[..., 1], np.inf)
        wall = np.where(d[..., 0] > 1e-9, (6.0 - x0) / d[..., 0], np.where(d[..., 0] < -1e-9, (-6.0 - x0) / d[..., 0], np.inf))
    return np.minimum(np.minimum(road, wall), 80.0)


def scene(B):
    K, inv_K = camera()
    q_tgt, q_src, T = np.empty((B, H, W), np.float32), np.empty((V, B, H, W), np.float32), np.empty((V, B, 12), np.float32)
    for b in range(B):
        tgt = pose(0.05 * b, 0.3 * b, 0.01 * b)
        q_tgt[b] = 1.0 / depth_of(tgt, inv_K)
        for v, k in enumerate((-1.0, 1.0)):
            src = pose(0.05 * b + 0.1 * k, 0.3 * b + 0.8 * k, 0.01 * b + 0.03 * k)
            q_src[v, b] = 1.0 / (1.06 * depth_of(src, inv_K))
            T[v, b] = (np.linalg.inv(src) @ tgt)[:3].reshape(12)
    return q_tgt, q_src, T, np.tile(K.reshape(1, 16), (B, 1)), np.tile(inv_K.reshape(1, 16), (B, 1))


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


def kernel(B, calls):
    from baseboostdepth_amd import _lib, ops
    dev = torch.device("cuda:0")
    q_tgt, q_src, T, K, inv_K = (torch.from_numpy(a).to(dev) for a in scene(B))
    res = ops.geometry_consistency(q_tgt, q_src, T, K, inv_K)                   # the wrapper: allocations and all
    lib, ptr = ops.default_backend().lib, _lib.ptr
    fw, bw = ops.geo_scratch_words(B, H, W, V, False), ops.geo_scratch_words(B, H, W, V, True)
    scratch = torch.empty(bw, dtype=torch.int64, device=dev)
    pair_sum, pair_count = torch.empty_like(res.pair_sum), torch.empty_like(res.pair_count)
    g = torch.full((V, B), 1.0 / float(res.pair_count.sum()), dtype=torch.float64, device=dev)
    grads = [torch.empty_like(q_tgt), torch.empty_like(q_src), torch.empty_like(T)]
    ins = [ptr(q_tgt), ptr(q_src), ptr(T), ptr(K), ptr(inv_K)]
    fwd_ms = timed(lambda: lib.call("bbd_geo_fwd", *ins, ptr(pair_sum), ptr(pair_count), ptr(None), ptr(None), ptr(scratch),
                                    fw, B, H, W, V, lib.stream_for(q_tgt)), calls)
    bwd_ms = timed(lambda: lib.call("bbd_geo_bwd", *ins, ptr(g), *[ptr(t) for t in grads], ptr(scratch), bw, B, H, W, V,
                                    lib.stream_for(q_tgt)), calls)
    n = V * B * H * W
    # forward: q_tgt and q_src read once per sample.  backward: the tap sums cleared (8 B), both maps read (8 B), every tap
    # sum read and written once by the atomics if they met in cache (16 B), read again and grad_q_src written (12 B), and
    # grad_q_tgt written once per pixel
    fwd_bytes, bwd_bytes = n * 8, n * (8 + 8 + 16 + 12) + B * H * W * 4
    model = lambda b: b / (COPY_GBPS * 1e9) * 1e3                               # noqa: E731
    return {"batch": B, "size": [H, W], "views": V, "calls": calls, "fwd_ms": fwd_ms, "bwd_ms": bwd_ms,
            "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes, "copy_GBps": COPY_GBPS, "fwd_model_ms": model(fwd_bytes),
            "bwd_model_ms": model(bwd_bytes), "fwd_ratio_to_model": fwd_ms / model(fwd_bytes),
            "bwd_ratio_to_model": bwd_ms / model(bwd_bytes), "loss": float(res.loss),
            "visible_share": float(res.pair_count.sum()) / n, "same_sum_again": bool(torch.equal(pair_sum, res.pair_sum)),
            "grad_T_max": float(grads[2].abs().max()), "device": torch.cuda.get_device_name(0)}


def step(B, steps, weight):
    from baseboostdepth_amd.synthetic import synthetic_batch
    from baseboostdepth_amd.trainer import Trainer
    out = {"batch": B, "size": [H, W], "steps": steps, "device": torch.cuda.get_device_name(0)}
    batch = synthetic_batch([1] * B, H, W, [0, 1, 2, 3], device="cuda:0", seed=3)
    for name, w in (("off", 0.0), ("on", weight)):
        opt = types.SimpleNamespace(
            height=H, width=W, batch_size=B, scales=[0, 1, 2, 3], frame_ids=[0, -1, 1], min_depth=0.1, max_depth=100.0,
            disparity_smoothness=1e-3, no_ssim=False, trimin=False, decomp=False, pose_error=5.5, incremental_skip=False,
            partial_skip=False, materialize_warps=False, num_layers=18, weights_init="scratch", learning_rate=1e-4,
            no_cuda=False, cuda=0, load_weights_folder="None", log_dir="/tmp", model_name="t", step_graph=True,
            geometry_consistency=w)
        torch.manual_seed(0)
        tr = Trainer(opt)
        tr.set_train()
        for _ in range(6):
            _, losses = tr.train_step(dict(batch))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            _, losses = tr.train_step(dict(batch))
        torch.cuda.synchronize()
        out["ms_per_step_" + name] = (time.perf_counter() - t0) / steps * 1e3
        out["loss_" + name] = float(losses["loss"])
        out["replays_" + name] = tr.graph_stats["replays"]
        if w > 0:
            out["weight"], out["loss_geometry"] = w, float(losses["loss/geometry"])
        del tr
    out["extra_ms_per_step"] = out["ms_per_step_on"] - out["ms_per_step_off"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        raise SystemExit("geo_bench: no GPU - nothing is measured without one")
    if a.kernel == a.step:
        raise SystemExit("geo_bench: one of --kernel and --step")
    result = kernel(a.batch, a.calls) if a.kernel else step(a.batch, a.steps, a.weight)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
