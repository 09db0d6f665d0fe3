#!/usr/bin/env python3
"""Measurements of the scene map on the GPU (profiles/map/README.md).

    python tools/map_bench.py [--frames 200] [--stride 2] [--voxel 0.2] [--calls 5] [--out profiles/map/map_bench.json]

Workload: `--frames` frames of 192 x 640 at `--stride` (200 at stride 2: 6.1 M candidates), voxel 0.2, the poses of a
straight drive of 1 m per frame through a synthetic street (a road 1.65 m below the camera, walls 6 m to either side,
depth beyond 30 m dropped).  HIP events around each of `--calls` calls after 2 warm-up calls (the mean), for

    clear        `ops.map_clear` of a table of 2^24 slots
    accumulate   ONE `ops.map_accumulate` call of all frames into the cleared table, in both forms: the default, which
                 sums runs of equal keys inside a wave before it adds, and BBD_MAP_NO_MERGE (`merge=False`)
    finish       `ops.map_finish` (the three compaction launches; the ordering by key and the read-back are not in it)
    eager        the same fusion with PyTorch-ROCm ops on the same GPU, from per-point keys, offsets and colours that are
                 computed beforehand and not timed: `torch.unique(return_inverse=True)` + seven `index_add_`

and the atomic bytes per second of `accumulate` without merging (40 B per kept point: three 8-byte and four 4-byte adds; the
compare-and-swap of a voxel's first point is not counted) against the chip-wide rate of global FLOAT atomic adds,
1.3 TB/s of added bytes.  Whether integer atomics run at that rate is not known: the figure is a yardstick, not a roof.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 192, 640
FLOAT_ATOMIC_TBPS = 1.3
BYTES_PER_POINT = 3 * 8 + 4 * 4


def street(n, inv_K, dev):
    """Depth [n,H,W] of the synthetic street (the same for every frame: the street is straight), colours, poses."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    iK = torch.as_tensor(inv_K, dtype=torch.float64)
    rx = iK[0, 0] * xx + iK[0, 1] * yy + iK[0, 2]
    ry = iK[1, 0] * xx + iK[1, 1] * yy + iK[1, 2]
    road = torch.where(ry > 1e-6, 1.65 / ry.clamp_min(1e-6), torch.full_like(ry, 1e3))
    wall = 6.0 / rx.abs().clamp_min(1e-6)
    depth = torch.minimum(road, wall).clamp(max=80.0)
    g = torch.Generator().manual_seed(0)
    depth = (depth[None] * (1.0 + 0.01 * torch.rand(n, H, W, generator=g, dtype=torch.float64))).float()
    rgb = torch.rand(n, 3, H, W, generator=g)
    poses = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    poses[:, 2, 3] = torch.arange(n, dtype=torch.float64)
    return (1.0 / depth).to(dev), rgb.to(dev), poses.to(dev)


def eager_points(disp, rgb, poses, inv_K, stride, lo, hi, voxel):
    """Per-point keys, offsets and colour bytes with torch ops in float64 (not timed; the kept points only)."""
    d = (1.0 / disp[:, ::stride, ::stride]).double()
    yy, xx = torch.meshgrid(torch.arange(0, H, stride, device=disp.device, dtype=torch.float64),
                            torch.arange(0, W, stride, device=disp.device, dtype=torch.float64), indexing="ij")
    iK = torch.as_tensor(inv_K, dtype=torch.float64, device=disp.device)
    rays = torch.stack([iK[j, 0] * xx + iK[j, 1] * yy + iK[j, 2] for j in range(3)], -1)            # [h,w,3]
    x = rays[None] * d[..., None]
    X = torch.einsum("nij,nhwj->nhwi", poses[:, :3, :3], x) + poses[:, None, None, :3, 3]
    keep = (d >= lo) & (d <= hi)
    u = X[keep] / voxel
    v = torch.floor(u)
    q = ((u - v) * 65536.0).long()
    vi = v.long() + (1 << 20)
    key = (vi[:, 0] << 42) | (vi[:, 1] << 21) | vi[:, 2]
    col = (rgb[:, :, ::stride, ::stride].permute(0, 2, 3, 1)[keep] * 255.0 + 0.5).long().clamp(0, 255)
    return key, q, col


def eager_fuse(key, q, col):
    keys, inverse = torch.unique(key, return_inverse=True)
    M = keys.shape[0]
    sum_q = torch.zeros(M, 3, dtype=torch.int64, device=key.device)
    sum_c = torch.zeros(M, 4, dtype=torch.int64, device=key.device)
    for j in range(3):
        sum_q[:, j].index_add_(0, inverse, q[:, j])
        sum_c[:, j].index_add_(0, inverse, col[:, j])
    sum_c[:, 3].index_add_(0, inverse, torch.ones_like(inverse))
    return keys, sum_q, sum_c


def sorted_state(state):
    """Keys in ascending order with their sums: what does not depend on which slot a key took."""
    keys, order = torch.sort(state.keys)
    return keys, state.pos[order], state.col[order]


def timed(fn, calls, before=None):
    """Mean milliseconds of `fn` over `calls` calls after 2 warm-up calls; `before` runs ahead of each and is not timed."""
    total, out = 0.0, None
    for i in range(2 + calls):
        if before is not None:
            before()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        if i >= 2:
            total += start.elapsed_time(stop)
    return total / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from baseboostdepth_amd import ops, pointcloud
    if not torch.cuda.is_available():
        raise SystemExit("map_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    inv_K = pointcloud.intrinsics(H, W)
    disp, rgb, poses = street(a.frames, inv_K, dev)
    iK = torch.from_numpy(inv_K).to(dev)
    lo, hi = 0.5, 30.0
    state = ops.map_state(a.capacity, dev)

    def accumulate(merge=True):
        ops.map_accumulate(state, disp, rgb, poses, iK, stride=a.stride, min_depth=lo, max_depth=hi, voxel=a.voxel,
                           merge=merge)

    clear_ms, _ = timed(lambda: ops.map_clear(state), a.calls)
    plain_ms, _ = timed(lambda: accumulate(False), a.calls, before=lambda: ops.map_clear(state))
    plain_state = sorted_state(state)
    acc_ms, _ = timed(accumulate, a.calls, before=lambda: ops.map_clear(state))
    forms_agree = all(torch.equal(x, y) for x, y in zip(plain_state, sorted_state(state)))
    fin_ms, fin = timed(lambda: ops.map_finish(state, a.voxel), a.calls)
    counters = state.counters.cpu().tolist()
    voxels = int(fin[3])
    key, q, col = eager_points(disp, rgb, poses, inv_K, a.stride, lo, hi, a.voxel)
    eager_ms, fused = timed(lambda: eager_fuse(key, q, col), a.calls)
    result = {"frames": a.frames, "size": [H, W], "stride": a.stride, "voxel": a.voxel, "slots": state.T, "calls": a.calls,
              "candidates": counters[0], "kept": counters[1], "dropped_range": counters[2], "dropped_full": counters[3],
              "voxels": voxels, "clear_ms": clear_ms, "accumulate_ms": acc_ms,
              "accumulate_no_merge_ms": plain_ms, "forms_agree": forms_agree, "finish_ms": fin_ms,
              "atomic_bytes": BYTES_PER_POINT * counters[1],
              "atomic_tb_per_s_no_merge": BYTES_PER_POINT * counters[1] / (plain_ms * 1e-3) / 1e12,
              "float_atomic_tb_per_s_yardstick": FLOAT_ATOMIC_TBPS,
              "eager_unique_index_add_ms": eager_ms, "eager_points": int(key.shape[0]), "eager_voxels": int(fused[0].shape[0])}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
