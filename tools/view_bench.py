#!/usr/bin/env python3
"""Measurements of the view rasteriser on the GPU (profiles/view/README.md).

    python tools/view_bench.py [--calls 5] [--out profiles/view/view_bench.json]

HIP events around each of `--calls` calls after 2 warm-up calls (the mean); the canvas, 1024 x 1024, is cleared before
every timed call, outside the timed span.

    map      `ops.view_points` on the finished voxels of the workload of tools/map_bench.py (200 frames of 192 x 640 at
             stride 2 through a synthetic street: about 162 k voxels in a table of 2^24 slots, so the launch spans 2^24
             records of which the device-side count admits the first 162 k), top view fitted to the drive, sizes 1 and 3
    cloud    `ops.view_points` on the clouds of 16 images of 375 x 1242 (7.45 M vertices, `ops.point_cloud` of the same
             street), seen by a camera of the same field of view turned 15 degrees about the median depth, sizes 1 and 3
    lines    `ops.view_lines` on a winding trajectory of 4541 poses (the length of KITTI odometry sequence 00), width 2
    clear, resolve

Each time is set against a byte model at the copy rate `benchmodes.stream_copy_ceiling` measures in the same process:
16 B per vertex read, and 8 B per touched cell in each direction (size^2 cells per drawn point; for lines the painted
cells); clear writes and resolve reads 8 B per cell, resolve writes 3 B per pixel.  The model counts every offer as a
read and a write of its cell: it is a floor for the traffic of atomics that all go through, and says nothing of how
atomics on one address queue up.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZE = 1024
CLOUD_H, CLOUD_W, CLOUD_N = 375, 1242, 16
POSES = 4541


def street_depth(h, w, inv_K):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    iK = torch.as_tensor(inv_K, dtype=torch.float64)
    rx = iK[0, 0] * xx + iK[0, 1] * yy + iK[0, 2]
    ry = iK[1, 0] * xx + iK[1, 1] * yy + iK[1, 2]
    road = torch.where(ry > 1e-6, 1.65 / ry.clamp_min(1e-6), torch.full_like(ry, 1e3))
    return torch.minimum(road, 6.0 / rx.abs().clamp_min(1e-6)).clamp(max=80.0)


def winding(n):
    """World positions of a drive of 0.8 m per frame whose heading swings slowly: loops and crossings, as sequence 00."""
    t = np.arange(n, dtype=np.float64)
    heading = 2.5 * np.sin(t / 310.0) + 1.5 * np.sin(t / 97.0)
    xyz = np.zeros((n, 3))
    xyz[:, 0], xyz[:, 2] = np.cumsum(0.8 * np.sin(heading)), np.cumsum(0.8 * np.cos(heading))
    return xyz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import map_bench
    from baseboostdepth_amd import benchmodes, ops, pointcloud
    if not torch.cuda.is_available():
        raise SystemExit("view_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    copy = benchmodes.stream_copy_ceiling(dev)
    rate = copy["GBps"] * 1e9
    state = ops.view_state(SIZE, SIZE, dev)
    clear = lambda: ops.view_clear(state)                                   # noqa: E731
    result = {"canvas": [SIZE, SIZE], "calls": a.calls, "stream_copy_GBps": copy["GBps"]}

    def measure(name, fn, vertices, painted_per_drawn):
        ms, _ = map_bench.timed(fn, a.calls, before=clear)
        offered, drawn, clipped, rejected = state.counters.cpu().tolist()
        covered = int((state.cells != -1).sum())
        model = (16 * vertices + 16 * painted_per_drawn * drawn) / rate * 1e3
        result[name] = {"ms": ms, "vertices": vertices, "drawn": drawn, "clipped": clipped, "covered_cells": covered,
                        "model_ms": model, "ratio_to_model": ms / model}

    # ---- the map of tools/map_bench.py
    inv_K = pointcloud.intrinsics(map_bench.H, map_bench.W)
    disp, rgb, poses = map_bench.street(200, inv_K, dev)
    table = ops.map_state(1 << 24, dev)
    ops.map_accumulate(table, disp, rgb, poses, torch.from_numpy(inv_K).to(dev), stride=2, min_depth=0.5, max_depth=30.0,
                       voxel=0.2)
    _, voxels, _, m = ops.map_finish(table, 0.2)
    n_vox = int(m)
    view, mpp = pointcloud.ortho_view((-8.0, -3.0, 0.0), (8.0, 2.0, 230.0), SIZE, SIZE, plane="top", near=-4.0)
    view_dev = torch.from_numpy(view).to(dev)
    for size in (1, 3):
        measure("map_size%d" % size, lambda: ops.view_points(state, voxels, view_dev, count=m, size=size), n_vox, size * size)
    result["map_m_per_px"] = mpp
    del disp, rgb, table

    # ---- 16 clouds of 375 x 1242
    inv_K = pointcloud.intrinsics(CLOUD_H, CLOUD_W)
    depth = street_depth(CLOUD_H, CLOUD_W, inv_K).float()
    g = torch.Generator().manual_seed(0)
    pred = (depth[None] * (1.0 + 0.01 * torch.rand(CLOUD_N, CLOUD_H, CLOUD_W, generator=g))).to(dev)
    colours = torch.randint(0, 256, (CLOUD_N * CLOUD_H * CLOUD_W * 3,), generator=g, dtype=torch.uint8).to(dev)
    cloud, counts, _ = ops.point_cloud(pred, ops.cloud_rows([(CLOUD_H, CLOUD_W)] * CLOUD_N), inv_K, rgb=colours,
                                       min_depth=0.0, max_depth=80.0)
    assert int(counts.sum()) == CLOUD_N * CLOUD_H * CLOUD_W
    K = pointcloud.camera_matrix(SIZE, SIZE)
    z = cloud.view(torch.float32).view(-1, 4)[:, 2]
    orbit = torch.from_numpy(pointcloud.orbit_view(K, 15.0, -10.0, float(z.median()))).to(dev)
    for size in (1, 3):
        measure("cloud_size%d" % size, lambda: ops.view_points(state, cloud, orbit, size=size),
                CLOUD_N * CLOUD_H * CLOUD_W, size * size)

    # ---- a trajectory of 4541 poses
    xyz = winding(POSES)
    tview, tmpp = pointcloud.ortho_view(xyz.min(0), xyz.max(0), SIZE, SIZE, plane="top")
    xyz_dev, tview_dev = torch.from_numpy(xyz).to(dev), torch.from_numpy(tview).to(dev)
    ms, _ = map_bench.timed(lambda: ops.view_lines(state, xyz_dev, tview_dev, width=2.0, layer=1), a.calls, before=clear)
    painted = int((state.cells != -1).sum())
    model = (24 * POSES + 16 * painted) / rate * 1e3
    result["lines"] = {"ms": ms, "poses": POSES, "painted_cells": painted, "m_per_px": tmpp, "model_ms": model,
                       "ratio_to_model": ms / model}

    # ---- clear and resolve
    ms, _ = map_bench.timed(clear, a.calls)
    result["clear"] = {"ms": ms, "model_ms": 8 * SIZE * SIZE / rate * 1e3}
    ms, _ = map_bench.timed(lambda: ops.view_resolve(state), a.calls)
    result["resolve"] = {"ms": ms, "model_ms": 11 * SIZE * SIZE / rate * 1e3}
    for k in ("clear", "resolve"):
        result[k]["ratio_to_model"] = result[k]["ms"] / result[k]["model_ms"]
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
