#!/usr/bin/env python3
"""Times the Velodyne depth maps: one `bbd_velo_depth` call for 1 frame and for 32 frames (device events, points already
resident), `kitti_utils.generate_depth_maps` end to end from .bin files (threads, upload, launch, one synchronise),
and a numpy restatement of the same four reductions on this host's CPU.  Prints one JSON line.  A record, not a gate.

    python tools/velo_bench.py [--points 120000] [--frames 32] [--iters 50] [--out FILE]

Scans are synthetic full-circle 64-beam sweeps (about half the points lie behind the camera, as in KITTI) on the
calibration texts of the test fixture.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import velo_checks as vc  # noqa: E402
from baseboostdepth_amd import kitti_utils, ops  # noqa: E402


def full_scan(rng, n):
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rng.integers(0, 64, n) * (26.8 / 63) - 24.8)
    r = np.minimum(1.73 / np.maximum(np.sin(-el), 1e-3), rng.uniform(4, 80, n))
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.random(n)],
                    1).astype(np.float32)


def numpy_depth_map(P, scan, h, w, vel_depth):
    """The four order-independent reductions of bbd_velo.hip with numpy ufuncs (ufunc.at), float64 as the reference."""
    p = scan[scan[:, 0] >= 0].astype(np.float64)
    q = p[:, 0:1] * P[None, :, 0] + p[:, 1:2] * P[None, :, 1] + p[:, 2:3] * P[None, :, 2] + P[None, :, 3]
    with np.errstate(all="ignore"):
        u, v = np.round(q[:, 0] / q[:, 2]) - 1, np.round(q[:, 1] / q[:, 2]) - 1
    z = p[:, 0] if vel_depth else q[:, 2]
    ok = (u >= 0) & (v >= 0) & (u < w) & (v < h)
    u, v, z = u[ok].astype(np.int64), v[ok].astype(np.int64), z[ok]
    order = np.arange(len(z))
    pixel, key = v * w + u, v * (w - 1) + u
    last = np.full(h * w, -1)
    np.maximum.at(last, pixel, order)
    first = np.full(h * w, len(z))
    np.minimum.at(first, key, order)
    count = np.zeros(h * w, np.int64)
    np.add.at(count, key, 1)
    least = np.full(h * w, np.inf)
    np.minimum.at(least, key, z)
    depth = np.zeros(h * w)
    hit = last >= 0
    depth[hit] = z[last[hit]]
    dup = np.flatnonzero(count > 1)
    depth[pixel[first[dup]]] = least[dup]
    depth[depth < 0] = 0
    return depth.reshape(h, w).astype(np.float32)


def device_ms(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "velo_bench.py times the MI355X kernel; there is no CPU path"
    dev = torch.device("cuda:0")
    v = vc.load()
    rng = np.random.default_rng(0)
    dates = ["2011_09_26", "2011_09_30"]
    res = {"points_per_frame": a.points, "frames": a.frames}
    with tempfile.TemporaryDirectory() as tmp:
        scans = [full_scan(rng, a.points) for _ in range(a.frames)]
        lines = vc.write_tree(v, tmp, [(dates[i % 2], i, s) for i, s in enumerate(scans)])
        split_dir = vc.write_split(tmp, "eigen", lines)
        frames = kitti_utils.split_frames(split_dir, "eigen", tmp)
        geo = [kitti_utils.velo_projection(f[0], 2) for f in frames]
        # numpy on this CPU, and agreement with the device on the benchmark's own scans
        t0 = time.perf_counter()
        host_maps = [numpy_depth_map(geo[i][0], scans[i], *geo[i][1], True) for i in range(min(4, a.frames))]
        res["numpy_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / len(host_maps)
        for n in (1, a.frames):
            pts = torch.from_numpy(np.concatenate(scans[:n])).to(dev)
            P = np.stack([g[0] for g in geo[:n]])
            shapes = [g[1] for g in geo[:n]]
            out, offs = ops.velo_depth(pts, [a.points] * n, P, shapes, vel_depth=True)
            got = out.cpu().numpy()
            for i in range(min(n, len(host_maps))):
                h, w = shapes[i]
                assert np.array_equal(got[offs[i]:offs[i] + h * w].reshape(h, w), host_maps[i]), "device != numpy restatement"
            ms = device_ms(lambda: ops.velo_depth(pts, [a.points] * n, P, shapes, out=out, offsets=offs, vel_depth=True), a.iters)
            res["launch_%d_frames_ms" % n] = ms
            res["launch_%d_frames_ms_per_frame" % n] = ms / n
        kitti_utils.generate_depth_maps(frames, dev, vel_depth=True)          # page cache, pinned pool, code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gts = kitti_utils.generate_depth_maps(frames, dev, vel_depth=True)
        torch.cuda.synchronize()
        res["from_files_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / a.frames
        res["nonzero_pixels_per_frame"] = int((gts.buffer != 0).sum()) // a.frames
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
