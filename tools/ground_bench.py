#!/usr/bin/env python3
"""Measurements of the ground-plane scale recovery on the GPU (profiles/ground/README.md).

    python tools/ground_bench.py [--calls 20] [--out profiles/ground/ground_bench.json]

HIP events around each of `--calls` `ops.ground_scale` calls after 2 warm-up calls (the mean), for n = 16 and n = 1
disparity maps of 192 x 640: a synthetic road under a camera 1.65 m up, pitched by a degree or two, cut by a wall at
20 m, with 0.2 % depth noise, each at a scale of its own.  A call is the wrapper's allocations and the two launches; the
kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (a run of its own, no counters).

Each time is set against the byte model of DESIGN.md 6l at the 6 076 GB/s float4 copy rate of DESIGN.md 3: the heights
launch reads 4 B and writes 4 B per pixel (+1 B with the mask), the select launch sweeps the 4 B per pixel of the
scratch map three times, from L2.
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

H, W = 192, 640
COPY_GBPS = 6076.0


def road(inv_K, pitch_deg, scale, seed, height=1.65, wall=20.0):
    """float32 [H,W] disparity of the plane (0, cos p, sin p) . P = height seen through inv_K, cut at z = wall."""
    iK = np.asarray(inv_K, np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ry = iK[1, 0] * u + iK[1, 1] * v + iK[1, 2]
    p = np.deg2rad(pitch_deg)
    along = np.cos(p) * ry + np.sin(p)
    depth = np.minimum(np.where(along > 1e-9, height / np.maximum(along, 1e-9), np.inf), wall) / scale
    depth = depth * (1.0 + 0.002 * np.random.default_rng(seed).standard_normal((H, W)))
    return (1.0 / depth).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import map_bench
    from baseboostdepth_amd import ops, pointcloud
    if not torch.cuda.is_available():
        raise SystemExit("ground_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    inv_K = pointcloud.intrinsics(H, W)
    scales = [1.0 + 0.45 * i for i in range(16)]
    disp = torch.from_numpy(np.stack([road(inv_K, (-3.0, 0.0, 2.0)[i % 3], s, i) for i, s in enumerate(scales)])).to(dev)
    iK = torch.from_numpy(inv_K).to(dev)
    result = {"size": [H, W], "calls": a.calls, "copy_GBps": COPY_GBPS}
    for n in (16, 1):
        for mask in (False, True):
            ms, (rows, _) = map_bench.timed(lambda: ops.ground_scale(disp[:n], iK, pred_is_disp=True, want_mask=mask),
                                            a.calls)
            rows = rows.cpu().numpy()
            error = float(np.abs(rows[:, 7] / np.array(scales[:n]) - 1.0).max())
            heights_bytes, select_bytes = n * H * W * (8 + int(mask)), 3 * 4 * n * H * W
            model = (heights_bytes + select_bytes) / (COPY_GBPS * 1e9) * 1e3
            result["n%d%s" % (n, "_mask" if mask else "")] = {
                "ms": ms, "heights_bytes": heights_bytes, "select_bytes": select_bytes, "model_ms": model,
                "ratio_to_model": ms / model, "ground_share": float((rows[:, 1] / rows[:, 2]).mean()),
                "max_scale_error": error}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
