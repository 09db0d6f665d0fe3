#!/usr/bin/env python3
"""Measurements of the point-cloud export on the GPU (profiles/cloud/README.md).

    python tools/cloud_bench.py [--images 16] [--stride 1] [--calls 50] [--out profiles/cloud/cloud_bench.json]
        time per `ops.point_cloud` call (HIP events around `--calls` calls after 5 warm-up calls) for `--images` images of
        375 x 1242 from a 192 x 640 disparity, in two forms: "image" - every pixel kept, coloured by the image, what
        `predict_cloud` asks for - and "masked" - BBD_CLOUD_MASK_GT | BBD_CLOUD_CLAMP with metrics rows and ground truth
        of which half is valid, coloured by inverse depth, what `--save_clouds` asks for; and the bytes each form moves
        by the model of DESIGN.md 6i
    rocprofv3 --kernel-trace --stats -d <dir> -o cloud --output-format csv -- python tools/cloud_bench.py --calls 20
        the same under the tracer: the kernel times of cloud_count_kernel, cloud_scan_kernel and cloud_write_kernel
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GH, GW, H, W = 375, 1242, 192, 640
COPY_GBPS = 6076.0          # what a float4 copy reaches on this part


def model_bytes(n, candidates, kept, rgb, gt):
    """16 B per kept vertex, 3 B of colour per kept vertex, 4 B of ground truth per candidate and pass,
    the chunk table (4 B per 256 candidates, written and read twice), the prediction once per pass."""
    chunks = -(-candidates // 256)
    return 16 * kept + (3 * kept if rgb else 0) + (8 * candidates if gt else 0) + 16 * chunks + 2 * 4 * n * H * W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from baseboostdepth_amd import _lib, ops, pointcloud
    if not torch.cuda.is_available():
        raise SystemExit("cloud_bench: no GPU - nothing is measured without one")
    dev, n = torch.device("cuda:0"), a.images
    g = torch.Generator().manual_seed(0)
    disp = (1.0 / (2.0 + 70.0 * torch.rand(n, H, W, generator=g))).to(dev)
    gt = 2.0 + 70.0 * torch.rand(n * GH * GW, generator=g)
    gt[torch.rand(n * GH * GW, generator=g) < 0.5] = 0.0
    gt = gt.to(dev)
    rgb = torch.randint(0, 256, (n * GH * GW * 3,), dtype=torch.uint8, generator=g).to(dev)
    rows = torch.zeros(n, _lib.EVAL_OUT)
    rows[:, 7] = 1.0 + 0.01 * torch.arange(n)
    rows = rows.to(dev)
    desc = ops.cloud_rows([(GH, GW)] * n)
    inv_K = pointcloud.intrinsics(GH, GW)
    forms = {
        "image": dict(rgb=rgb, min_depth=0.0, max_depth=1e6, pred_is_disp=True),
        "masked": dict(gt=gt, rows=rows, min_depth=1e-3, max_depth=80.0, pred_is_disp=True, mask_gt=True, clamp_depth=True),
    }
    result = {"images": n, "gt_size": [GH, GW], "pred_size": [H, W], "stride": a.stride, "calls": a.calls, "forms": {}}
    for name, kw in forms.items():
        for _ in range(5):
            out = ops.point_cloud(disp, desc, inv_K, stride=a.stride, **kw)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            out = ops.point_cloud(disp, desc, inv_K, stride=a.stride, **kw)
        stop.record()
        torch.cuda.synchronize()
        kept = int(out[1].sum())
        candidates = sum(ops.cloud_capacity(r, a.stride) for r in desc)
        nbytes = model_bytes(n, candidates, kept, "rgb" in kw, "gt" in kw)
        result["forms"][name] = {"us_per_call": 1e3 * start.elapsed_time(stop) / a.calls, "candidates": candidates,
                                 "kept": kept, "model_bytes": nbytes, "model_us_at_copy_rate": nbytes / COPY_GBPS / 1e3}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
