#!/usr/bin/env python3
"""Measurement of the affine-invariant depth evaluation on the GPU (profiles/align/README.md).

    python tools/align_bench.py [--calls 20] [--out profiles/align/align_bench.json]

HIP events around each of `--calls` calls after 2 warm-up calls (the mean, and the range), on buffers allocated
beforehand: `bbd_depth_metrics_affine` and, in the same process on the same inputs, `bbd_depth_metrics` - 16
predictions of 192 x 640 against 16 maps of 375 x 1242 with about 4 % valid pixels inside the Garg window, the
configuration of tools/uncert_bench.py.  A device-to-device copy of 256 MiB is timed in the same run; the byte model -
three sweeps, each reading the windowed map and the taps of the prediction - is priced at that rate.  Identical calls
must give identical bytes: the last output is compared with the first."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, W, GH, GW = 16, 192, 640, 375, 1242


def timed(fn, calls):
    """(mean, min, max) milliseconds of `fn` over `calls` calls after 2 warm-up calls (HIP events)."""
    times = []
    for i in range(2 + calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        if i >= 2:
            times.append(start.elapsed_time(stop))
    return float(np.mean(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    from baseboostdepth_amd import evaluation, ops
    from baseboostdepth_amd._lib import ALIGN_OUT, EVAL_OUT, EVAL_PRED_IS_DISP, EVAL_MEDIAN_MIDPOINT, ptr
    dev = "cuda:0"
    backend = ops.default_backend()
    g = torch.Generator().manual_seed(3)
    depth = 3.0 + 70.0 * torch.rand(N, GH, GW, generator=g)
    pred = (1.0 / (2.0 * (3.0 + 70.0 * torch.rand(N, H, W, generator=g)))).to(dev)
    keep = torch.rand(N, GH, GW, generator=g) < 0.04
    gts = evaluation.GroundTruthSet([(depth[i] * keep[i]).numpy() for i in range(N)], dev, crop=True)
    out = torch.empty(N, ALIGN_OUT, dtype=torch.float64, device=dev)
    rows = torch.empty(N, EVAL_OUT, dtype=torch.float32, device=dev)

    def affine():
        backend.run("bbd_depth_metrics_affine", pred, ptr(pred), ptr(gts.buffer), ptr(gts.desc), ptr(out), N, H, W, 1e-3,
                    80.0, 0)

    def median():
        backend.run("bbd_depth_metrics", pred, ptr(pred), ptr(gts.buffer), ptr(gts.desc), ptr(rows), N, H, W, 1e-3, 80.0,
                    1e-3, 80.0, 1.0, EVAL_PRED_IS_DISP | EVAL_MEDIAN_MIDPOINT)

    affine()
    first = out.clone()
    t_affine, t_median = timed(affine, args.calls), timed(median, args.calls)
    src = torch.empty(1 << 26, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.calls)
    copy_gbps = 2 * src.numel() * 4 / t_copy[0] / 1e6
    d = gts.desc_host.astype(np.int64)
    window_pixels = int(((d[:, 5] - d[:, 4]) * (d[:, 7] - d[:, 6])).sum())
    valid = int(out[:, 10].sum().item())
    # per sweep: the window's ground truth (4 B a pixel) and the prediction plane once (its taps are shared by neighbours)
    model_bytes = 3 * (window_pixels * 4 + N * H * W * 4)
    result = dict(n=N, h=H, w=W, gh=GH, gw=GW, calls=args.calls, valid=valid, window_pixels=window_pixels,
                  affine_ms=t_affine[0], affine_range=t_affine[1:], depth_metrics_ms=t_median[0],
                  depth_metrics_range=t_median[1:], copy_gbps=copy_gbps, model_bytes=model_bytes,
                  model_ms=model_bytes / copy_gbps / 1e6, identical=bool(torch.equal(out.view(torch.int64),
                                                                                     first.view(torch.int64))),
                  counts_agree=bool(torch.equal(out[:, 10].float(), rows[:, 10])))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
