#!/usr/bin/env python3
"""Measurements of the uncertainty kernels on the GPU (profiles/uncert/README.md).

    python tools/uncert_bench.py [--calls 20] [--out profiles/uncert/uncert_bench.json]

HIP events around each of `--calls` calls after 2 warm-up calls (the mean, and the range), on buffers allocated
beforehand, for

  realistic   `bbd_sparsification`, 16 predictions of 192 x 640 against 16 maps of 375 x 1242 with about 4 % valid pixels
              inside the Garg window, 50 intervals
  dense       the same with every pixel of the 16 whole maps valid (no crop window): the sort's extreme
  flip        `bbd_post_process_uncert` next to `bbd_post_process_disp`, 16 x 192 x 640

each set against its byte model at the 6 076 GB/s float4 copy rate of DESIGN.md 3.  The launches' own times come from a
`rocprofv3 --kernel-trace --stats` run of this script (a run of its own).  Identical calls must give identical bytes:
the last output of every workload is compared with the first."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, W, GH, GW, K = 16, 192, 640, 375, 1242, 50
COPY_GBPS = 6076.0


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


def sparsification_model(window_pixels, valid):
    """Bytes the algorithm needs: the prediction and uncertainty planes once, the windows' ground truth twice (count,
    terms), per ordering and digit pass one read and one write of 8 bytes per valid pixel (and one more read of the key
    for the histogram), the terms written once and gathered through the sorted slots (12 B + 4 B, four orderings)."""
    planes = 2 * N * H * W * 4
    windows = 2 * window_pixels * 4
    sort = 4 * 4 * valid * (8 + 8 + 4)
    terms = valid * (12 + 4 * 8)
    gather = 4 * valid * (4 + 12)
    return dict(planes=planes, windows=windows, sort=sort, terms=terms, gather=gather,
                total=planes + windows + sort + terms + gather)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurements need the MI355X"
    from baseboostdepth_amd import evaluation, ops
    from baseboostdepth_amd._lib import ptr, SPARS_SUMMARY
    dev = "cuda:0"
    backend = ops.default_backend()
    g = torch.Generator().manual_seed(3)
    depth = 3.0 + 70.0 * torch.rand(N, GH, GW, generator=g)
    pred = (1.0 / (2.0 * (3.0 + 70.0 * torch.rand(N, H, W, generator=g)))).to(dev)
    uncert = torch.rand(N, H, W, generator=g).to(dev)
    result = dict(n=N, h=H, w=W, gh=GH, gw=GW, intervals=K, calls=args.calls, copy_gbps=COPY_GBPS)
    for name, crop, share in (("realistic", True, 0.04), ("dense", False, 2.0)):
        keep = torch.rand(N, GH, GW, generator=g) < share
        gts = evaluation.GroundTruthSet([(depth[i] * keep[i]).numpy() for i in range(N)], dev, crop=crop)
        idx = list(range(N))
        rows = evaluation.depth_metrics(pred, gts, idx, pred_is_disp=True, median="numpy")
        nbytes = ops.sparsification_scratch_bytes(gts.desc_host, N)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        out = torch.empty(N, SPARS_SUMMARY + 6 * (K + 1), dtype=torch.float64, device=dev)

        def call():
            backend.run("bbd_sparsification", pred, ptr(pred), ptr(uncert), ptr(gts.buffer), ptr(gts.desc), ptr(rows),
                        ptr(out), ptr(scratch), nbytes, N, H, W, K, 1e-3, 80.0, 1.0, 0)

        call()
        first = out.clone()
        mean, lo, hi = timed(call, args.calls)
        valid = int(out[:, 6].sum().item())
        d = gts.desc_host.astype(np.int64)
        window_pixels = int(((d[:, 5] - d[:, 4]) * (d[:, 7] - d[:, 6])).sum())
        model = sparsification_model(window_pixels, valid)
        wrapper = timed(lambda: ops.sparsification(pred, uncert, gts, idx, rows, intervals=K), args.calls)[0]
        result[name] = dict(valid=valid, window_pixels=window_pixels, scratch_bytes=nbytes, ms=mean, ms_min=lo, ms_max=hi,
                            wrapper_ms=wrapper, model_bytes=model, model_ms=model["total"] / COPY_GBPS / 1e6,
                            identical=bool(torch.equal(out.view(torch.int64), first.view(torch.int64))),
                            ause=out[:, :3].mean(0).tolist(), aurg=out[:, 3:6].mean(0).tolist())
        print(name, json.dumps(result[name]))
    disp = torch.rand(2 * N, H, W, generator=g).to(dev)
    blended, both, u = (torch.empty(N, H, W, device=dev) for _ in range(3))
    plain = timed(lambda: backend.run("bbd_post_process_disp", disp, ptr(disp), ptr(blended), N, H, W), args.calls)
    with_u = timed(lambda: backend.run("bbd_post_process_uncert", disp, ptr(disp), ptr(both), ptr(u), N, H, W), args.calls)
    plane = N * H * W * 4
    result["flip"] = dict(post_process_disp_ms=plain[0], post_process_uncert_ms=with_u[0], disp_range=plain[1:],
                          uncert_range=with_u[1:], disp_model_ms=3 * plane / COPY_GBPS / 1e6,
                          uncert_model_ms=4 * plane / COPY_GBPS / 1e6, same_blend=bool(torch.equal(blended, both)))
    print("flip", json.dumps(result["flip"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
