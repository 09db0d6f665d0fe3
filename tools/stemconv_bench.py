#!/usr/bin/env python3
"""The encoder stems' conv1 (7x7, stride 2, pad 3, C -> 64) and its weight gradient on fp32 MFMA against MIOpen's, on the
GPU (profiles/stem_conv/README.md).

    python tools/stemconv_bench.py [--repeats 20] [--out profiles/stem_conv/stemconv_bench.json]

For the depth stem (C = 3, N = 12), the pose stem (C = 6, N = 24) and, for information, the pooled step's pose pass
(C = 6, N = 236), all at 192 x 640, in one process and with the shipped MIOpen database, HIP events around

  fwd    new     ops.stem_conv_fwd                       miopen  F.conv2d(x, w, None, 2, 3)
  wgrad  new     ops.stem_conv_wgrad (both launches      miopen  aten.convolution_backward with output mask
                 and the scratch allocation)                     [False, True, False] (transposes and zero-fill included)

after 5 warm-up calls of each, `--repeats` timed calls each, alternating.  min / median / max in microseconds.  A direction
of a shape counts as FASTER - and only then belongs into ops.STEMCONV_ROUTES - when the new call's slowest repeat beats
MIOpen's fastest.  Also recorded: the ratio of the new call's median to both floors (FLOPs at 157 TFLOP/s; bytes of x, w
and out / grad_out at 4.6 TB/s), the error of both sides against float64 as a fraction of 2^-24 * sum |a| |b| (the new
calls' bounds: P + 1 = 149 / 297 forward, BBD_WGRAD_RUN + 1 for the gradient), and whether two new calls gave equal bits."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
#         stem               C   N   H    W    may be routed
SHAPES = [("depth conv1", 3, 12, 192, 640, True), ("pose conv1", 6, 24, 192, 640, True),
          ("pose conv1, pooled", 6, 236, 192, 640, False)]
MFMA_FLOPS, STREAM_BYTES = 157e12, 4.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_conv", "stemconv_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 20, "at least 20 timed repeats"
    from baseboostdepth_amd import ops, tuning, _lib
    tuning.use_shipped_db()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    rows = []
    for stem, C, N, H, W, routable in SHAPES:
        x = torch.rand(N, C, H, W, generator=gen).to(dev)
        w = (0.1 * torch.randn(64, C, 7, 7, generator=gen)).to(dev)
        go = torch.randn(N, 64, H // 2, W // 2, generator=gen).to(dev)
        flops = 2.0 * N * 64 * (H // 2) * (W // 2) * C * 49
        nbytes = 4.0 * (x.numel() + w.numel() + go.numel())
        floors = {"mfma_us": 1e6 * flops / MFMA_FLOPS, "bytes_us": 1e6 * nbytes / STREAM_BYTES}
        directions = {
            "fwd": {"new": lambda: ops.stem_conv_fwd(x, w), "miopen": lambda: F.conv2d(x, w, None, 2, 3)},
            "wgrad": {"new": lambda: ops.stem_conv_wgrad(x, w, go),
                      "miopen": lambda: torch.ops.aten.convolution_backward(go, x, w, None, [2, 2], [3, 3], [1, 1], False,
                                                                            [0, 0], 1, [False, True, False])[1]},
        }
        w64 = w.double().requires_grad_(True)
        out64 = F.conv2d(x.double(), w64, None, 2, 3)
        out64.backward(go.double())
        a64 = torch.zeros_like(w64).requires_grad_(True)
        F.conv2d(x.double().abs(), a64, None, 2, 3).backward(go.double().abs())
        ref = {"fwd": out64.detach(), "wgrad": w64.grad}
        unit = {"fwd": 2.0 ** -24 * F.conv2d(x.double().abs(), w.double().abs(), None, 2, 3), "wgrad": 2.0 ** -24 * a64.grad}
        del out64
        for direction, calls in directions.items():
            times = {name: [] for name in calls}
            for i in range(5 + args.repeats):
                for name, fn in calls.items():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    fn()
                    stop.record()
                    torch.cuda.synchronize()
                    if i >= 5:
                        times[name].append(1e3 * start.elapsed_time(stop))
            first = calls["new"]()
            row = {"stem": stem, "direction": direction, "N": N, "C": C, "H": H, "W": W, "repeats": args.repeats,
                   "same_bits": bool(torch.equal(first, calls["new"]())), "floors": floors}
            del first
            for name, fn in calls.items():
                t = times[name]
                row[name + "_us"] = {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))}
                row[name + "_error_units"] = float(((fn().double() - ref[direction]).abs() / unit[direction].clamp_min(1e-300)).max())
            row["new_over_mfma_floor"] = row["new_us"]["median"] / floors["mfma_us"]
            row["new_over_bytes_floor"] = row["new_us"]["median"] / floors["bytes_us"]
            row["faster"] = row["new_us"]["max"] < row["miopen_us"]["min"]
            row["routed"] = (C, H, W, direction) in ops.STEMCONV_ROUTES
            row["for_information"] = not routable
            rows.append(row)
            print("%-20s %-5s N %3d  new %7.1f / %7.1f / %7.1f us   miopen %7.1f / %7.1f / %7.1f us   %s%s   %.2f x MFMA floor, "
                  "%.2f x byte floor   error (units of 2^-24 S): new %.2f, miopen %.2f%s" % (
                      stem, direction, N, row["new_us"]["min"], row["new_us"]["median"], row["new_us"]["max"],
                      row["miopen_us"]["min"], row["miopen_us"]["median"], row["miopen_us"]["max"],
                      "FASTER" if row["faster"] else "not faster", ", routed" if row["routed"] else "",
                      row["new_over_mfma_floor"], row["new_over_bytes_floor"], row["new_error_units"], row["miopen_error_units"],
                      "" if row["same_bits"] else "   BITS DIFFER"), flush=True)
        del x, w, go, ref, unit
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "wgrad_run": _lib.WGRAD_RUN, "rows": rows}, f, indent=1)
        f.write("\n")
    bad = ["%s %s" % (r["stem"], r["direction"]) for r in rows
           if r["routed"] and not r["for_information"] and not (r["faster"] and r["same_bits"])]
    if bad:
        print("routed but not measured faster: %s" % ", ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
