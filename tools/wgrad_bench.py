#!/usr/bin/env python3
"""The ConvBlock weight gradient from the NCHW tensors against MIOpen's, on the GPU (profiles/decoder_wgrad/README.md).

    python tools/wgrad_bench.py [--repeats 20] [--batch 12] [--out profiles/decoder_wgrad/wgrad_bench.json]

For the four fine-scale shapes of the MD2 depth decoder, in one process and with the shipped MIOpen database, HIP events
around

  new      ops.conv3x3_wgrad (both launches and the scratch allocation)
  miopen   aten.convolution_backward with output mask [False, True, False] (its transposes and zero-fill included)

after 5 warm-up calls of each, `--repeats` timed calls each, alternating.  min / median / max in microseconds.  A shape
counts as FASTER - and only then belongs into ops.WGRAD_ROUTES - when the new call's slowest repeat beats MIOpen's
fastest.  Also recorded: the error of both against the float64 gradient, as a fraction of 2^-24 * sum |grad_z| |xp| (the
new call's bound is BBD_WGRAD_RUN + 1 on that measure), and whether two calls of the new one gave the same bits."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
#        layer          C   K   H    W
SHAPES = [("upconv(0,1)", 16, 16, 192, 640), ("upconv(0,0)", 32, 16, 96, 320), ("upconv(1,0)", 64, 32, 48, 160),
          ("upconv(1,1)", 96, 32, 96, 320)]


def wgrad64(xp, gz, K):
    w = torch.zeros(K, xp.shape[1], 3, 3, device=xp.device, dtype=torch.float64, requires_grad=True)
    F.conv2d(xp.double(), w, None).backward(gz.double())
    return w.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_wgrad", "wgrad_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 20, "at least 20 timed repeats"
    from baseboostdepth_amd import ops, tuning, _lib
    tuning.use_shipped_db()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    rows = []
    for layer, C, K, H, W in SHAPES:
        N = args.batch
        xp = torch.randn(N, C, H + 2, W + 2, generator=gen).to(dev)
        gz = torch.randn(N, K, H, W, generator=gen).to(dev)
        w = torch.randn(K, C, 3, 3, generator=gen).to(dev)
        calls = {
            "new": lambda: ops.conv3x3_wgrad(xp, gz),
            "miopen": lambda: torch.ops.aten.convolution_backward(gz, xp, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                                  [False, True, False])[1],
        }
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
        ref = wgrad64(xp, gz, K)
        unit = 2.0 ** -24 * wgrad64(xp.abs(), gz.abs(), K)
        first = calls["new"]()
        row = {"layer": layer, "N": N, "C": C, "K": K, "H": H, "W": W, "repeats": args.repeats,
               "same_bits": bool(torch.equal(first, calls["new"]())),
               "scratch_MB": ops.default_backend().lib.conv3x3_wgrad_scratch_doubles(N, C, K, H, W) * 8 / 1e6}
        for name, fn in calls.items():
            t = times[name]
            row[name + "_us"] = {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))}
            row[name + "_error_units"] = float(((fn().double() - ref).abs() / unit).max())
        row["faster"] = row["new_us"]["max"] < row["miopen_us"]["min"]
        row["routed"] = (C, K, H, W) in ops.WGRAD_ROUTES
        rows.append(row)
        print("%-12s new %7.1f / %7.1f / %7.1f us   miopen %7.1f / %7.1f / %7.1f us   %s%s   error (units of 2^-24 S): "
              "new %.2f of %d allowed, miopen %.2f" % (
                  layer, row["new_us"]["min"], row["new_us"]["median"], row["new_us"]["max"], row["miopen_us"]["min"],
                  row["miopen_us"]["median"], row["miopen_us"]["max"], "FASTER" if row["faster"] else "not faster",
                  ", routed" if row["routed"] else "", row["new_error_units"], _lib.WGRAD_RUN + 1,
                  row["miopen_error_units"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "wgrad_run": _lib.WGRAD_RUN, "shapes": rows}, f, indent=1)
        f.write("\n")
    bad = [r["layer"] for r in rows if r["routed"] and not (r["faster"] and r["same_bits"])]
    if bad:
        print("routed but not measured faster: %s" % ", ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
