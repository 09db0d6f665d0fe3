#!/usr/bin/env python3
"""The ResNet shortcut convolution (1x1, stride 2, no bias) in its three directions on fp32 MFMA against MIOpen's, and the
joint backward of a down-sampling block's entry against the separate form, on the GPU (profiles/conv1x1/README.md).

    python tools/conv1x1_bench.py [--repeats 20] [--out profiles/conv1x1/conv1x1_bench.json]

For the six shortcuts of an MD2 step - layer2 (64 -> 128, 48 x 160), layer3 (128 -> 256, 24 x 80), layer4 (256 -> 512,
12 x 40), each at N = 12 (depth encoder) and N = 24 (pose encoder) - in one process and with the shipped MIOpen database,
HIP events around the WHOLE call of each side (allocations, transposes and zero-fills included):

  fwd    new  ops.conv1x1s2_fwd                          miopen  F.conv2d(x, w, None, 2)
  dgrad  new  ops.conv1x1s2_bwd_data (plain mode)        miopen  aten.convolution_backward, mask [True, False, False]
  wgrad  new  ops.conv1x1s2_wgrad (both launches and     miopen  aten.convolution_backward, mask [False, True, False]
              the scratch allocation)
  joint  new  conv_backward(g3, x, w3) of the block's    miopen  the same conv_backward, the shortcut's data gradient from
              3x3 stride-2 conv1, then                           MIOpen and the ATen add of the two
              ops.conv1x1s2_bwd_data in accumulate mode  plain   ... with ops.conv1x1s2_bwd_data in plain mode + the add
              on its grad_x

after 5 warm-up calls of each, `--repeats` timed calls each, alternating.  min / median / max in microseconds.  A direction
of a shape counts as FASTER when the new call's slowest repeat beats MIOpen's fastest; a row (C, K, H, W, direction)
belongs into ops.CONV1X1_ROUTES only when that holds at N = 12 AND at N = 24.  Also recorded: both floors of the new call
(byte_model below at 4.6 TB/s, FLOPs at 157 TFLOP/s), the error of both sides against float64 as a fraction of
2^-24 * sum |a| |b| (the new calls' bounds: C + 1, K + 1, BBD_WGRAD_RUN + 1), and whether two new calls gave equal bits."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYERS = [("layer2", 64, 128, 48, 160), ("layer3", 128, 256, 24, 80), ("layer4", 256, 512, 12, 40)]
BATCHES = [12, 24]
MFMA_FLOPS, STREAM_BYTES = 157e12, 4.6e12


def byte_model(direction, N, C, K, H, W):
    """Bytes a direction has to move: the even rows of x (whole rows: half of every sector is unused either way), y or
    grad_y, all of grad_x where it is written, the weight; the weight gradient's float64 records are extra and listed."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    even_rows, y, w = 4 * N * C * Ho * W, 4 * N * K * Ho * Wo, 4 * K * C
    return {"fwd": even_rows + y + w, "dgrad": y + w + 4 * N * C * H * W, "wgrad": even_rows + y + w,
            "joint": y + w + 2 * 4 * N * C * Ho * Wo}[direction]


def _backward(gy, x, w, stride, pad, mask):
    return torch.ops.aten.convolution_backward(gy, x, w, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1, mask)


def _timed(calls, repeats):
    times = {name: [] for name in calls}
    for i in range(5 + repeats):
        for name, fn in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            if i >= 5:
                times[name].append(1e3 * start.elapsed_time(stop))
    return {name: {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1x1", "conv1x1_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 20, "at least 20 timed repeats"
    from baseboostdepth_amd import ops, tuning, _lib
    tuning.use_shipped_db()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    rows = []
    for layer, C, K, H, W in LAYERS:
        for N in BATCHES:
            Ho, Wo = H // 2, W // 2
            x = torch.randn(N, C, H, W, generator=gen).to(dev)
            w = (0.1 * torch.randn(K, C, 1, 1, generator=gen)).to(dev)
            gy = torch.randn(N, K, Ho, Wo, generator=gen).to(dev)
            w3 = (0.1 * torch.randn(K, C, 3, 3, generator=gen)).to(dev)
            g3 = torch.randn(N, K, Ho, Wo, generator=gen).to(dev)
            flops = 2.0 * N * K * Ho * Wo * C

            def joint_new():
                gx, gw3, _ = _backward(g3, x, w3, 2, 1, [True, True, False])
                return ops.conv1x1s2_bwd_data(gy, w, x.shape, into=gx)

            def joint_plain():
                gx, gw3, _ = _backward(g3, x, w3, 2, 1, [True, True, False])
                return gx + ops.conv1x1s2_bwd_data(gy, w, x.shape)

            def joint_miopen():
                gx, gw3, _ = _backward(g3, x, w3, 2, 1, [True, True, False])
                return gx + _backward(gy, x, w, 2, 0, [True, False, False])[0]

            directions = {
                "fwd": {"new": lambda: ops.conv1x1s2_fwd(x, w), "miopen": lambda: F.conv2d(x, w, None, 2)},
                "dgrad": {"new": lambda: ops.conv1x1s2_bwd_data(gy, w, x.shape),
                          "miopen": lambda: _backward(gy, x, w, 2, 0, [True, False, False])[0]},
                "wgrad": {"new": lambda: ops.conv1x1s2_wgrad(x, w, gy),
                          "miopen": lambda: _backward(gy, x, w, 2, 0, [False, True, False])[1]},
                "joint": {"new": joint_new, "plain": joint_plain, "miopen": joint_miopen},
            }
            x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
            y64 = F.conv2d(x64, w64, None, 2)
            y64.backward(gy.double())
            xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
            ya = F.conv2d(xa, wa, None, 2)
            ya.backward(gy.double().abs())
            ref = {"fwd": y64.detach(), "dgrad": x64.grad, "wgrad": w64.grad}
            unit = {"fwd": 2.0 ** -24 * ya.detach(), "dgrad": 2.0 ** -24 * xa.grad, "wgrad": 2.0 ** -24 * wa.grad}
            for direction, calls in directions.items():
                row = {"layer": layer, "direction": direction, "N": N, "C": C, "K": K, "H": H, "W": W, "repeats": args.repeats}
                for name, t in _timed(calls, args.repeats).items():
                    row[name + "_us"] = t
                first = calls["new"]()
                row["same_bits"] = bool(torch.equal(first, calls["new"]()))
                del first
                nbytes = byte_model(direction, N, C, K, H, W)
                row["floors"] = {"mfma_us": 1e6 * flops / MFMA_FLOPS, "bytes_us": 1e6 * nbytes / STREAM_BYTES, "bytes": nbytes}
                if direction == "wgrad":
                    row["record_bytes"] = 8 * ops.default_backend().lib.conv1x1s2_wgrad_scratch_doubles(N, C, K, H, W)
                if direction in ref:
                    for name, fn in calls.items():
                        err = (fn().double() - ref[direction]).abs() / unit[direction].clamp_min(1e-300)
                        row[name + "_error_units"] = float(err[unit[direction] > 0].max())
                floor = max(row["floors"]["mfma_us"], row["floors"]["bytes_us"])
                row["bound_by"] = "bytes" if row["floors"]["bytes_us"] >= row["floors"]["mfma_us"] else "mfma"
                row["new_over_floor"] = row["new_us"]["median"] / floor
                row["faster"] = row["new_us"]["max"] < row["miopen_us"]["min"]
                row["routed"] = (C, K, H, W, direction) in ops.CONV1X1_ROUTES
                rows.append(row)
                print("%-6s %-5s N %2d  new %6.1f / %6.1f / %6.1f us   miopen %6.1f / %6.1f / %6.1f us%s   %s%s   %.2f x its %s floor "
                      "(%.1f us)%s%s" % (
                          layer, direction, N, row["new_us"]["min"], row["new_us"]["median"], row["new_us"]["max"],
                          row["miopen_us"]["min"], row["miopen_us"]["median"], row["miopen_us"]["max"],
                          "   plain %6.1f / %6.1f / %6.1f us" % tuple(row["plain_us"][k] for k in ("min", "median", "max"))
                          if "plain_us" in row else "",
                          "FASTER" if row["faster"] else "not faster", ", routed" if row["routed"] else "",
                          row["new_over_floor"], row["bound_by"], floor,
                          "   error (units of 2^-24 S): new %.2f, miopen %.2f" % (row["new_error_units"], row["miopen_error_units"])
                          if direction in ref else "", "" if row["same_bits"] else "   BITS DIFFER"), flush=True)
            del x, w, gy, w3, g3, ref, unit, x64, w64, xa, wa, y64, ya
            torch.cuda.empty_cache()
    # a row of the table: a direction that is FASTER at both batches (`joint`: a row of ops.BLOCK_ENTRY_ROUTES)
    passing = sorted((C, K, H, W, d) for _, C, K, H, W in LAYERS for d in ("fwd", "dgrad", "wgrad", "joint")
                     if all(r["faster"] and r["same_bits"] for r in rows if (r["C"], r["direction"]) == (C, d)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "wgrad_run": _lib.WGRAD_RUN, "passing_rows": passing, "rows": rows},
                  f, indent=1)
        f.write("\n")
    print("rows that pass at N = 12 and N = 24: %s" % (passing,))
    bad = sorted(row for row in ops.CONV1X1_ROUTES if tuple(row) not in set(passing))
    if bad:
        print("routed but not measured faster: %s" % (bad,))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
