#!/usr/bin/env python3
"""The finest decoder level's up-sample + pad + 3x3 convolution in sub-pixel form against today's composition, on the GPU
(profiles/decoder_up2conv/README.md).

    python tools/up2conv_bench.py [--repeats 20] [--batch 12] [--out profiles/decoder_up2conv/up2conv_bench.json]

For DepthDecoder upconv(0,1) at 640 x 192 (z [N,16,96,320]), in one process and with the shipped MIOpen database, HIP
events around three things, each as

  new          ops.up2_conv3x3(z, bias, w)
  composition  ConvBlock.conv_raw(ops.upcat_pad_act(z, bias)): the copy, MIOpen's convolution, bbd_conv3x3_wgrad

  forward       the whole forward
  backward      the whole backward, weight gradient included (the new call re-materialises the copy for it)
  backward_data the backward without the weight gradient

after 5 warm-up calls of each, `--repeats` timed calls each, alternating.  min / median / max in microseconds.  The shape
counts as FASTER - and only then belongs into ops.UP2CONV_ROUTES - when the new call's slowest repeat beats the
composition's fastest, forward and full backward each.  Also recorded: the error of both paths against the float64
composition, forward in units of 2^-24 * S (S: the same expression on absolute values; the new call's bound is
BBD_UP2CONV_ROUNDINGS), grad_z as the largest error over the largest |gradient|, and whether two calls of the new one gave
equal bits."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [("upconv(0,1)", 16, 16, 96, 320)]       # layer, C, K, h, w


def up_pad_conv(y, w):
    return F.conv2d(F.pad(F.interpolate(y, scale_factor=2, mode="nearest"), (1, 1, 1, 1), mode="reflect"), w)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_up2conv", "up2conv_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 20, "at least 20 timed repeats"
    from baseboostdepth_amd import layers, ops, tuning, _lib
    tuning.use_shipped_db()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    rows = []
    for layer, C, K, h, w in SHAPES:
        N = args.batch
        z = (3.0 * torch.randn(N, C, h, w, generator=gen)).to(dev).requires_grad_(True)
        bias = (0.5 * torch.randn(C, generator=gen)).to(dev).requires_grad_(True)
        block = layers.ConvBlock(C, K).to(dev)
        weight = block.conv.conv.weight
        gout = torch.randn(N, K, 2 * h, 2 * w, generator=gen).to(dev)
        paths = {
            "new": lambda: ops.up2_conv3x3(z, bias, weight),
            "composition": lambda: block.conv_raw(ops.upcat_pad_act(z, bias, None)),
        }
        # the same two with a weight that asks for no gradient: their backward is the data path alone
        frozen = weight.detach()
        block_frozen = layers.ConvBlock(C, K).to(dev)
        block_frozen.conv.conv.weight = torch.nn.Parameter(frozen.clone(), requires_grad=False)
        data_paths = {
            "new": lambda: ops.up2_conv3x3(z, bias, frozen),
            "composition": lambda: block_frozen.conv_raw(ops.upcat_pad_act(z, bias, None)),
        }
        times = {(name, what): [] for name in paths for what in ("forward", "backward", "backward_data")}
        for i in range(5 + args.repeats):
            for name, fwd in paths.items():
                t_f, out = timed(fwd)
                t_b, _ = timed(lambda: torch.autograd.grad(out, (z, bias, weight), gout))
                out = data_paths[name]()
                t_d, _ = timed(lambda: torch.autograd.grad(out, (z, bias), gout))
                if i >= 5:
                    for what, t in (("forward", t_f), ("backward", t_b), ("backward_data", t_d)):
                        times[(name, what)].append(t)
        # errors against the float64 composition
        z64, b64, w64 = (t.detach().double().requires_grad_(True) for t in (z, bias, weight))
        y64 = F.elu(z64 + b64.view(1, -1, 1, 1))
        out64 = up_pad_conv(y64, w64)
        gz64, gb64, gw64 = torch.autograd.grad(out64, (z64, b64, w64), gout.double())
        unit = 2.0 ** -24 * up_pad_conv(y64.detach().abs(), w64.detach().abs())
        row = {"layer": layer, "N": N, "C": C, "K": K, "h": h, "w": w, "repeats": args.repeats,
               "rounding_bound_units": _lib.UP2CONV_ROUNDINGS}
        results = {}
        for name, fwd in paths.items():
            out = fwd()
            gz, gb, gw = torch.autograd.grad(out, (z, bias, weight), gout)
            results[name] = (out.detach(), gz, gb, gw)
            row[name + "_forward_error_units"] = float(((out.detach().double() - out64.detach()).abs() / unit).max())
            row[name + "_grad_z_error_rel"] = float((gz.double() - gz64).abs().max() / gz64.abs().max())
            row[name + "_grad_bias_error_rel"] = float((gb.double() - gb64).abs().max() / gb64.abs().max())
            row[name + "_grad_w_error_rel"] = float((gw.double() - gw64).abs().max() / gw64.abs().max())
            for what in ("forward", "backward", "backward_data"):
                t = times[(name, what)]
                row["%s_%s_us" % (name, what)] = {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))}
        out2 = paths["new"]()
        again = (out2.detach(),) + torch.autograd.grad(out2, (z, bias, weight), gout)
        row["same_bits"] = all(bool(torch.equal(a, b)) for a, b in zip(results["new"], again))
        row["weight_gradient_bits_of_composition"] = bool(torch.equal(results["new"][3], results["composition"][3]))
        row["faster"] = {what: row["new_%s_us" % what]["max"] < row["composition_%s_us" % what]["min"]
                         for what in ("forward", "backward", "backward_data")}
        row["rule_met"] = row["faster"]["forward"] and row["faster"]["backward"]
        row["routed"] = (C, K, h, w) in ops.UP2CONV_ROUTES
        rows.append(row)
        for what in ("forward", "backward", "backward_data"):
            a, b = row["new_%s_us" % what], row["composition_%s_us" % what]
            print("%-12s %-14s new %7.1f / %7.1f / %7.1f us   composition %7.1f / %7.1f / %7.1f us   %s" % (
                layer, what, a["min"], a["median"], a["max"], b["min"], b["median"], b["max"],
                "FASTER" if row["faster"][what] else "not faster"), flush=True)
        print("%-12s forward error (units of 2^-24 S): new %.2f of %d allowed, composition %.2f; grad_z error / max: new %.2e, "
              "composition %.2e; same bits %s; routed %s" % (
                  layer, row["new_forward_error_units"], _lib.UP2CONV_ROUNDINGS, row["composition_forward_error_units"],
                  row["new_grad_z_error_rel"], row["composition_grad_z_error_rel"], row["same_bits"], row["routed"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
        f.write("\n")
    bad = [r["layer"] for r in rows if r["routed"] and not (r["rule_met"] and r["same_bits"])]
    if bad:
        print("routed but not measured faster: %s" % ", ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
