#!/usr/bin/env python3
"""Measurements of the semi-global stereo matcher on the GPU (profiles/sgm/README.md).

    python tools/sgm_bench.py --kernel [--batch 12] [--disparities 128] [--paths 8] [--calls 10] [--out FILE.json]
        HIP events around each of `--calls` `bbd_sgm_hints` calls after 2 warm-up calls (mean, fastest, slowest) on
        buffers allocated beforehand: `--batch` pairs of 192 x 640 random byte texture, the partner shifted by 4 to 40
        pixels in eight horizontal bands, no fill - the call the trainer makes.  The time is set against the byte model
        of every launch at a copy rate MEASURED in the same process: a 512 MiB float32 tensor copied onto
        another, read + written bytes over the mean of 10 copies.  Run under `rocprofv3 --kernel-trace --stats` for the
        time of each launch.
    python tools/sgm_bench.py --step [--batch 12] [--steps 20] [--weight 0.5] [--out FILE.json]
        wall time per MD2 training step (ResNet-18, frames 0 -1 1, step graph) on one synthetic batch, with
        --depth_hints 0 and with `--weight`: the mean over `--steps` steps after the capture and 5 more steps.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 192, 640


def byte_model(B, D, paths):
    """Bytes each launch must move at the least, P = B H W pixels: {launch: bytes}."""
    P = B * H * W
    model = {"sgm_grey_kernel": 2 * P * 12 + 2 * P,             # both images' three float planes in, a byte a pixel out
             "sgm_census_kernel": 2 * P + 16 * P,                # grey in once (the 62 neighbours are cache hits), words out
             "sgm_cost_kernel": 16 * P + P * D,                  # both census rows in, a byte a disparity out
             "sgm_path_kernel (first)": P * D + 2 * P * D,       # cost in, S out
             "sgm_path_kernel (others)": (paths - 1) * (P * D + 4 * P * D),      # cost in, S in and out
             "sgm_select_kernel": 2 * P * D + 4 * P,             # S in once (the diagonal is the same lines), a word out
             "sgm_finish_kernel": 8 * P + 6 * P + 2 * P}         # two words and three sums in, a value out
    return model


def timed(fn, calls):
    ms = []
    for i in range(2 + calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(start.elapsed_time(stop))
    return ms


def copy_rate():
    a = torch.empty(128 << 20, dtype=torch.float32, device="cuda:0").normal_()
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a), 10)
    return 2 * a.numel() * 4 / (sum(ms) / len(ms) * 1e-3) / 1e9


def scene(B, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    left = torch.randint(0, 256, (B, 3, H, W + 64), generator=gen, device=dev).float() / 255
    right = torch.empty(B, 3, H, W, device=dev)
    for band in range(8):
        shift, rows = 4 + 5 * band, slice(band * H // 8, (band + 1) * H // 8)
        right[:, :, rows] = left[:, :, rows, shift:shift + W]            # matches at x - shift
    return left[..., :W].contiguous(), right


def kernel(B, D, paths, calls):
    from baseboostdepth_amd import _lib, ops
    dev = torch.device("cuda:0")
    left, right = scene(B, dev)
    side = torch.zeros(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(ops.sgm_scratch_bytes(B, H, W, D, paths), dtype=torch.uint8, device=dev)
    first, count = ops.stereo_hints(left, right, side, D, paths, scratch=scratch)
    lib, ptr = ops.default_backend().lib, _lib.ptr
    disp16, valid = torch.empty_like(first), torch.empty_like(count)
    ms = timed(lambda: lib.call("bbd_sgm_hints", ptr(left), ptr(right), ptr(side), ptr(disp16), ptr(valid), ptr(scratch),
                                scratch.numel(), B, H, W, D, paths, _lib.SGM_P1, _lib.SGM_P2, _lib.SGM_UNIQUENESS, 0,
                                lib.stream_for(left)), calls)
    rate = copy_rate()
    model = byte_model(B, D, paths)
    total = sum(model.values())
    mean = sum(ms) / len(ms)
    return {"batch": B, "size": [H, W], "disparities": D, "paths": paths, "calls": calls, "launches": 6 + paths,
            "call_ms": mean, "call_ms_min": min(ms), "call_ms_max": max(ms), "copy_GBps": rate, "model_bytes": model,
            "model_bytes_total": total, "model_ms": total / (rate * 1e9) * 1e3,
            "ratio_to_model": mean / (total / (rate * 1e9) * 1e3), "scratch_bytes": scratch.numel(),
            "density": float(count.sum()) / (B * H * W), "same_bytes_again": bool(torch.equal(disp16, first)),
            "device": torch.cuda.get_device_name(0)}


def step(B, D, steps, weight):
    from baseboostdepth_amd.synthetic import synthetic_batch
    from baseboostdepth_amd.trainer import Trainer
    out = {"batch": B, "size": [H, W], "disparities": D, "steps": steps, "device": torch.cuda.get_device_name(0)}
    batch = synthetic_batch([1] * B, H, W, [0, 1, 2, 3], device="cuda:0", seed=3)
    for name, w in (("off", 0.0), ("on", weight)):
        opt = types.SimpleNamespace(
            height=H, width=W, batch_size=B, scales=[0, 1, 2, 3], frame_ids=[0, -1, 1], min_depth=0.1, max_depth=100.0,
            disparity_smoothness=1e-3, no_ssim=False, trimin=False, decomp=False, pose_error=5.5, incremental_skip=False,
            partial_skip=False, materialize_warps=False, num_layers=18, weights_init="scratch", learning_rate=1e-4,
            no_cuda=False, cuda=0, load_weights_folder="None", log_dir="/tmp", model_name="t", step_graph=True,
            depth_hints=w, hint_disparities=D)
        torch.manual_seed(0)
        tr = Trainer(opt)
        tr.set_train()
        for _ in range(6):
            _, losses = tr.train_step(dict(batch))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            _, losses = tr.train_step(dict(batch))
        torch.cuda.synchronize()
        out["ms_per_step_" + name] = (time.perf_counter() - t0) / steps * 1e3
        out["loss_" + name] = float(losses["loss"])
        out["replays_" + name] = tr.graph_stats["replays"]
        if w > 0:
            out["weight"], out["loss_hints"], out["hint_share"] = w, float(losses["loss/hints"]), float(losses["hint_share"])
        tr._graphs.clear()
        del tr
    out["extra_ms_per_step"] = out["ms_per_step_on"] - out["ms_per_step_off"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        raise SystemExit("sgm_bench: no GPU - nothing is measured without one")
    if a.kernel == a.step:
        raise SystemExit("sgm_bench: one of --kernel and --step")
    result = kernel(a.batch, a.disparities, a.paths, a.calls) if a.kernel else step(a.batch, a.disparities, a.steps, a.weight)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
