#!/usr/bin/env python3
"""Timing of the prediction tail ("Colour-mapped disparity"): HIP events, warm-up, median of >= 50
repetitions.

    python tools/viz_bench.py [--reps 60] [--e2e 64]

(i)   ops.disp_viz for 1 and for 12 images, 192x640 -> 375x1242;
(ii)  the same tail the way the reference does it on this machine: F.interpolate on the GPU, .cpu(), np.percentile,
      the LUT in numpy (wall clock per image, it is host work);
(iii) test_simple.py's body end to end on a folder of synthetic 375x1242 PNGs with randomly initialised ResNet-18
      weights: images per second, and the share of host decode and save (summed thread time over the pool).
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from baseboostdepth_amd import inference, ops  # noqa: E402

H, W, H0, W0 = 192, 640, 375, 1242


def event_median_ms(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def reference_tail(disp, lut):
    d = torch.nn.functional.interpolate(disp, (H0, W0), mode="bilinear", align_corners=False)
    s = (1 / 80.0 + (1 / 0.1 - 1 / 80.0) * d).squeeze().cpu().numpy()
    vmin, vmax = s.min(), np.percentile(s, 95)
    x = (s - vmin) / (vmax - vmin)
    return lut[np.clip((x * np.float32(256)).astype(np.int64), 0, 255)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--e2e", type=int, default=64)
    a = ap.parse_args()
    dev = "cuda:0"
    out = {}
    g = torch.Generator().manual_seed(0)
    for n in (1, 12):
        disp = torch.rand(n, 1, H, W, generator=g).to(dev)
        sizes = [(H0, W0)] * n
        out["disp_viz_ms_n%d" % n] = event_median_ms(lambda: ops.disp_viz(disp, sizes), a.reps)
        out["disp_viz_float_ms_n%d" % n] = event_median_ms(lambda: ops.disp_viz(disp, sizes, want_float=True), a.reps)
    lut = ops.magma_lut("cpu").numpy()
    disp1 = torch.rand(1, 1, H, W, generator=g).to(dev)
    wall = []
    for k in range(10 + a.reps):
        t = time.perf_counter()
        reference_tail(disp1, lut)
        if k >= 10:
            wall.append((time.perf_counter() - t) * 1e3)
    out["reference_tail_ms_per_image"] = statistics.median(wall)

    if a.e2e:
        from PIL import Image
        from baseboostdepth_amd import networks
        spent = {"load": 0.0, "save": 0.0}
        real_load, real_save = inference._load, inference._save

        def timed(name, fn):
            def run(*args):
                t = time.perf_counter()
                r = fn(*args)
                spent[name] += time.perf_counter() - t          # float add under the GIL: good enough for a share
                return r
            return run
        inference._load, inference._save = timed("load", real_load), timed("save", real_save)
        with tempfile.TemporaryDirectory() as tmp:
            rng = np.random.default_rng(0)
            for k in range(a.e2e):
                Image.fromarray(rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)).save(os.path.join(tmp, "%03d.png" % k))
            torch.manual_seed(0)
            enc = networks.ResnetEncoder(18, False)
            pred = inference.DepthPredictor(enc, networks.DepthDecoder(enc.num_ch_enc), H, W, dev)
            args = inference.parse_args(["--image_path", tmp, "--save_path", os.path.join(tmp, "o"), "--ext", "png",
                                         "--weights", "unused"])
            inference.run_cli(args, predictor=pred)                 # warm-up: kernel selection, allocator
            spent["load"] = spent["save"] = 0.0
            t = time.perf_counter()
            inference.run_cli(args, predictor=pred)
            wall_s = time.perf_counter() - t
        out["e2e_images_per_s"] = a.e2e / wall_s
        out["e2e_wall_s"] = wall_s
        out["e2e_decode_thread_s"], out["e2e_save_thread_s"] = spent["load"], spent["save"]
        out["e2e_host_threads"] = inference.HOST_THREADS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
