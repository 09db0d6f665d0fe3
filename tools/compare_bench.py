#!/usr/bin/env python3
"""Measurements of the checkpoint comparison sheets on the GPU (profiles/compare/README.md).

    python tools/compare_bench.py [--frames 200] [--runs 2] [--out profiles/compare/compare_bench.json]
        wall time of `compare.run_cli` (the body of validation.py, `--error_maps`) on a synthetic KITTI-shaped tree:
        `--frames` JPEGs of 192 x 640 (a window sliding over one picture), sparse ground truth (5 %) at that size, two
        random-weight ResNet-18 checkpoints with feed size 192 x 640; first call (kernel selection included) and the next
    rocprofv3 --kernel-trace --stats -d <dir> -o compare --output-format csv -- python tools/compare_bench.py --runs 1
        the same, once: the kernel times of bbd_gt_viz and bbd_error_map are in the trace
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W = 192, 640
FOLDER = "2011_09_26/2011_09_26_drive_0001_sync"


def write_tree(tmp, frames):
    from PIL import Image
    rng = np.random.default_rng(0)
    kt, split = os.path.join(tmp, "kitti"), os.path.join(tmp, "split")
    d = os.path.join(kt, FOLDER, "image_02", "data")
    os.makedirs(d)
    os.makedirs(split)
    base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 40, 3)).astype(np.uint8)
    big = np.asarray(Image.fromarray(base).resize((W + 8 * 39, H), Image.BILINEAR))
    data = np.empty(frames, dtype=object)
    with open(os.path.join(split, "val_files.txt"), "w") as f:
        for t in range(frames):                                   # a window sliding over one picture: cheap, distinct frames
            shift = (t * 7) % (8 * 39)
            Image.fromarray(big[:, shift:shift + W]).save(os.path.join(d, "%010d.jpg" % t), quality=90)
            f.write("%s %d l\n" % (FOLDER, t))
            gt = (3.0 + 70.0 * rng.random((H, W))).astype(np.float32)
            gt[rng.random((H, W)) >= 0.05] = 0.0
            data[t] = gt
    np.savez(os.path.join(split, "gt_depths.npz"), data=data)
    return kt, split


def write_models(tmp, names):
    from baseboostdepth_amd import networks
    root = os.path.join(tmp, "models")
    for k, name in enumerate(names):
        torch.manual_seed(k)
        encoder = networks.ResnetEncoder(18, False)
        decoder = networks.DepthDecoder(encoder.num_ch_enc)
        os.makedirs(os.path.join(root, name))
        state = encoder.state_dict()
        state["height"], state["width"] = H, W
        torch.save(state, os.path.join(root, name, "encoder.pth"))
        torch.save(decoder.state_dict(), os.path.join(root, name, "depth.pth"))
    return root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from baseboostdepth_amd import compare
    names = ["first", "second"]
    result = {"frames": a.frames, "models": len(names), "height": H, "width": W, "wall_s": []}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        kt, split = write_tree(tmp, a.frames)
        models = write_models(tmp, names)
        result["setup_s"] = time.perf_counter() - t0
        for run in range(a.runs):
            argv = ["--model_name"] + names + ["--models_dir", models, "--kt_path", kt, "--split_dir", split, "--output",
                                               os.path.join(tmp, "out%d" % run), "--error_maps"]
            t0 = time.perf_counter()
            abs_rel, _ = compare.run_cli(compare.parse_args(argv))
            torch.cuda.synchronize()
            result["wall_s"].append(time.perf_counter() - t0)
            print("run %d: %.3f s" % (run, result["wall_s"][-1]), flush=True)
        result["abs_rel_mean"] = abs_rel.mean(0).tolist()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
