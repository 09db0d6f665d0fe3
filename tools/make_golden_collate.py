#!/usr/bin/env python3
"""Golden vectors for the collate and validation-metric checks of tests/test_trainer_poses.py, from the live reference.

Runs ONLY where the reference tree is present: imports the reference's `Trainer.custom_collate` (trainer.py:867-886)
and `Trainer.compute_depth_losses` (trainer.py:572-617) unmodified through tools/refshim.py and runs them on the seeded
inputs the tests rebuild themselves (`make_item` items, a sparse LiDAR-like ground truth).  Output:
tests/golden/collate_metrics.npz (data only).

    python tools/make_golden_collate.py

Key encoding inside the npz file:
    collate/<i>/ms                   int  [B]  per-sample max frame offsets of case i (COLLATE_CASES)
    collate/<i>/tensors              JSON      [[key as a JSON list or string, dtype, shape, sha256 of the bytes], ...]
                                               for every tensor of the collated dict (the images alone are ~0.7 MB)
    collate/<i>/lists                JSON      the dict's non-tensor values (ordering, frames)
    metrics/names, metrics/want      the seven depth metrics of the reference on METRICS_SEED's inputs
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "collate_metrics.npz")
torch.set_num_threads(1)

COLLATE_CASES = ([3, 1, 0, 5], [0, 0], [7, 2], [1, 1, 1])
COLLATE_H, COLLATE_W, COLLATE_SCALES = 32, 64, [0, 1, 2, 3]
METRIC_NAMES = ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]
METRICS_SEED = 2


def collate_items(ms):
    """The ragged items of one collate case (seed 1, 32x64, four scales)."""
    from make_golden import make_item
    gen = torch.Generator().manual_seed(1)
    return [make_item(gen, m, COLLATE_H, COLLATE_W, COLLATE_SCALES, max(max(ms), 1), 0.3) for m in ms]


def metric_inputs():
    """(depth [1,1,192,640], sparse ground truth [375,1242]) of the metrics case."""
    gen = torch.Generator().manual_seed(METRICS_SEED)
    gt = (torch.rand(375, 1242, generator=gen) * 90).numpy()
    gt[gt < 20] = 0                                              # sparse LiDAR-like ground truth
    depth = 0.5 + 60 * torch.rand(1, 1, 192, 640, generator=gen)
    return depth, gt


def tensor_record(key, t):
    """[key, dtype, shape, sha256 of the contiguous bytes]: equal records <=> same key, dtype, shape and bits."""
    import hashlib
    return [list(key) if isinstance(key, tuple) else key, str(t.dtype), list(t.shape),
            hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()]


def collate_record(collated):
    """(sorted tensor records, non-tensor values) of a collated batch dict."""
    tensors = sorted((tensor_record(k, v) for k, v in collated.items() if torch.is_tensor(v)), key=json.dumps)
    return tensors, {k: v for k, v in collated.items() if not torch.is_tensor(v)}


def load_collate(z, i):
    """Case i of the fixture back as (ms, tensor records, non-tensor values)."""
    p = "collate/%d/" % i
    return [int(m) for m in z[p + "ms"]], json.loads(str(z[p + "tensors"])), json.loads(str(z[p + "lists"]))


def main():
    from make_golden import make_ref_trainer, make_opt as ref_opt
    rt, rl, rn = refshim.import_reference()
    rec = {}
    for i, ms in enumerate(COLLATE_CASES):
        p = "collate/%d/" % i
        ref = make_ref_trainer(rt, rl, ref_opt(COLLATE_H, COLLATE_W, len(ms), COLLATE_SCALES, True, True)).custom_collate(
            collate_items(ms))
        tensors, lists = collate_record(ref)
        rec[p + "ms"] = np.array(ms)
        rec[p + "tensors"] = np.array(json.dumps(tensors))
        rec[p + "lists"] = np.array(json.dumps(lists))
    depth, gt = metric_inputs()
    tr = rt.Trainer.__new__(rt.Trainer)
    tr.device, tr.depth_metric_names, tr.gt_depths = torch.device("cpu"), METRIC_NAMES, [gt]
    want = {}
    tr.compute_depth_losses({("depth", 0, 0): depth.clone()}, want, 0)
    rec["metrics/names"] = np.array(METRIC_NAMES)
    rec["metrics/want"] = np.array([float(want[k]) for k in METRIC_NAMES], dtype=np.float64)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KB")


if __name__ == "__main__":
    main()
