#!/usr/bin/env python3
"""Writes tests/golden/syns_cases.npz: what the float64 numpy reference (tests/syns_ref.py) gives on the seeded inputs
of tests/syns_checks.py.  Inputs are NOT stored (they are regenerated from their seeds); edge maps and rounding bands
are stored as bits.  Asserts, on the reference alone, the two conditions the tests rely on: at most 1e-3 of an image
lies within delta of the edge threshold, and a float32 blur (a second rounding order) flips no pixel outside that band.

    python tools/make_golden_syns.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import syns_checks as C  # noqa: E402
import syns_ref  # noqa: E402


def main():
    out = {}
    inv_K = syns_ref.syns_camera()[1]
    for name in C.CASES:
        depth, gt, gt_edge = C.case_inputs(name)
        for mode in ("evaluate", "trainer"):
            pred = (1.0 / depth if mode == "evaluate" else depth).astype(np.float32)
            at_gt = C.resized(pred, *gt.shape, mode)
            edge, mag, mean, delta = syns_ref.pred_edges(at_gt)
            band = np.abs(mag - mean) <= delta
            edge32 = syns_ref.pred_edges(at_gt, np.float32)[0]
            flips = int(((edge32 != edge) & ~band).sum())
            print("%-10s %-8s delta %.3e band share %.3e float32-blur flips outside the band %d (inside %d)"
                  % (name, mode, delta, band.mean(), flips, int(((edge32 != edge) & band).sum())))
            assert band.mean() <= C.BAND_SHARE_CAP, (name, mode, band.mean())
            assert flips == 0, (name, mode, flips)
            lo, hi = C.depth_range(mode)
            m = syns_ref.edge_metrics(edge, gt, gt_edge, lo, hi)
            p, ratio = C.scaled(at_gt, gt, mode)
            key = name if mode == "evaluate" else name + "/trainer"
            out[key + "/edge_bits"] = C.pack_bits(edge)
            out[key + "/band_bits"] = C.pack_bits(band)
            out[key + "/metrics"] = np.array([m["edge_Acc"], m["edge_comp"], syns_ref.err(p, gt, lo, hi), m["n_near"],
                                              m["n_tgt"], m["n_valid"], m["n_edge"], float(ratio)], np.float64)
        if name != "full":                   # (the full-size clouds are 3e5 points: checked on a subset by the GPU tier)
            p, _ = C.scaled(C.resized((1.0 / depth).astype(np.float32), *gt.shape, "evaluate"), gt, "evaluate")
            for rays in ("reference", "pixel"):
                f, iou, P, R, nn_p, nn_t = syns_ref.pointcloud_metrics(p, gt, inv_K, *C.depth_range("evaluate"), rays)
                out[name + "/cloud_" + rays] = np.array([f, iou, P, R, len(nn_p)], np.float32)
                print("%-10s cloud %-9s f %.6f iou %.6f P %.6f R %.6f N %d" % (name, rays, f, iou, P, R, len(nn_p)))
    rng = np.random.default_rng(77)
    a = (rng.standard_normal((3000, 3)) * 4).astype(np.float32)
    b = (rng.standard_normal((2500, 3)) * 4).astype(np.float32)
    out["nn/seed"] = np.array([77, 3000, 2500])
    out["nn/a"] = syns_ref.nn_sq(a, b)
    out["nn/b"] = syns_ref.nn_sq(b, a)
    mask = np.random.default_rng(78).random((90, 140)) < 0.004
    out["edt/seed"] = np.array([78, 90, 140])
    out["edt/sq"] = syns_ref.edt_sq(mask).astype(np.int32)
    np.savez_compressed(C.GOLDEN, **out)
    print("wrote %s: %d bytes" % (C.GOLDEN, os.path.getsize(C.GOLDEN)))


if __name__ == "__main__":
    main()
