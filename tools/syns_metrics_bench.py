#!/usr/bin/env python3
"""Times the SYNS-Patches metrics on the device, stage by stage, at 376x1242 (one image and a batch of 8), against
the same metrics written as eager PyTorch operations on the same GPU and, where scipy exists, against the host
restatement (numpy filters + scipy distance transforms; the all-pairs search has no host form worth waiting for).

    python tools/syns_metrics_bench.py --out profiles/syns/syns_metrics_bench.json

Times are HIP events around repeated calls after a warm-up.  Measuring without a GPU is an error, not a fallback.
The nearest-neighbour kernel is also reported as pair evaluations per second and as a share of the fp32 vector-issue
bound: 9 lane operations per pair (3 subtractions, 3 products, 2 sums, 1 minimum) against 256 CUs x 4 SIMDs x 16
lanes x 2 (packed fp32) x 2.4 GHz = 78.6e12 lane operations per second (157.3 TFLOP/s of FMA, MI355X data sheet)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_LANE_OPS = 256 * 4 * 16 * 2 * 2.4e9
OPS_PER_PAIR = 9
GH, GW, H, W = 376, 1242, 192, 640


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


# ---------------------------------------------------------------------------- eager PyTorch forms of the same metrics
def eager_edges(depth_at_gt):
    import torch.nn.functional as F
    L = (depth_at_gt > 0) * torch.log(depth_at_gt.clamp(min=1.1920928955078125e-07))
    k = torch.exp(-torch.tensor([-1.0, 0.0, 1.0], device=L.device) ** 2 / 2)
    k = (k / k.sum()).float()
    x = L[None, None]
    x = F.conv2d(F.pad(x, (1, 1, 0, 0), mode="reflect"), k.view(1, 1, 1, 3))
    x = F.conv2d(F.pad(x, (0, 0, 1, 1), mode="reflect"), k.view(1, 1, 3, 1)).double()
    sm = torch.tensor([1.0, 4, 6, 4, 1], device=L.device, dtype=torch.float64)
    dv = torch.tensor([-1.0, -2, 0, 2, 1], device=L.device, dtype=torch.float64)
    p = F.pad(x, (2, 2, 2, 2), mode="reflect")
    dx = F.conv2d(F.conv2d(p, dv.view(1, 1, 1, 5)), sm.view(1, 1, 5, 1))
    dy = F.conv2d(F.conv2d(p, sm.view(1, 1, 1, 5)), dv.view(1, 1, 5, 1))
    mag = torch.sqrt(dx * dx + dy * dy)[0, 0]
    return mag > mag.mean()


def eager_edt_sq(mask, rows_per_chunk=8):
    """The same two passes with tensor operations: nearest set row above / below by running maxima, then a chunked
    [rows, x, x'] minimum."""
    Hh, Ww = mask.shape
    ys = torch.arange(Hh, device=mask.device)[:, None].expand(Hh, Ww)
    big = 1 << 15
    up = torch.cummax(torch.where(mask, ys, torch.full_like(ys, -big)), 0).values
    dn = -torch.cummax(torch.where(mask, -ys, torch.full_like(ys, -big)).flip(0), 0).values.flip(0)
    g = torch.minimum(ys - up, dn - ys).clamp(max=big)
    g2 = torch.where(g >= big, torch.full_like(g, 1 << 30), g * g)
    xs = torch.arange(Ww, device=mask.device)
    off = (xs[:, None] - xs[None, :]) ** 2
    out = torch.empty_like(g2)
    for r in range(0, Hh, rows_per_chunk):
        out[r:r + rows_per_chunk] = (off[None] + g2[r:r + rows_per_chunk, None, :]).min(2).values
    return out


def eager_nn(q, t, chunk=256):
    out = torch.empty(q.shape[0], device=q.device)
    for s in range(0, q.shape[0], chunk):
        d = q[s:s + chunk, None, :] - t[None, :, :]
        out[s:s + chunk] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1).values
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syns", "syns_metrics_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eager_nn_queries", type=int, default=8192,
                    help="queries of the eager all-pairs search (all targets); its full time is extrapolated from them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("syns_metrics_bench: no GPU - nothing is measured without one")
    import syns_checks as C
    import syns_ref
    from baseboostdepth_amd import evaluation as E, ops
    dev = torch.device("cuda:0")
    inv_K = syns_ref.syns_camera()[1]
    result = {"device": torch.cuda.get_device_name(0), "gt_size": [GH, GW], "pred_size": [H, W], "reps": args.reps,
              "peak_lane_ops_per_s": PEAK_LANE_OPS, "lane_ops_per_pair": OPS_PER_PAIR, "batches": {}}
    for n in (1, 8):
        gt = [C.make_gt(200 + i, GH, GW, density=0.7) for i in range(n)]
        gts = E.GroundTruthSet([g[0] for g in gt], dev, crop=False, edges=[g[1] for g in gt])
        disp = torch.from_numpy(np.stack([1.0 / C.make_depth(300 + i, H, W) for i in range(n)])).float().to(dev)
        idx = list(range(n))
        rows = E.depth_metrics(disp, gts, idx, max_depth=125.0, pred_is_disp=True, median="numpy")
        edge, _ = E.pred_edges(disp, gts, idx, pred_is_disp=True)
        _, _, stride = E.syns_strides(gts)
        valid = [(g[0] > 1e-3) & (g[0] < 125.0) for g in gt]
        tgt = torch.zeros(n, stride, dtype=torch.uint8, device=dev)
        for i in range(n):
            tgt[i, :GH * GW] = torch.from_numpy((valid[i] & gt[i][1][..., 0]).reshape(-1).astype(np.uint8)).to(dev)
        r = {}
        r["depth_metrics_ms"] = timed(lambda: E.depth_metrics(disp, gts, idx, max_depth=125.0, pred_is_disp=True, median="numpy"), args.reps)
        r["edges_ms"] = timed(lambda: E.pred_edges(disp, gts, idx, pred_is_disp=True), args.reps)
        r["edt_target_ms"] = timed(lambda: E.distance_transform(tgt, gts, idx), args.reps)
        r["edt_pred_ms"] = timed(lambda: E.distance_transform(edge, gts, idx), args.reps)
        r["edge_metrics_call_ms"] = timed(lambda: E.edge_metrics(disp, gts, idx, edge, rows, pred_is_disp=True), args.reps)
        r["reduction_ms_by_difference"] = r["edge_metrics_call_ms"] - r["edt_target_ms"] - r["edt_pred_ms"]
        r["pointcloud_call_ms"] = timed(lambda: E.pointcloud_metrics(disp, gts, idx, rows, inv_K, pred_is_disp=True), max(2, args.reps // 2), 1)
        counts = [int(v.sum()) for v in valid]
        pairs = float(sum(c * c for c in counts))
        r["points_per_cloud"] = counts
        # the two directions are the same kernel on swapped arguments and equal sizes: one direction = half the call
        pc = E.pointcloud_metrics(disp, gts, idx, rows, inv_K, pred_is_disp=True)
        a = torch.rand(counts[0], 3, device=dev) * 50
        b = a + 0.05 * torch.randn_like(a)
        nn_ms = timed(lambda: ops.chamfer_nn(a, b), max(2, args.reps // 2), 1) / 2
        if n == 1:
            r["nn_per_direction_ms"] = nn_ms
            r["nn_pairs_per_direction"] = float(counts[0]) ** 2
            r["nn_pairs_per_s"] = r["nn_pairs_per_direction"] / (nn_ms * 1e-3)
            r["nn_share_of_vector_issue_bound"] = r["nn_pairs_per_s"] * OPS_PER_PAIR / PEAK_LANE_OPS
        r["pointcloud_pairs_both_directions"] = 2 * pairs
        r["pointcloud_pairs_per_s"] = 2 * pairs / (r["pointcloud_call_ms"] * 1e-3)
        r["pointcloud_share_of_vector_issue_bound"] = r["pointcloud_pairs_per_s"] * OPS_PER_PAIR / PEAK_LANE_OPS
        r["syns_metrics_total_ms"] = timed(lambda: E.syns_metrics(disp, gts, idx, inv_K=inv_K, chamfer=True), 2, 1)
        r["syns_metrics_no_chamfer_ms"] = timed(lambda: E.syns_metrics(disp, gts, idx), args.reps)
        r["f1_iou_image0"] = [float(pc[0, 0]), float(pc[0, 1])]
        if n == 1:
            # ---- eager PyTorch on the same GPU, same image
            import torch.nn.functional as F
            at_gt = 1.0 / F.interpolate(disp[:, None], (GH, GW), mode="bilinear", align_corners=False)[0, 0]
            e_edge = eager_edges(at_gt)
            t_mask = tgt[0, :GH * GW].view(GH, GW).bool()
            eg = {"edges_ms": timed(lambda: eager_edges(at_gt), args.reps),
                  "edt_target_ms": timed(lambda: eager_edt_sq(t_mask), 2, 1),
                  "edt_pred_ms": timed(lambda: eager_edt_sq(e_edge), 2, 1)}
            same = torch.equal(eager_edt_sq(t_mask).int(), E.image_view(E.distance_transform(tgt, gts, idx), gts, 0, 0))
            eg["edt_equals_kernel"] = bool(same)
            q = a[:args.eager_nn_queries]
            ms = timed(lambda: eager_nn(q, b), 2, 1)
            eg["nn_queries_timed"] = int(q.shape[0])
            eg["nn_pairs_per_s"] = float(q.shape[0]) * counts[0] / (ms * 1e-3)
            eg["nn_per_direction_ms_extrapolated"] = r["nn_pairs_per_direction"] / eg["nn_pairs_per_s"] * 1e3
            eg["nn_equals_kernel"] = bool(torch.equal(eager_nn(q, b), ops.chamfer_nn(a, b)[0][:q.shape[0]]))
            r["eager_pytorch"] = eg
            # ---- host restatement (numpy filters + scipy transforms), one image
            try:
                from scipy import ndimage
                at = at_gt.cpu().numpy()
                t0 = time.perf_counter()
                he = syns_ref.pred_edges(at)[0]
                t1 = time.perf_counter()
                ndimage.distance_transform_edt(1 - t_mask.cpu().numpy())
                ndimage.distance_transform_edt(1 - he)
                t2 = time.perf_counter()
                r["host"] = {"edges_ms": (t1 - t0) * 1e3, "two_distance_transforms_ms": (t2 - t1) * 1e3,
                             "nearest_neighbour": "not measured"}
            except ImportError:
                r["host"] = "not measured"
        result["batches"][str(n)] = r
        print(json.dumps({str(n): r}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
