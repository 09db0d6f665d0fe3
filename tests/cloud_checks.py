"""The checks of the point-cloud export, written once and run by both tiers: tests/test_cloud_port.py through the host
port on the CPU, tests/test_gpu_cloud.py through the kernels.  Every check takes (backend, device).

Everything is compared bit for bit - the whole vertex buffer including the bytes nothing may write, and the counts -
against tests/cloud_ref.py: kernel, port and reference perform the same float32 operations without contraction, so
there is no tolerance anywhere in this file.

A case is a dict: `pred` float32 [n,h,w]; `shapes` [(GH, GW)]; optional `gts` (list of float32 maps), `windows`,
`ratios` (column 7 of the rows), `rgbs` (list of uint8 [GH,GW,3]), `inv_K` ([3,3] or [n,3,3]; default: a camera per
image) and `kw`, the keyword arguments of `ops.point_cloud` that the reference takes as well."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import cloud_ref  # noqa: E402
import syns_ref  # noqa: E402
from baseboostdepth_amd import _lib, evaluation, ops  # noqa: E402

FILL = 0xA5
GUARD, GAP = 7, 5            # vertices before the first region / after the last one, and between two regions
V = _lib.CLOUD_VERTEX


def lut():
    return ops.magma_lut("cpu").numpy()


def camera(i, gh, gw):
    """A pinhole camera per image, float32 [3,3] inverse: focal lengths and centre vary with i so that a mixed-up
    inv_K row shows."""
    K = np.array([[0.58 * gw + i, 0, 0.5 * gw - i], [0, 1.92 * gh - i, 0.5 * gh + i], [0, 0, 1]], dtype=np.float32)
    return np.linalg.pinv(K).astype(np.float32)


def depth_like(rng, h, w, lo=2.0, hi=50.0):
    return (lo + (hi - lo) * rng.random((h, w))).astype(np.float32)


def colours(rng, shapes):
    return [rng.integers(0, 256, (gh, gw, 3), dtype=np.uint8) for gh, gw in shapes]


def inv_Ks(case):
    if "inv_K" in case:
        iK = np.asarray(case["inv_K"], np.float32)
        return np.broadcast_to(iK[..., :3, :3], (len(case["shapes"]), 3, 3)) if iK.ndim == 2 else iK[:, :3, :3]
    return np.stack([camera(i, gh, gw) for i, (gh, gw) in enumerate(case["shapes"])])


def layout(case, guard=GUARD, gap=GAP):
    """(region starts, capacities, vertices of the buffer): a guard band, the regions with gaps between them, a guard."""
    stride = case.get("kw", {}).get("stride", 1)
    rows = ops.cloud_rows(case["shapes"], windows=case.get("windows"))
    caps = [ops.cloud_capacity(r, stride) for r in rows]
    regions, at = [], guard
    for c in caps:
        regions.append(at)
        at += c + gap
    return regions, caps, at - gap + guard


def run_case(backend, dev, case, guard=GUARD, gap=GAP):
    """`ops.point_cloud` on a buffer pre-filled with 0xA5.  Returns (buffer bytes, counts, regions, caps) on the host."""
    n = len(case["shapes"])
    regions, caps, total = layout(case, guard, gap)
    out = torch.full((total * V,), FILL, dtype=torch.uint8, device=dev)
    gt = rgb = rows = None
    if case.get("gts") is not None:
        gt = torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in case["gts"]])).to(dev)
    if case.get("rgbs") is not None:
        rgb = torch.from_numpy(np.concatenate([np.asarray(c, np.uint8).reshape(-1) for c in case["rgbs"]])).to(dev)
    if case.get("ratios") is not None:
        r = np.zeros((n, _lib.EVAL_OUT), np.float32)
        r[:, 7] = case["ratios"]
        rows = torch.from_numpy(r).to(dev)
    pred = torch.from_numpy(np.asarray(case["pred"], np.float32)).to(dev)
    vertices, counts, offsets = ops.point_cloud(pred, ops.cloud_rows(case["shapes"], windows=case.get("windows")),
                                                inv_Ks(case), gt=gt, rows=rows, rgb=rgb, out=out, regions=regions,
                                                backend=backend, **case.get("kw", {}))
    assert vertices is out and list(offsets) == regions and counts.dtype == torch.int32
    return out.cpu().numpy(), counts.cpu().numpy(), regions, caps


def expected(case, regions, total_bytes):
    """The same buffer from the reference.  Returns (bytes, counts, raw depths per image)."""
    buf = np.full(total_bytes, FILL, np.uint8)
    counts, raws = [], []
    iK = inv_Ks(case)
    for i, shape in enumerate(case["shapes"]):
        v, raw = cloud_ref.cloud(case["pred"][i], shape, iK[i], lut(),
                                 gt=None if case.get("gts") is None else case["gts"][i],
                                 window=None if case.get("windows") is None else case["windows"][i],
                                 ratio=None if case.get("ratios") is None else case["ratios"][i],
                                 rgb=None if case.get("rgbs") is None else case["rgbs"][i], **case.get("kw", {}))
        buf[regions[i] * V:(regions[i] + len(v)) * V] = v.view(np.uint8)
        counts.append(len(v))
        raws.append(raw)
    return buf, np.array(counts, np.int32), raws


def check_case(backend, dev, case, what=""):
    """Counts equal, every byte equal - vertices and everything that must still hold 0xA5.  Returns (counts, caps,
    raw depths)."""
    got, counts, regions, caps = run_case(backend, dev, case)
    want, want_counts, raws = expected(case, regions, got.size)
    print("%s: capacities %s, counts %s (reference %s)" % (what, caps, counts.tolist(), want_counts.tolist()))
    assert np.array_equal(counts, want_counts), what
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "%s: %d bytes differ, the first at byte %d (vertex %d)" % (what, diff.size, diff[0], diff[0] // V)
    return counts, caps, raws


# ------------------------------------------------------------------------------------------------ 1. ragged batch
RAGGED_SHAPES = [(5, 7), (37, 91), (64, 130)]


def check_ragged(backend, dev):
    rng = np.random.default_rng(11)
    depth = np.stack([depth_like(rng, 8, 16) for _ in RAGGED_SHAPES])
    rgbs = colours(rng, RAGGED_SHAPES)
    for disp in (False, True):
        for ratios in (None, [1.25, 0.8, 1.0625]):
            for use_rgb in (False, True):
                for rays in ("pixel", "reference"):
                    case = dict(pred=1.0 / depth if disp else depth, shapes=RAGGED_SHAPES, ratios=ratios,
                                rgbs=rgbs if use_rgb else None,
                                kw=dict(pred_is_disp=disp, rays=rays, min_depth=1e-3, max_depth=125.0 if disp else 80.0))
                    counts, caps, _ = check_case(backend, dev, case, "ragged disp=%s rows=%s rgb=%s rays=%s"
                                                 % (disp, ratios is not None, use_rgb, rays))
                    assert counts.tolist() == caps == [gh * gw for gh, gw in RAGGED_SHAPES]      # all pixels are kept


# ------------------------------------------------------------------------------------------------ 2. wave / chunk edges
def _pattern_case(shapes, period, from_gt):
    """Images whose keep pattern has the given period over the flat pixel index: the first half of every period is
    kept.  Prediction and ground truth have the images' own sizes (every image its own prediction slot size is not
    possible in one batch, so the pattern lives in the ground truth, or - one image - in the prediction)."""
    rng = np.random.default_rng(100 + period)
    gts = []
    for gh, gw in shapes:
        g = depth_like(rng, gh, gw)
        k = np.arange(gh * gw).reshape(gh, gw)
        g[(k % period) >= (period + 1) // 2] = 0.5            # finite, below min_depth = 1
        gts.append(g)
    if from_gt:
        pred = np.ones((len(shapes), 2, 2), np.float32)
        return dict(pred=pred, shapes=shapes, gts=gts, kw=dict(from_gt=True, min_depth=1.0, max_depth=80.0))
    assert len(shapes) == 1       # same size: the resampled prediction is the prediction (weights 1 and 0, finite values)
    return dict(pred=np.stack(gts), shapes=shapes, kw=dict(min_depth=1.0, max_depth=80.0))


def check_wave_and_chunk_edges(backend, dev):
    small = [(1, 63), (1, 64), (1, 65), (1, 127), (3, 43)]
    for period in (1, 2, 3):
        counts, caps, _ = check_case(backend, dev, _pattern_case(small, period, True), "wave edges, period %d" % period)
        assert (period > 1) == (counts.tolist() != caps)
    for period in (3, 64):                    # 257 * 259 = 66 563 candidates: 261 chunks, more totals than a wave holds
        for from_gt in (True, False):
            counts, caps, _ = check_case(backend, dev, _pattern_case([(257, 259)], period, from_gt),
                                         "257x259, period %d, from_gt=%s" % (period, from_gt))
            assert caps == [257 * 259] and 0 < counts[0] < caps[0]


# ------------------------------------------------------------------------------------------------ 3. degenerate keeps
def check_degenerate(backend, dev):
    rng = np.random.default_rng(5)
    shapes = [(9, 20), (7, 33), (6, 11), (10, 13), (8, 70)]
    gts = [depth_like(rng, gh, gw) for gh, gw in shapes]
    gts[1][:] = 0.0                                     # nothing kept, in the middle of the batch
    keep_first = gts[2].copy()
    gts[2][:] = 0.0
    gts[2][0, 0] = keep_first[0, 0]                     # only the first pixel
    keep_last = gts[3].copy()
    gts[3][:] = 0.0
    gts[3][-1, -1] = keep_last[-1, -1]                  # only the last pixel; images 0 and 4 keep everything
    case = dict(pred=np.ones((5, 2, 2), np.float32), shapes=shapes, gts=gts,
                kw=dict(from_gt=True, min_depth=1.0, max_depth=80.0))
    counts, caps, _ = check_case(backend, dev, case, "degenerate keeps")
    assert counts.tolist() == [caps[0], 0, 1, 1, caps[4]]
    # the same through the mask, the prediction exported
    case = dict(pred=np.stack([depth_like(rng, 4, 6) for _ in shapes]), shapes=shapes, gts=gts,
                kw=dict(mask_gt=True, min_depth=1.0, max_depth=80.0))
    counts, _, _ = check_case(backend, dev, case, "degenerate keeps through the mask")
    assert counts.tolist() == [caps[0], 0, 1, 1, caps[4]]

    # 0, negative values, infinities and NaN, isolated from one another by four finite pixels
    special = [0.0, -3.0, np.inf, -np.inf, np.nan]
    shape = (12, 40)
    base = depth_like(rng, *shape)
    flat = base.reshape(-1)
    where = np.arange(len(special) * 6) * 5 + 43
    flat[where] = np.tile(special, 6)
    for clamp_depth in (False, True):
        kw = dict(min_depth=1.0, max_depth=60.0, clamp_depth=clamp_depth)
        # as ground truth: the value itself is the depth
        _, _, raws = check_case(backend, dev, dict(pred=np.ones((1, 2, 2), np.float32), shapes=[shape], gts=[base],
                                                   kw=dict(from_gt=True, **kw)), "specials as gt, clamp=%s" % clamp_depth)
        assert np.isnan(raws[0]).sum() == 6 and np.isinf(raws[0]).sum() == 12 and (raws[0] == 0).sum() == 6
        # as a prediction of the image's own size, depth and disparity: the resampling sees them (a weight of zero
        # times an infinity is a NaN, in the reference as in the kernel)
        for disp in (False, True):
            counts, caps, raws = check_case(backend, dev, dict(pred=base[None], shapes=[shape], kw=dict(pred_is_disp=disp, **kw)),
                                            "specials as prediction, disp=%s clamp=%s" % (disp, clamp_depth))
            r = raws[0]
            assert np.isnan(r).any() and (np.isinf(r).any() or not disp) and (r < 1.0).any()
            finite_in_range = int(((r >= 1.0) & (r <= 60.0)).sum())
            assert counts[0] == (int((~np.isnan(r)).sum()) if clamp_depth else finite_in_range)


# ------------------------------------------------------------------------------------------------ 4. window and stride
def check_window_and_stride(backend, dev):
    rng = np.random.default_rng(8)
    shape, window = (37, 91), (15, 36, 3, 88)
    depth = depth_like(rng, 8, 16)[None]
    rgbs = colours(rng, [shape])
    for stride in (1, 2, 3, 7, 100):
        for disp in (False, True):
            case = dict(pred=1.0 / depth if disp else depth, shapes=[shape], windows=[window], rgbs=rgbs,
                        kw=dict(stride=stride, pred_is_disp=disp, min_depth=1e-3, max_depth=125.0))
            counts, caps, _ = check_case(backend, dev, case, "window %s stride %d disp=%s" % (window, stride, disp))
            want = len(range(15, 36, stride)) * len(range(3, 88, stride))
            assert caps == [want] and counts.tolist() == [want]           # capacity equals the candidate count
            assert stride != 100 or want == 1                             # a stride beyond the window: one candidate
    # a window that reaches outside the image is cut to it
    case = dict(pred=depth, shapes=[shape], windows=[(-4, 50, 80, 200)], kw=dict(stride=2, max_depth=80.0))
    counts, caps, _ = check_case(backend, dev, case, "window cut to the image")
    assert caps == [len(range(0, 37, 2)) * len(range(80, 91, 2))] == counts.tolist()


# ------------------------------------------------------------------------------------------------ 5. nothing else
def check_nothing_else_is_written(backend, dev):
    """check_case compares every byte already; here with wide gaps, a partial keep and the capacity tail made explicit."""
    rng = np.random.default_rng(21)
    shapes = [(17, 29), (5, 7), (30, 65)]
    gts = [depth_like(rng, gh, gw) for gh, gw in shapes]
    for g in gts:
        g[rng.random(g.shape) < 0.4] = 0.0
    case = dict(pred=np.stack([depth_like(rng, 6, 9) for _ in shapes]), shapes=shapes, gts=gts,
                kw=dict(mask_gt=True, clamp_depth=True, min_depth=1e-3, max_depth=80.0))
    got, counts, regions, caps = run_case(backend, dev, case, guard=300, gap=129)
    want, want_counts, _ = expected(case, regions, got.size)
    assert np.array_equal(counts, want_counts) and np.array_equal(got, want)
    written = np.zeros(got.size, bool)
    for r, c, cap in zip(regions, counts, caps):
        assert 0 < c < cap
        written[r * V:(r + int(c)) * V] = True
    assert (got[~written] == FILL).all() and written.sum() == V * int(counts.sum())
    assert (got[:300 * V] == FILL).all() and (got[-300 * V:] == FILL).all()


# ------------------------------------------------------------------------------------------------ 6. determinism, arguments
class Recorder:
    """Passes a backend's calls through and keeps the last call's arguments."""

    def __init__(self, inner):
        self.inner, self.lib, self.name = inner, inner.lib, inner.name
        self.call = None

    def _check(self, *tensors):
        return self.inner._check(*tensors)

    def run(self, name, anchor, *args):
        self.call = (name, anchor, args)
        return self.inner.run(name, anchor, *args)


def status(backend, name, anchor, args):
    """The status the entry point returns for `args`, on either tier."""
    if hasattr(backend, "status"):
        return backend.status(name, *args)
    return getattr(backend.lib._dll, name)(*args, backend.lib.stream_for(anchor))


# positions in the argument list of bbd_point_cloud
PRED, GT, DESC, ROWS, INV_K, RGB, LUT, VERT, COUNTS, SCRATCH, N_INTS, N, H, W, MAX_H, MAX_W, STRIDE = range(17)
FLAGS = 22


def check_determinism_and_arguments(backend, dev):
    rng = np.random.default_rng(3)
    shapes = [(20, 31), (9, 100)]
    gts = [depth_like(rng, gh, gw) for gh, gw in shapes]
    gts[0][rng.random(gts[0].shape) < 0.3] = 0.0
    case = dict(pred=1.0 / np.stack([depth_like(rng, 6, 9) for _ in shapes]), shapes=shapes, gts=gts, ratios=[1.5, 0.7],
                kw=dict(mask_gt=True, clamp_depth=True, pred_is_disp=True, min_depth=1e-3, max_depth=125.0))
    rec = Recorder(backend)
    a = run_case(rec, dev, case)
    b = run_case(backend, dev, case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # two calls, equal bytes

    # every refusal of the contract: the status, and the pre-filled buffer stays as it is
    name, anchor, good = rec.call
    assert name == "bbd_point_cloud" and len(good) == 23
    regions, caps, total = layout(case)
    out = torch.full((total * V,), FILL, dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev)
    good = list(good)
    good[VERT], good[COUNTS] = _lib.ptr(out), _lib.ptr(counts)
    null = ctypes.c_void_p(0)

    def refused(changes, want=-1):
        args = list(good)
        for k, v in changes.items():
            args[k] = v
        rc = status(backend, name, anchor, args)
        assert rc == want, (changes, rc)

    for k in (PRED, DESC, INV_K, VERT, COUNTS, SCRATCH):
        refused({k: null})
    refused({GT: null})                                             # MASK_GT reads the ground truth
    refused({GT: null, FLAGS: _lib.EVAL_PRED_IS_DISP | _lib.CLOUD_FROM_GT})
    refused({RGB: null, LUT: null})                                 # no colour source at all
    for k in (N, H, W, MAX_H, MAX_W, STRIDE):
        refused({k: 0})
        refused({k: -1})
    for bit in (_lib.EVAL_MEDIAN_MIDPOINT, _lib.EVAL_NO_MEDIAN_SCALING, _lib.SYNS_RAYS_PIXEL, 256, 1 << 30):
        refused({FLAGS: good[FLAGS] | bit})
    refused({N_INTS: good[N_INTS] - 1})                             # scratch too small
    refused({VERT: ctypes.c_void_p(out.data_ptr() + 8)})            # vertices must be 16-byte aligned
    refused({N: 65536}, want=-2)
    refused({MAX_H: 65536, MAX_W: 65536}, want=-2)
    assert backend.lib.point_cloud_scratch_ints(0, 4, 4, 1) == -1 and backend.lib.point_cloud_scratch_ints(1, 4, 4, 0) == -1
    assert backend.lib.point_cloud_scratch_ints(1, 65536, 65536, 1) == -2
    assert backend.lib.point_cloud_scratch_ints(3, 16, 16, 1) == 3 and backend.lib.point_cloud_scratch_ints(3, 17, 16, 1) == 6
    assert (out.cpu().numpy() == FILL).all() and (counts.cpu().numpy() == -7).all()


# ------------------------------------------------------------------------------------------------ 7. what the metric scored
def check_cloud_is_what_the_metric_scored(backend, dev):
    """The exported clouds, through bbd_chamfer_nn and the header's definition of P and R, against bbd_syns_pointcloud's
    {P, R, count_p, count_t, N} for the same images - once per ray pairing."""
    rng = np.random.default_rng(17)
    shape, n = (24, 40), 2
    gts_np, depth = [], []
    for i in range(n):
        g = (4.0 + 6.0 * rng.random(shape)).astype(np.float32)
        depth.append(g * (1.0 + 0.01 * rng.standard_normal(shape)))      # a prediction about 1 % off, at the same size
        g[rng.random(shape) < 0.2] = 0.0                         # no return
        g[rng.random(shape) < 0.03] = 130.0                      # beyond the SYNS range
        gts_np.append(g)
    gts = evaluation.GroundTruthSet(gts_np, dev, crop=False)
    pred = torch.from_numpy((1.0 / np.stack(depth)).astype(np.float32)).to(dev)
    rows_np = np.zeros((n, _lib.EVAL_OUT), np.float32)
    rows_np[:, 7] = [1.0078125, 0.99609375]
    rows = torch.from_numpy(rows_np).to(dev)
    inv_K = syns_ref.syns_camera(*shape)[1]
    lo, hi, th = evaluation.SYNS_MIN_DEPTH, evaluation.SYNS_MAX_DEPTH, np.float32(evaluation.SYNS_CLOUD_TH)
    valid = [int(((g > np.float32(lo)) & (g < np.float32(hi))).sum()) for g in gts_np]
    assert all(0.7 * g.size < v < g.size for v, g in zip(valid, gts_np))       # the mask matters, most pixels stay
    for rays in ("pixel", "reference"):
        pc = evaluation.pointcloud_metrics(pred, gts, [0, 1], rows, inv_K, pred_is_disp=True, rays=rays,
                                           backend=backend).cpu().numpy()
        kw = dict(gt=gts.buffer, min_depth=lo, max_depth=hi, mask_gt=True, rays=rays, backend=backend)
        vp, cp, op = ops.point_cloud(pred, gts.desc_host[[0, 1]], inv_K, rows=rows, pred_is_disp=True, clamp_depth=True, **kw)
        vt, ct, ot = ops.point_cloud(pred, gts.desc_host[[0, 1]], inv_K, from_gt=True, **kw)
        cp, ct = cp.cpu().numpy(), ct.cpu().numpy()
        assert cp.tolist() == ct.tolist() == valid
        for i in range(n):
            N = valid[i]
            P = vp.view(torch.float32).view(-1, 4)[op[i]:op[i] + N, :3].contiguous()
            T = vt.view(torch.float32).view(-1, 4)[ot[i]:ot[i] + N, :3].contiguous()
            nn_p, nn_t = ops.chamfer_nn(P, T, backend=backend)
            count_p = int((np.sqrt(nn_p.cpu().numpy()) < th).sum())
            count_t = int((np.sqrt(nn_t.cpu().numpy()) < th).sum())
            want = np.array([np.float32(count_p) / np.float32(N), np.float32(count_t) / np.float32(N), count_p, count_t, N],
                            np.float32)
            print("rays %s image %d: P, R, count_p, count_t, N = %s; bbd_syns_pointcloud %s" % (rays, i, want, pc[i, 2:7]))
            assert np.array_equal(want.view(np.uint32), pc[i, 2:7].view(np.uint32)), (rays, i)
            assert 0 < count_p < N                                  # a comparison that can fail: neither all nor none


ALL_CHECKS = [check_ragged, check_wave_and_chunk_edges, check_degenerate, check_window_and_stride,
              check_nothing_else_is_written, check_determinism_and_arguments, check_cloud_is_what_the_metric_scored]
