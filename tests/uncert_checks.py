"""The cases of the uncertainty kernels (`bbd_post_process_uncert`, `bbd_sparsification`), shared by the
CPU tier (tests/test_uncert_port.py: the host port against the numpy reference tests/uncert_ref.py) and the GPU tier
(tests/test_gpu_uncert.py: the device against the port, byte for byte).  Test infrastructure only.

Every sparsification case is a ragged batch of 2-3 small maps in ONE call.  The prediction has another size than the
maps (so both resizes work) except where a case must control the resampled uncertainty itself: `dense` (random bit
patterns as keys), `ties` (four levels must stay four) and `perfect` (the uncertainty is e_abs).  The metrics rows every
call takes (`rows[i][7]`, the median-scaling ratio) come from `depth_metrics` on the host port, computed once per case
and shared by the reference, the port and the device."""
import functools

import numpy as np
import torch

import uncert_ref as ref
from baseboostdepth_amd import _lib, evaluation, ops

F = np.float32
CASES = ("tiny", "exact", "ragged", "dense", "ties", "spoilt", "empty", "unscaled", "k1", "k100", "perfect")
FLIP_WIDTHS = (1, 2, 7, 64)
RAGGED = ((24, 80), (37, 122), (12, 40))


def _scene(shape, rng):
    """A smooth depth field between 4 and 60 m at `shape`, with 10 % noise."""
    gh, gw = shape
    y, x = np.mgrid[0:gh, 0:gw]
    depth = 4.0 + 56.0 * (1.0 - (y + 0.5) / gh) * (0.6 + 0.4 * np.cos(3.0 * (x + 0.5) / gw))
    return np.clip((np.abs(depth) + 2.0) * (1.0 + 0.1 * rng.standard_normal(shape)), 1.0, 75.0)


def _gt(shape, rng, share=None, count=None):
    """Ground truth at `shape`: `share` of the pixels (or exactly `count` of them) carry a depth, the others 0."""
    depth = _scene(shape, rng)
    keep = np.zeros(depth.size, bool)
    if count is not None:
        keep[rng.permutation(depth.size)[:count]] = True
    else:
        keep = rng.random(depth.size) < share
    return np.where(keep.reshape(shape), depth, 0.0).astype(F)


def _batch(shapes, size, rng, **gt_kw):
    """(gts, pred disparity [n,h,w], uncert [n,h,w]): the disparity of the same scene at `size`, half the true scale, and
    an uncertainty that knows something about the error (the noise it was drawn with) plus noise of its own."""
    kws = gt_kw.pop("per_map", [gt_kw] * len(shapes))
    gts = [_gt(s, rng, **kw) for s, kw in zip(shapes, kws)]
    pred, uncert = [], []
    for _ in shapes:
        noise = 0.15 * rng.standard_normal(size)
        pred.append(1.0 / (2.0 * _scene(size, rng) * np.abs(1.0 + noise)))
        uncert.append(np.abs(noise) * 0.05 + 0.01 * rng.random(size))
    return gts, np.stack(pred).astype(F), np.stack(uncert).astype(F)


def _case(gts, pred, uncert, crop, K=50, median_scaling=True, scale_factor=1.0):
    return dict(gts=gts, pred=np.ascontiguousarray(pred, F), uncert=np.ascontiguousarray(uncert, F), crop=crop, K=K,
                median_scaling=median_scaling, scale_factor=scale_factor, min_depth=1e-3, max_depth=80.0)


def _random_floats(shape, rng):
    """Finite float32 values of random bit patterns: every byte of the key takes (nearly) every value."""
    bits = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7f800000) == 0x7f800000] &= 0xbfffffff          # inf / NaN -> finite
    return bits.view(F)


@functools.lru_cache(maxsize=None)
def make(name):
    rng = np.random.default_rng(sum(ord(c) for c in name))
    if name == "tiny":                       # N = 1, 3 and 7 < K: most buckets are empty
        shapes = ((3, 5), (7, 9), (7, 9))
        gts, pred, uncert = _batch(shapes, (4, 6), rng, per_map=[dict(count=1), dict(count=3), dict(count=7)])
        return _case(gts, pred, uncert, crop=False)
    if name == "exact":                      # N = K and N = 2 K
        gts, pred, uncert = _batch(((10, 12), (11, 13)), (6, 8), rng, per_map=[dict(count=50), dict(count=100)])
        return _case(gts, pred, uncert, crop=False)
    if name in ("ragged", "k1", "k100", "unscaled"):
        gts, pred, uncert = _batch(RAGGED, (16, 52), np.random.default_rng(11), share=0.05 if name != "unscaled" else 0.3)
        if name == "unscaled":
            return _case(gts, pred * F(2.0 * 5.4), uncert, crop=True, median_scaling=False, scale_factor=5.4)
        return _case(gts, pred, uncert, crop=True, K={"ragged": 50, "k1": 1, "k100": 100}[name])
    if name == "dense":                      # 30 720 pixels: 30 sort chunks, keys whose four bytes all vary
        shapes = ((96, 320), (9, 33))
        gts, pred, _ = _batch(shapes, (96, 320), rng, share=2.0)
        return _case(gts, pred, _random_floats(pred.shape, rng), crop=False)
    if name == "ties":                       # four levels, and a constant map: the tie rule decides everything
        gts, pred, uncert = _batch(((24, 80), (24, 80)), (24, 80), rng, share=0.5)
        uncert[0] = F(0.25) * rng.integers(0, 4, uncert[0].shape).astype(F)
        uncert[1] = F(0.5)
        return _case(gts, pred, uncert, crop=True)
    if name == "spoilt":                     # an external uncertainty file may hold anything; a NaN in the prediction
        gts, pred, uncert = _batch(RAGGED, (16, 52), rng, share=0.3)
        hit = rng.random(uncert.shape) < 0.1
        kind = rng.integers(0, 4, uncert.shape)
        for k, bad in enumerate((np.nan, np.inf, -0.0, -0.3)):
            uncert[hit & (kind == k)] = bad
        pred[1, 12, 30] = np.nan
        return _case(gts, pred, uncert, crop=True)
    if name == "empty":
        gts, pred, uncert = _batch(RAGGED, (16, 52), rng, share=0.3)
        gts[1][:] = 0.0
        return _case(gts, pred, uncert, crop=True)
    if name == "perfect":                    # the uncertainty is e_abs itself, at the maps' own size
        shapes = ((24, 80), (24, 80))
        gts, pred, uncert = _batch(shapes, (24, 80), rng, share=0.4)
        case = _case(gts, pred, uncert, crop=True)
        ratios = _rows(case)[:, 7]
        for i, gt in enumerate(gts):
            t = ref.terms(pred[i], uncert[i], gt, windows(case)[i], ratios[i])
            plane = np.zeros(gt.shape, F)
            plane[t["mask"]] = t["e_abs"]
            case["uncert"][i] = plane
        return case
    raise KeyError(name)


def windows(case):
    return [evaluation.garg_window(*g.shape) if case["crop"] else (0, g.shape[0], 0, g.shape[1]) for g in case["gts"]]


def _port():
    import ports
    return ports.PortBackend()


def _rows(case):
    """The float32 [n,12] rows `depth_metrics` gives the case's predictions, on the host port."""
    gts = evaluation.GroundTruthSet(case["gts"], "cpu", crop=case["crop"])
    rows = evaluation.depth_metrics(torch.from_numpy(case["pred"]), gts, list(range(len(case["gts"]))),
                                    min_depth=case["min_depth"], max_depth=case["max_depth"], pred_is_disp=True,
                                    median="numpy", median_scaling=case["median_scaling"],
                                    scale_factor=case["scale_factor"], backend=_port())
    return rows.numpy()


@functools.lru_cache(maxsize=None)
def rows(name):
    r = _rows(make(name))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy reference's answer to a case (computed once, shared, never changed)."""
    case = make(name)
    out = ref.sparsification(case["pred"], case["uncert"], case["gts"], windows(case), rows(name)[:, 7], K=case["K"],
                             min_depth=case["min_depth"], max_depth=case["max_depth"], scale_factor=case["scale_factor"],
                             median_scaling=case["median_scaling"])
    out["out"].setflags(write=False)
    return out


def run(name, backend, device):
    """`ops.sparsification` on a case -> float64 [n, 8 + 6 (K + 1)] as a numpy array."""
    case = make(name)
    gts = evaluation.GroundTruthSet(case["gts"], device, crop=case["crop"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    out = ops.sparsification(dev(case["pred"]), dev(case["uncert"]), gts, list(range(len(case["gts"]))), dev(rows(name).copy()),
                             intervals=case["K"], min_depth=case["min_depth"], max_depth=case["max_depth"],
                             scale_factor=case["scale_factor"], median_scaling=case["median_scaling"], backend=backend)
    return out.cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def split(out, K):
    """(summary [n,8], curves [n,2,3,K+1]) of an `out` tensor."""
    return out[:, :ref.SUMMARY], out[:, ref.SUMMARY:].reshape(out.shape[0], 2, 3, K + 1)


def precondition(name):
    """What keeps a case from going hollow, asserted on the reference alone; prints the figures."""
    case, r = make(name), reference(name)
    K = case["K"]
    summary, curves = split(r["out"], K)
    Ns = summary[:, 6].astype(int).tolist()
    print("%s: N %s, AUSE %s, AURG %s" % (name, Ns, summary[:, :3].round(4).tolist(), summary[:, 3:6].round(4).tolist()))
    if name == "tiny":
        assert Ns == [1, 3, 7]
    if name == "exact":
        assert Ns == [50, 100] and K == 50
    if name in ("ragged", "k1", "k100"):
        assert all(10 < N < 400 and N % 50 for N in Ns), Ns           # about 5 % of the Garg windows
        assert K == {"ragged": 50, "k1": 1, "k100": 100}[name]
        assert (summary[:, 3] > 0).all()                   # the uncertainty knows something: it beats random removal
    if name == "dense":
        assert Ns == [30720, 297]
        keys = np.stack([ref.order_key(r["terms"][0][k]) for k in ("u", "e_abs", "e_sq", "th")])
        distinct = [len(np.unique((keys >> shift) & 255)) for shift in (0, 8, 16, 24)]
        print("dense: distinct values per key byte %s" % distinct)
        assert min(distinct) >= 200, distinct
    if name == "ties":
        levels = [len(np.unique(ref.order_key(t["u"]))) for t in r["terms"]]
        assert max(levels) <= 4 and levels[1] == 1 and min(Ns) > 200, (levels, Ns)
    if name == "spoilt":
        u = np.concatenate([t["u"] for t in r["terms"]])
        assert np.isnan(u).any() and np.isposinf(u).any() and (u < 0).any() and (case["uncert"].view(np.uint32) == 0x80000000).any()
        hit = np.isnan(r["terms"][1]["e_abs"])
        assert 0 < hit.sum() < 40 and not np.isnan(r["terms"][0]["e_abs"]).any() and not np.isnan(r["terms"][2]["e_abs"]).any()
        assert np.isfinite(r["out"][[0, 2]]).all()
        # the NaN prediction reaches abs_rel and rmse of its map - as long as a NaN pixel remains - and nothing else
        assert np.isnan(summary[1, [0, 1, 3, 4]]).all() and np.isfinite(summary[1, [2, 5, 6]]).all()
        assert np.isfinite(curves[1, :, 2]).all() and np.isnan(curves[1, :, :2, 0]).all()
        assert np.isfinite(curves[1, 1, :2, 1:]).all()     # the oracle removes the NaN pixels first
    if name == "empty":
        assert [N == 0 for N in Ns] == [False, True, False] and np.isnan(r["out"][1, :6]).all()
        assert np.isnan(r["out"][1, 8:]).all() and np.isfinite(r["out"][[0, 2]]).all()
    if name == "unscaled":
        assert not case["median_scaling"] and case["scale_factor"] == 5.4 and (summary[:, 3] > 0).all()
    if name == "perfect":
        assert (summary[:, 0] == 0.0).all() and min(Ns) > 200, summary[:, 0]


# ---------------------------------------------------------------------------- the flip pass
@functools.lru_cache(maxsize=None)
def make_flip(w):
    rng = np.random.default_rng(100 + w)
    return (0.01 + rng.random((6, 5, w))).astype(F)          # n = 3, h = 5


def run_flip(w, backend, device):
    """(out, uncert, out of ops.post_process_disp) as numpy arrays."""
    disp = torch.from_numpy(make_flip(w)).to(device)
    out, uncert = ops.post_process_uncert(disp, backend=backend)
    return out.cpu().numpy(), uncert.cpu().numpy(), ops.post_process_disp(disp, backend=backend).cpu().numpy()


# ---------------------------------------------------------------------------- argument errors
def bad_argument_sweep(status, device):
    """Every refusal of `bbd_sparsification` through `status(name, *args)` (the port's or the device library's raw call):
    BBD_E_BADARG, and the output buffer keeps its pattern.  Ends with a valid call, which writes the reference's row."""
    from baseboostdepth_amd._lib import ptr
    name = "ragged"
    case = make(name)
    n, h, w = case["pred"].shape
    K = case["K"]
    gts = evaluation.GroundTruthSet(case["gts"], device, crop=case["crop"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    ins = dict(pred=dev(case["pred"]), uncert=dev(case["uncert"]), gt=gts.buffer, desc=gts.desc, rows=dev(rows(name).copy()))
    nbytes = ops.sparsification_scratch_bytes(gts.desc_host, n)
    assert nbytes == 128 + 8916 * n + 81 * sum((r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in windows(case))
    bufs = dict(out=torch.full((n, 8 + 6 * (K + 1)), 7.0, dtype=torch.float64).to(device),
                scratch=torch.zeros((nbytes + 7) // 8, dtype=torch.int64).to(device))
    before = bufs["out"].clone()
    valid = dict(scratch_bytes=nbytes, n=n, h=h, w=w, intervals=K, min_depth=1e-3, max_depth=80.0, scale_factor=1.0, flags=0)
    order = "pred uncert gt desc rows out scratch scratch_bytes n h w intervals min_depth max_depth scale_factor flags".split()
    bad = [dict(pred=None), dict(uncert=None), dict(gt=None), dict(desc=None), dict(rows=None), dict(out=None),
           dict(scratch=None), dict(n=0), dict(n=65536), dict(h=0), dict(w=0), dict(intervals=0), dict(intervals=101),
           dict(flags=1), dict(flags=8), dict(scratch_bytes=nbytes - 1), dict(scratch_bytes=0)]

    def sync():
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()

    def call_with(change):
        args = dict(valid)
        args.update({k: ptr(v) for k, v in list(ins.items()) + list(bufs.items())})
        args.update({k: ptr(None) if v is None else v for k, v in change.items()})
        return status("bbd_sparsification", *[args[k] for k in order])

    for change in bad:
        assert call_with(change) == _lib.E_BADARG, change
    sync()
    assert torch.equal(bufs["out"], before)
    assert call_with({}) == 0
    sync()
    return bufs["out"].cpu().numpy()
