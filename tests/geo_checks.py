"""The cases of the geometry-consistency loss (`bbd_geo_fwd` / `bbd_geo_bwd`), shared by the CPU tier
(tests/test_geo_port.py: the host port against the float64 reference) and the GPU tier (tests/test_gpu_geo.py: the
device against the host port, byte for byte).  Test infrastructure only.

A case is the five inputs and a weight per pair; `run` calls `ops.geometry_consistency`, takes the gradient of
sum(weights * pair_sum) and returns every output as numpy.  The street scenes are those of tests/geo_ref.py at 19 x 67
(67 crosses a wave edge, 1 273 pixels are one ragged work item) and 33 x 130 (4 290 pixels: three work items a sample);
`full` is the one full-size case, 192 x 640 (60 work items a sample).

Tolerances against the reference (float32 against float64): the loss within 1e-5 relative, every gradient within 1e-4
of that gradient's largest magnitude - the project's bars.  Samples within 1e-3 of a kink of the loss are left out of
the comparison of the two depth gradients (not of the pose gradient); the reference must show them to be at most 2 % of
the visible ones."""
import functools

import numpy as np
import torch

import geo_ref as ref
from consist_checks import spoil
from baseboostdepth_amd import ops

SMALL, MID, LARGE = (19, 67), (33, 130), (192, 640)
OUTPUTS = ("loss", "pair_sum", "pair_count", "err", "code", "grad_q_tgt", "grad_q_src", "grad_T")
LOSS_TOL, GRAD_TOL, KINK_SHARE = 1e-5, 1e-4, 0.02
SEEDS = {"street19": 0, "street33": 0}


def exact_camera(B):
    """Focal lengths and centre that are powers of two, with the exact inverse, as [B,16]."""
    K, inv_K = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    K[:2, :3] = [[64.0, 0.0, 32.0], [0.0, 32.0, 8.0]]
    inv_K[:2, :3] = [[1.0 / 64.0, 0.0, -0.5], [0.0, 1.0 / 32.0, -0.25]]
    return np.tile(K.reshape(1, 16), (B, 1)), np.tile(inv_K.reshape(1, 16), (B, 1))


def _dyadic(shape, seed):
    """Inverse depths 1/8, 1/4 and 1/2: their sums, differences and products with 8, 4 and 2 are exact in float32."""
    return np.random.default_rng(seed).choice(np.array([0.125, 0.25, 0.5], np.float32), shape)


def _flat(B, V, size, yaw=0.0):
    """Identical cameras (or sources turned by `yaw`) on the exact camera, q_src == q_tgt."""
    import consist_ref
    K, inv_K = exact_camera(B)
    q = _dyadic((B,) + size, 7)
    T = np.tile(ref.relative(consist_ref.pose(), consist_ref.pose(yaw=yaw)), (V, B, 1))
    return dict(q_tgt=q, q_src=np.ascontiguousarray(np.broadcast_to(q, (V,) + q.shape)), T=T, K=K, inv_K=inv_K)


@functools.lru_cache(maxsize=None)
def make(name):
    if name == "street19":
        case = ref.scene(2, 2, *SMALL, seed=SEEDS[name])
    elif name == "street33":
        case = ref.scene(2, 2, *MID, seed=SEEDS[name])
    elif name == "full":
        case = ref.scene(1, 2, *LARGE, seed=0)
    elif name == "spoilt":
        case = ref.scene(2, 2, *MID, seed=1)
        case["q_tgt"], case["q_src"] = spoil(case["q_tgt"], 4), spoil(case["q_src"], 5)
    elif name == "v1_b1":
        case = ref.scene(1, 1, *SMALL, seed=2)
    elif name == "v8_b3":
        case = ref.scene(3, 8, *SMALL, seed=3)
    elif name == "identical":
        case = _flat(2, 2, SMALL)
    elif name == "turned":
        case = _flat(2, 2, SMALL, yaw=np.pi)
    elif name in ("thin_h", "thin_w"):
        case = _flat(2, 2, (1, 9) if name == "thin_h" else (7, 1))
    else:
        raise KeyError(name)
    V, B = case["q_src"].shape[:2]
    case["weights"] = (1.0 / (1.0 + np.arange(V * B, dtype=np.float64))).reshape(V, B)
    for a in case.values():
        a.setflags(write=False)
    return case


CASES = ("street19", "street33", "spoilt", "v1_b1", "v8_b3", "identical", "turned", "thin_h", "thin_w")
STREETS = ("street19", "street33")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference's answer to a case (computed once, shared, never changed)."""
    case = make(name)
    out = ref.geometry(case["q_tgt"], case["q_src"], case["T"], case["K"], case["inv_K"], case["weights"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def tensors(case, device):
    return {k: torch.from_numpy(np.array(v)).to(device) for k, v in case.items()}


def run(name, backend, device):
    """Every output of a case as numpy arrays: the forward's, and the gradients of sum(weights * pair_sum)."""
    t = tensors(make(name), device)
    q_tgt, q_src, T = (t[k].requires_grad_() for k in ("q_tgt", "q_src", "T"))
    res = ops.geometry_consistency(q_tgt, q_src, T, t["K"], t["inv_K"], want_err=True, want_code=True, backend=backend)
    (res.pair_sum * t["weights"]).sum().backward()
    out = {k: getattr(res, k).detach().cpu().numpy() for k in ("loss", "pair_sum", "pair_count", "err", "code")}
    out.update(grad_q_tgt=q_tgt.grad.cpu().numpy(), grad_q_src=q_src.grad.cpu().numpy(), grad_T=T.grad.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def port_result(name):
    """The host port's answer to a case (computed once, shared, never changed)."""
    from ports import PortBackend
    out = run(name, PortBackend(), "cpu")
    for v in out.values():
        v.setflags(write=False)
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(got, want):
    """The outputs of two results that are not the same bytes."""
    return [k for k in OUTPUTS if not same_bytes(got[k], want[k])]


def all_finite(got):
    return all(np.isfinite(got[k]).all() for k in OUTPUTS)


def excluded(r):
    """(pixels [B,H,W], taps [V,B,H,W]) left out of the depth gradients' comparison: the target pixels with a sample near
    a kink, and the four taps of every such sample."""
    near = r["near_kink"]
    V, B, H, W = near.shape
    taps = np.zeros(near.shape, bool)
    v, b, y, x = np.nonzero(near)
    x0, y0 = r["x0"][v, b, y, x], r["y0"][v, b, y, x]
    for dy in (0, 1):
        for dx in (0, 1):
            taps[v, b, y0 + dy, x0 + dx] = True
    return near.any(0), taps


def against_reference(name, got):
    """The street cases: counts and codes equal, the loss and the gradients within the bars; prints every figure."""
    r = reference(name)
    visible = int(r["pair_count"].sum())
    share = float(r["near_kink"].sum()) / max(visible, 1)
    pixels, taps = excluded(r)
    figures = dict(visible=visible, of=int(r["code"].size), kink_share=share,
                   loss=float(got["loss"]), loss_rel=abs(float(got["loss"]) - float(r["loss"])) / abs(float(r["loss"])))
    for k, keep in (("grad_q_tgt", ~pixels), ("grad_q_src", ~taps), ("grad_T", np.ones(r["grad_T"].shape, bool))):
        figures[k] = float(np.abs(got[k].astype(np.float64) - r[k])[keep].max() / np.abs(r[k]).max())
    print(name, figures)
    assert share <= KINK_SHARE and visible > 0.8 * r["code"].size, figures
    assert taps.mean() <= 4 * KINK_SHARE
    assert np.array_equal(got["pair_count"], r["pair_count"]) and np.array_equal(got["code"], r["code"]), figures
    assert (r["code"] == 1).sum() > 0.6 * visible and (r["code"] == 3).sum() > 0     # a - 1 has a definite sign on most
    assert figures["loss_rel"] <= LOSS_TOL, figures
    # e moves by half the relative error of a = z s; s is sampled at a coordinate known to a few ulps of W, and across a
    # depth edge it changes by about itself in one pixel: 130 * 2^-22 / 2 = 1.6e-5 at the larger size
    assert np.abs(got["err"].astype(np.float64) - r["err"]).max() <= 2e-5, figures
    for k in ("grad_q_tgt", "grad_q_src", "grad_T"):
        assert figures[k] <= GRAD_TOL and np.abs(r[k]).max() > 0, (k, figures)
    return figures


def precondition(name, got):
    """What a case other than the streets must show, exactly."""
    case = make(name)
    V, B, H, W = case["q_src"].shape
    assert all_finite(got), name
    if name == "identical":
        vis = (got["code"] & 1) == 1
        assert vis.all() and (got["err"] == 0.0).all() and got["loss"] == 0.0
        assert (got["code"] == 1).all() and got["pair_count"].tolist() == [[H * W] * B] * V
        assert not got["grad_q_tgt"].any() and not got["grad_q_src"].any() and not got["grad_T"].any()   # a == 1: slope 0
    if name in ("turned", "thin_h", "thin_w"):
        assert not got["pair_count"].any() and got["loss"] == 0.0 and not got["pair_sum"].any()
        assert not got["code"].any() and not got["err"].any()
        for k in ("grad_q_tgt", "grad_q_src", "grad_T"):
            assert same_bytes(got[k], np.zeros(got[k].shape, np.float32)), k
    if name == "spoilt":
        clean = ref.scene(2, 2, *MID, seed=1)
        was = ref.geometry(clean["q_tgt"], clean["q_src"], clean["T"], clean["K"], clean["inv_K"])
        bad_t = ~((case["q_tgt"] > 0) & np.isfinite(case["q_tgt"]))
        now = (got["code"] & 1) == 1
        assert 0.03 < bad_t.mean() < 0.07 and not now[:, bad_t].any()                    # spoilt target pixels
        assert ((was["code"] & 1 == 1) & ~now & ~bad_t[None]).sum() > 100                # spoilt taps
        assert not (now & (was["code"] & 1 == 0)).any() and now.sum() > 4000
        assert not got["grad_q_tgt"][bad_t].any() and np.abs(got["grad_q_tgt"]).max() > 0
    if name in ("v1_b1", "v8_b3"):
        assert (got["pair_count"] > 0.3 * H * W).all() and tuple(got["pair_sum"].shape) == (V, B)
        assert all(np.abs(got[k]).max() > 0 for k in ("grad_q_tgt", "grad_q_src", "grad_T"))
        assert np.abs(got["grad_T"]).reshape(V * B, 12).max(1).min() > 0                 # every pair has a pose gradient


# Argument errors: (entry, change, status).  None = a NULL pointer.
BAD = [("fwd", {k: None}, -1) for k in "q_tgt q_src T K inv_K pair_sum pair_count scratch".split()] + \
      [("bwd", {k: None}, -1) for k in "q_tgt q_src T K inv_K g grad_q_tgt grad_q_src grad_T scratch".split()] + \
      [(e, c, s) for e in ("fwd", "bwd") for c, s in (
          (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(V=0), -1), (dict(V=9), -1),
          (dict(scratch_words="short"), -1), (dict(H=4096, W=4096), -2), (dict(B=300, H=2048, W=2048, V=2), -2))]
ORDER = dict(fwd="q_tgt q_src T K inv_K pair_sum pair_count err code scratch scratch_words B H W V".split(),
             bwd="q_tgt q_src T K inv_K g grad_q_tgt grad_q_src grad_T scratch scratch_words B H W V".split())


def bad_argument_sweep(status, device):
    """Every row of BAD through `status(name, *args)` (the port's or the device library's raw call): the status is the
    ABI's and no buffer changes.  Ends with valid calls, which do write - the forward also without its optional outputs."""
    from baseboostdepth_amd._lib import ptr
    case = make("street19")
    V, B, H, W = case["q_src"].shape
    ins = tensors(case, device)
    ins["g"] = ins.pop("weights")
    words = dict(fwd=ops.geo_scratch_words(B, H, W, V, False), bwd=ops.geo_scratch_words(B, H, W, V, True))
    bufs = dict(pair_sum=torch.full((V, B), 7.0, dtype=torch.float64), pair_count=torch.full((V, B), 7, dtype=torch.int64),
                err=torch.full((V, B, H, W), 7.0), code=torch.full((V, B, H, W), 7, dtype=torch.uint8),
                grad_q_tgt=torch.full((B, H, W), 7.0), grad_q_src=torch.full((V, B, H, W), 7.0),
                grad_T=torch.full((V, B, 12), 7.0), scratch=torch.full((words["bwd"],), 7, dtype=torch.int64))
    bufs = {k: v.to(device) for k, v in bufs.items()}
    before = {k: v.clone() for k, v in bufs.items()}

    def sync():
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()

    def call_with(entry, change):
        args = dict(B=B, H=H, W=W, V=V, scratch_words=words[entry])
        args.update({k: ptr(v) for k, v in list(bufs.items()) + list(ins.items())})
        for k, v in change.items():
            args[k] = ptr(None) if v is None else words[entry] - 1 if v == "short" else v
        return status("bbd_geo_" + entry, *[args[k] for k in ORDER[entry]])

    for entry, change, want in BAD:
        assert call_with(entry, change) == want, (entry, change)
    sync()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    want = port_result("street19")
    assert call_with("fwd", dict(err=None, code=None)) == 0               # the optional outputs
    sync()
    assert torch.equal(bufs["err"], before["err"]) and torch.equal(bufs["code"], before["code"])
    assert same_bytes(bufs["pair_sum"].cpu().numpy(), want["pair_sum"])
    assert call_with("fwd", {}) == 0 and call_with("bwd", {}) == 0
    sync()
    got = {k: v.cpu().numpy() for k, v in bufs.items()}
    assert all(same_bytes(got[k], want[k]) for k in OUTPUTS if k != "loss")
