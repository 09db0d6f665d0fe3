"""GPU tier: the ResNet shortcut convolution - 1x1, stride 2, no padding, no bias - in its three directions on fp32 MFMA
(ops.conv1x1s2_fwd / conv1x1s2_bwd_data / conv1x1s2_wgrad / conv1x1_s2 / block_entry, csrc/bbd_conv1x1.hip) against float64
on the device,

    F.conv2d(x, w, None, 2)        and its autograd gradients for a random grad_out.

The ops are called directly, not through ops.CONV1X1_ROUTES.  The bounds are derived from the kernels' chain lengths, not
measured (include/bbd_hip.h): in (L + 1) * 2^-24 * sum |a| |b|, L is the number of fp32 roundings on the longest path,

    forward          L = C: conv1x1s2_fwd_kernel adds the C products of an output in one MFMA fma chain
    data gradient    L = K: conv1x1s2_bwd_data_kernel, one chain over the K output channels; accumulate mode adds the
                     result to the element in fp32 - one more rounding, and |grad_x before| joins the sum
    weight gradient  L = BBD_WGRAD_RUN (= 16 * BBD_C1_RUN_STRIPS of csrc/bbd_conv1x1_math.h): fp32 runs of that many
                     products, then float64

The largest observed share of each bound is printed, for information."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "baseboostdepth_amd", "csrc", "bbd_conv1x1_math.h")) as _f:
    RUN_STRIPS = int(re.search(r"#define BBD_C1_RUN_STRIPS (\d+)", _f.read()).group(1))

#         N  C    K    H  W
SHAPES = [(1, 16, 16, 2, 2),        # P' = 1: a lone pixel; one tile in every dimension
          (2, 16, 32, 5, 7),        # odd H and W; P' = 12 < 16
          (3, 32, 16, 6, 34),       # Wo = 17, P' = 51: rows not 16-byte aligned, a tail of 3, tiles crossing samples
          (2, 64, 128, 8, 40),      # layer2 in miniature; several K and C blocks
          (1, 256, 512, 6, 20)]     # layer4's channel counts on one small sample; weight-gradient workgroups with no pixels
KINDS = ["uniform", "outliers", "positive"]
CASES = [shape + (kind,) for shape in SHAPES for kind in KINDS]
BLOCK = (2, 64, 128, 8, 40)


def _ops():
    from baseboostdepth_amd import ops, _lib
    return ops, _lib


def _inputs(case):
    N, C, K, H, W, kind = case
    gen = torch.Generator().manual_seed(1000003 * N + 10007 * C + 101 * K + 13 * H + W)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2

    def draw(*shape):
        t = torch.rand(*shape, generator=gen)
        if kind != "positive":                                   # all-positive: nothing cancels, the sums are largest
            t = 2.0 * t - 1.0
        if kind == "outliers":                                   # a few elements of magnitude 1e4
            t = torch.where(torch.rand(*shape, generator=gen) < 0.02, t.sign() * 1e4, t)
        return t.to(DEV)

    return draw(N, C, H, W), draw(K, C, 1, 1), draw(N, K, Ho, Wo), draw(N, C, H, W)


_REFERENCE = {}


def _reference(case):
    """float64 results and the four bounds of a case: computed once, shared, left unchanged"""
    if case not in _REFERENCE:
        _, _lib = _ops()
        N, C, K, H, W, _ = case
        x, w, gy, gx0 = _inputs(case)
        x64, w64 = x.to(F64).requires_grad_(True), w.to(F64).requires_grad_(True)
        y64 = F.conv2d(x64, w64, None, 2)
        y64.backward(gy.to(F64))
        xa, wa = x.to(F64).abs().requires_grad_(True), w.to(F64).abs().requires_grad_(True)
        ya = F.conv2d(xa, wa, None, 2)
        ya.backward(gy.to(F64).abs())                            # xa.grad = sum |w| |gy|, wa.grad = sum |gy| |x|
        _REFERENCE[case] = {
            "y": y64.detach(), "gx": x64.grad, "gw": w64.grad, "gx_acc": gx0.to(F64) + x64.grad,
            "y_bound": (C + 1) * U * ya.detach(),
            "gx_bound": (K + 1) * U * xa.grad,
            "gx_acc_bound": (K + 2) * U * (xa.grad + gx0.to(F64).abs()),
            "gw_bound": (_lib.WGRAD_RUN + 1) * U * wa.grad,
        }
    return _REFERENCE[case]


def _share(got, want, bound):
    err = (got.to(F64) - want).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_C%d_K%d_H%d_W%d_%s" % c)
def test_three_directions_against_float64(case):
    ops, _lib = _ops()
    N, C, K, H, W, _ = case
    backend = ops.default_backend()
    lib = backend.lib
    assert lib.conv1x1s2_supported(N, C, K, H, W) == 1 and _lib.WGRAD_RUN == 16 * RUN_STRIPS == 128
    x, w, gy, gx0 = _inputs(case)
    ref = _reference(case)
    keep = (x.clone(), w.clone(), gy.clone())

    y = ops.conv1x1s2_fwd(x, w)
    gx = ops.conv1x1s2_bwd_data(gy, w, x.shape)
    acc = gx0.clone()
    assert ops.conv1x1s2_bwd_data(gy, w, x.shape, into=acc) is acc
    gw = ops.conv1x1s2_wgrad(x, w, gy)
    assert y.shape == ref["y"].shape and gx.shape == x.shape and gw.shape == w.shape
    assert y.dtype == gx.dtype == gw.dtype == F32
    assert all(torch.equal(a, b) for a, b in zip((x, w, gy), keep))
    shares = (_share(y, ref["y"], ref["y_bound"]), _share(gx, ref["gx"], ref["gx_bound"]),
              _share(acc, ref["gx_acc"], ref["gx_acc_bound"]), _share(gw, ref["gw"], ref["gw_bound"]))
    print("N%d C%d K%d H%d W%d %s: largest error / bound:" % case
          + " forward %.4f, data gradient %.4f, accumulated %.4f, weight gradient %.4f" % shares)

    # plain mode: the odd rows and columns are exact zeros; accumulate mode: they keep the input's bits
    odd = torch.ones(H, W, dtype=torch.bool, device=DEV)
    odd[::2, ::2] = False
    assert not bool(gx[:, :, odd].any())
    assert torch.equal(acc[:, :, odd], gx0[:, :, odd])

    # equal bits from a second launch, and from one whose outputs and scratch were NaN before: every element is written
    run, ptr = backend.run, _lib.ptr
    doubles = lib.conv1x1s2_wgrad_scratch_doubles(N, C, K, H, W)
    assert doubles > 0 and doubles == lib.conv1x1s2_wgrad_scratch_doubles(7 * N, C, K, H, W)     # it does not grow with N
    for _ in range(2):
        y2, gx2, gw2 = (torch.full_like(t, float("nan")) for t in (y, gx, gw))
        scratch = torch.full((doubles,), float("nan"), device=DEV, dtype=F64)
        acc2 = gx0.clone()
        run("bbd_conv1x1s2_fwd", x, ptr(x), ptr(w), ptr(y2), N, C, K, H, W)
        run("bbd_conv1x1s2_bwd_data", gy, ptr(gy), ptr(w), ptr(gx2), N, C, K, H, W, 0)
        run("bbd_conv1x1s2_bwd_data", gy, ptr(gy), ptr(w), ptr(acc2), N, C, K, H, W, 1)
        run("bbd_conv1x1s2_wgrad", x, ptr(x), ptr(gy), ptr(gw2), ptr(scratch), doubles, N, C, K, H, W)
        assert torch.equal(y2, y) and torch.equal(gx2, gx) and torch.equal(acc2, acc) and torch.equal(gw2, gw)
        assert not bool(torch.isnan(scratch).any())              # every record element is written


def _deterministic_convolutions(monkeypatch):
    """as tests/test_gpu_conv_wgrad.py: MIOpen's solvers that add with atomics are not chosen, so today's path repeats"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def _miopen_backward(gy, x, w, stride, padding):
    return torch.ops.aten.convolution_backward(gy, x, w, None, [stride, stride], [padding, padding], [1, 1], False, [0, 0], 1,
                                               [True, True, False])[:2]


def test_each_direction_forced_on_and_off_keeps_miopens_side_in_bits(monkeypatch):
    ops, _ = _ops()
    _deterministic_convolutions(monkeypatch)
    case = BLOCK + ("uniform",)
    x, w, gy, _ = _inputs(case)
    ref = _reference(case)
    y_m = F.conv2d(x, w, None, 2)
    gx_m, gw_m = _miopen_backward(gy, x, w, 2, 0)
    backend = ops.default_backend()
    names = []
    real = backend.run
    monkeypatch.setattr(backend, "run", lambda name, *a: (names.append(name), real(name, *a))[1])
    for fwd in (False, True):
        for dgrad in (False, True):
            for wgrad in (False, True):
                xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
                del names[:]
                y = ops.conv1x1_s2(xr, wr, fwd=fwd, dgrad=dgrad, wgrad=wgrad)
                y.backward(gy)
                assert names == (["bbd_conv1x1s2_fwd"] * fwd + ["bbd_conv1x1s2_wgrad"] * wgrad + ["bbd_conv1x1s2_bwd_data"] * dgrad)
                for got, mine, miopen, key in ((y.detach(), fwd, y_m, "y"), (xr.grad, dgrad, gx_m, "gx"), (wr.grad, wgrad, gw_m, "gw")):
                    if mine:
                        _share(got, ref[key], ref[key + "_bound"])
                    else:
                        assert torch.equal(got, miopen), (fwd, dgrad, wgrad, key)
    # a gradient that is not asked for is not computed
    del names[:]
    wr = w.clone().requires_grad_(True)
    ops.conv1x1_s2(x, wr, fwd=True, dgrad=True, wgrad=True).backward(gy)
    assert names == ["bbd_conv1x1s2_fwd", "bbd_conv1x1s2_wgrad"]


def test_block_entry_against_the_separate_calls(monkeypatch):
    ops, _lib = _ops()
    _deterministic_convolutions(monkeypatch)
    case = BLOCK + ("uniform",)
    N, C, K, H, W, _ = case
    x, w1, g1, _ = _inputs(case)
    ref = _reference(case)
    gen = torch.Generator().manual_seed(77)
    w3 = (0.1 * torch.randn(K, C, 3, 3, generator=gen)).to(DEV)
    g3 = torch.randn(N, K, H // 2, W // 2, generator=gen).to(DEV)
    y3_m = F.conv2d(x, w3, None, 2, 1)
    gx_m, gw3_m = _miopen_backward(g3, x, w3, 2, 1)
    y1_new = ops.conv1x1s2_fwd(x, w1)

    xr, w3r, w1r = (t.clone().requires_grad_(True) for t in (x, w3, w1))
    y3, y1 = ops.block_entry(xr, w3r, w1r, fwd=True, wgrad=True)
    torch.autograd.backward([y3, y1], [g3, g1])
    assert torch.equal(y3, y3_m) and torch.equal(y1, y1_new) and torch.equal(w3r.grad, gw3_m)
    share_w = _share(w1r.grad, ref["gw"], ref["gw_bound"])
    even = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    even[::2, ::2] = True
    assert torch.equal(xr.grad[:, :, ~even], gx_m[:, :, ~even])
    bound = (K + 2) * U * (ref["gx_bound"] / ((K + 1) * U) + gx_m.to(F64).abs())
    share_x = _share(xr.grad[:, :, even], (gx_m.to(F64) + ref["gx"])[:, :, even], bound[:, :, even])
    print("block_entry: largest error / bound: grad_x %.4f, grad_w1 %.4f" % (share_x, share_w))

    # the shortcut's forward and weight gradient left to MIOpen: their bits are MIOpen's
    xr, w3r, w1r = (t.clone().requires_grad_(True) for t in (x, w3, w1))
    y3, y1 = ops.block_entry(xr, w3r, w1r, fwd=False, wgrad=False)
    torch.autograd.backward([y3, y1], [g3, g1])
    assert torch.equal(y1, F.conv2d(x, w1, None, 2)) and torch.equal(w1r.grad, _miopen_backward(g1, x, w1, 2, 0)[1])
    assert torch.equal(y3, y3_m) and torch.equal(w3r.grad, gw3_m)


def _encoder_run(enc, image):
    for p in enc.parameters():
        p.grad = None
    feats = enc(image)
    sum((f * (i + 1.0)).sum() for i, f in enumerate(feats)).backward()
    res = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    res.update({"feature %d" % i: f.detach().clone() for i, f in enumerate(feats)})
    return res


def test_encoder_with_the_routes_on_and_off(monkeypatch):
    """One ResnetEncoder(18) at 64 x 128, batch 2, with that size's shortcut rows in the table: the new entry points run
    three times each way, and no feature and no parameter gradient is further from a float64 run of the same module than
    twice the distance of MIOpen's own path (the switch off) - `of the size MIOpen's path is`; the reference is the
    float64 module, MIOpen's figure is printed beside ours.  Unpatched, none of the new entry points is launched."""
    ops, _ = _ops()
    _deterministic_convolutions(monkeypatch)
    from baseboostdepth_amd import networks
    backend = ops.default_backend()
    names = []
    real = backend.run
    monkeypatch.setattr(backend, "run", lambda name, *a: (names.append(name), real(name, *a))[1])
    torch.manual_seed(5)
    enc = networks.ResnetEncoder(18, False).to(DEV).train()
    image = torch.rand(2, 3, 64, 128, device=DEV)

    unpatched = _encoder_run(enc, image)
    assert not [n for n in names if "conv1x1s2" in n]
    rows = {(C, 2 * C, H, W, d) for C, H, W in ((64, 16, 32), (128, 8, 16), (256, 4, 8)) for d in ("fwd", "dgrad", "wgrad")}
    monkeypatch.setattr(ops, "CONV1X1_ROUTES", rows)
    monkeypatch.setattr(ops, "BLOCK_ENTRY_ROUTES", {row[:4] for row in rows})
    del names[:]
    on = _encoder_run(enc, image)
    for entry in ("bbd_conv1x1s2_fwd", "bbd_conv1x1s2_bwd_data", "bbd_conv1x1s2_wgrad"):
        assert names.count(entry) == 3, (entry, names.count(entry))
    monkeypatch.setattr(ops, "BLOCK_ENTRY_ROUTES", set())                                       # without the joint entry
    del names[:]
    separate = _encoder_run(enc, image)
    assert [names.count("bbd_conv1x1s2_" + d) for d in ("fwd", "bwd_data", "wgrad")] == [3, 3, 3]
    monkeypatch.setattr(ops, "BLOCK_ENTRY_ROUTES", {row[:4] for row in rows})
    monkeypatch.setattr(ops, "FUSED_CONV1X1", False)
    del names[:]
    off = _encoder_run(enc, image)
    assert not [n for n in names if "conv1x1s2" in n]
    assert sorted(off) == sorted(unpatched) and all(torch.equal(off[n], unpatched[n]) for n in off)
    enc64 = networks.ResnetEncoder(18, False).to(DEV).double().train()
    enc64.load_state_dict(enc.state_dict())
    ref = _encoder_run(enc64, image.double())
    del enc, enc64

    assert sorted(on) == sorted(off) == sorted(separate) == sorted(ref)
    worst = []
    for name in sorted(on):
        e_on = float((on[name].to(F64) - ref[name]).abs().max())
        e_sep = float((separate[name].to(F64) - ref[name]).abs().max())
        e_off = float((off[name].to(F64) - ref[name]).abs().max())
        print("%-44s error against float64: routes on %.3e, without the joint entry %.3e, MIOpen %.3e" % (name, e_on, e_sep, e_off))
        if max(e_on, e_sep) > 2.0 * e_off:
            worst.append((name, e_on, e_sep, e_off))
    assert not worst, worst
