"""GPU tier: the encoder stems' conv1 - 7x7, stride 2, pad 3, C = 3 or 6 -> 64 - and its weight gradient on fp32 MFMA
(ops.stem_conv_fwd / stem_conv_wgrad / stem_conv, csrc/bbd_stemconv.hip) against float64 on the device,

    F.conv2d(x, w, None, 2, 3)        and its autograd weight gradient for a random grad_out.

The ops are called directly, not through ops.STEMCONV_ROUTES.  The bounds are derived, not tuned (include/bbd_hip.h):

    forward   |out - out64| <= (P + 1) * 2^-24 * sum |x| |w|, P = the tap count padded to a multiple of 4 (148 or 296):
              the MFMA is an fma chain of P products
    grad_w    |gw - gw64|   <= (BBD_WGRAD_RUN + 1) * 2^-24 * sum |grad_out| |x|: fp32 runs of BBD_WGRAD_RUN products, then
              float64

With `normalize` the float64 reference takes the fp32 normalised image, and a case of its own asks the kernel's normalised
values to have the bits of the torch ops.  The kernels' tile is BBD_STEM_TH x BBD_STEM_TW output pixels (read from
csrc/bbd_stemconv_math.h)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "baseboostdepth_amd", "csrc", "bbd_stemconv_math.h")) as _f:
    _TEXT = _f.read()
TH = int(re.search(r"#define BBD_STEM_TH (\d+)", _TEXT).group(1))
TW = int(re.search(r"#define BBD_STEM_TW (\d+)", _TEXT).group(1))

#         N  C  H            W
SHAPES = [(1, 3, 2, 2),                      # one output pixel, almost every tap in the padding
          (1, 6, 7, 9),                      # odd sizes, Ho * 2 != H
          (2, 3, 5, 33),
          (2, 6, 2 * TH, 2 * TW + 2),        # exactly a tile in H, a tile plus one column in W
          (3, 6, 2 * TH + 1, 2 * TW - 1),    # the same edges with odd sizes
          (2, 3, 32, 64)]
KINDS = ["wide", "mean100", "zeros"]
CASES = [shape + (kind,) for shape in SHAPES for kind in KINDS]


def _ops():
    from baseboostdepth_amd import ops, _lib
    return ops, _lib


def _inputs(case):
    N, C, H, W, kind = case
    gen = torch.Generator().manual_seed(100000 * N + 10000 * C + 100 * H + W)
    x = torch.randn(N, C, H, W, generator=gen)
    if kind == "wide":
        x = 3.0 * x
    elif kind == "mean100":
        x = 100.0 + x                                            # cancellation
    else:
        x = x * (torch.rand(N, C, H, W, generator=gen) > 0.7)    # many exact zeros
    w = 0.2 * torch.randn(64, C, 7, 7, generator=gen)
    gout = torch.randn(N, 64, (H + 1) // 2, (W + 1) // 2, generator=gen)
    if kind == "zeros":
        gout = gout * (torch.rand(gout.shape, generator=gen) > 0.7)
    return x.to(DEV), w.to(DEV), gout.to(DEV)


def _conv64(x, w):
    return F.conv2d(x.to(F64), w.to(F64), None, 2, 3)


_REFERENCE = {}


def _reference(case, normalize):
    """float64 forward, weight gradient and both bounds of a case: computed once, shared, left unchanged"""
    key = case + (normalize,)
    if key not in _REFERENCE:
        _, _lib = _ops()
        x, w, gout = _inputs(case)
        xn = (x - 0.45) / 0.225 if normalize else x              # the fp32 normalised image
        w64 = w.to(F64).requires_grad_(True)
        out64 = _conv64(xn, w64)
        out64.backward(gout.to(F64))
        u = 2.0 ** -24
        P = 4 * ((case[1] * 49 + 3) // 4)
        fwd_bound = (P + 1) * u * _conv64(xn.abs(), w.abs())
        a64 = torch.zeros_like(w64).requires_grad_(True)
        _conv64(xn.abs(), a64).backward(gout.to(F64).abs())
        gw_bound = (_lib.WGRAD_RUN + 1) * u * a64.grad
        _REFERENCE[key] = (out64.detach(), w64.grad.detach(), fwd_bound, gw_bound)
    return _REFERENCE[key]


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_C%d_H%d_W%d_%s" % c)
def test_forward_and_weight_gradient_against_float64(case, normalize):
    ops, _lib = _ops()
    N, C, H, W, _ = case
    backend = ops.default_backend()
    assert backend.lib.stem_conv7s2_supported(N, C, 64, H, W, 7, 7) == 1
    assert 4 * ((C * 49 + 3) // 4) == {3: 148, 6: 296}[C] and _lib.WGRAD_RUN == 128
    x, w, gout = _inputs(case)
    out64, gw64, fwd_bound, gw_bound = _reference(case, normalize)
    keep = x.clone()

    out = ops.stem_conv_fwd(x, w, normalize)
    gw = ops.stem_conv_wgrad(x, w, gout, normalize)
    assert out.shape == out64.shape and out.dtype == F32 and gw.shape == w.shape and gw.dtype == F32 and torch.equal(x, keep)
    e_out, e_gw = (out.to(F64) - out64).abs(), (gw.to(F64) - gw64).abs()
    print("N%d C%d H%d W%d %s normalize %d: largest error / bound: forward %.4f, grad_w %.4f"
          % (case + (normalize, _ratio(e_out, fwd_bound), _ratio(e_gw, gw_bound))))
    assert bool((e_out <= fwd_bound).all())
    assert bool((e_gw <= gw_bound).all())

    # equal bits from a second launch, and from one whose outputs and scratch were NaN before
    run, ptr = backend.run, _lib.ptr
    doubles = backend.lib.stem_conv7s2_wgrad_scratch_doubles(N, C, 64, H, W, 7, 7)
    assert doubles > 0
    for _ in range(2):
        out2, gw2 = torch.full_like(out, float("nan")), torch.full_like(gw, float("nan"))
        scratch = torch.full((doubles,), float("nan"), device=DEV, dtype=F64)
        run("bbd_stem_conv7s2_fwd", x, ptr(x), ptr(w), ptr(out2), N, C, 64, H, W, int(normalize))
        run("bbd_stem_conv7s2_wgrad", x, ptr(x), ptr(gout), ptr(gw2), ptr(scratch), doubles, N, C, 64, H, W, int(normalize))
        assert torch.equal(out2, out) and torch.equal(gw2, gw)
        assert not bool(torch.isnan(scratch).any())              # every record element is written


def test_the_folded_normalisation_has_the_bits_of_the_torch_ops():
    """A weight that picks single pixels (tap (3, 3) of channel c for output channel c, stride 2: the even pixels; tap
    (4, 4): the odd ones) returns the kernel's normalised image: it must equal `(x - 0.45) / 0.225` as torch evaluates it."""
    ops, _ = _ops()
    gen = torch.Generator().manual_seed(11)
    x = (torch.round(torch.rand(2, 6, 18, 70, generator=gen) * 255) / 255).to(DEV)
    x[1, :, 4:9] = 0.0
    want = (x - 0.45) / 0.225
    for tap in (3, 4):
        w = torch.zeros(64, 6, 7, 7, device=DEV)
        for c in range(6):
            w[c, c, tap, tap] = 1.0
        got = ops.stem_conv_fwd(x, w, True)[:, :6]
        assert torch.equal(got, want[:, :, tap - 3::2, tap - 3::2])
        assert torch.equal(ops.stem_conv_fwd(x, w, False)[:, :6], x[:, :, tap - 3::2, tap - 3::2])


def test_refused_shapes_reach_miopen_through_the_module(monkeypatch):
    ops, _lib = _ops()
    lib = ops.default_backend().lib
    # N, C, K, H, W, R, S
    refused = [(2, 3, 32, 8, 8, 7, 7), (2, 3, 128, 8, 8, 7, 7), (2, 4, 64, 8, 8, 7, 7), (2, 1, 64, 8, 8, 7, 7),
               (2, 12, 64, 8, 8, 7, 7), (2, 3, 64, 8, 8, 3, 3), (2, 3, 64, 8, 8, 7, 5), (2, 3, 64, 8, 8, 5, 7),
               (0, 3, 64, 8, 8, 7, 7), (2, 3, 64, 0, 8, 7, 7), (2, 3, 64, 8, 0, 7, 7), (1 << 20, 6, 64, 192, 640, 7, 7)]
    for shape in refused:
        assert lib.stem_conv7s2_supported(*shape) == 0 and lib.stem_conv7s2_wgrad_scratch_doubles(*shape) == 0, shape
    t = torch.zeros(4096, device=DEV)
    s = torch.zeros(4096, device=DEV, dtype=F64)
    p = _lib.ptr(t)
    for N, C, K, H, W, R, S in refused:
        if (R, S) == (7, 7):
            assert lib._dll.bbd_stem_conv7s2_fwd(p, p, p, N, C, K, H, W, 0, lib.stream_for(t)) == _lib.E_BADARG
            assert lib._dll.bbd_stem_conv7s2_wgrad(p, p, p, _lib.ptr(s), 1 << 30, N, C, K, H, W, 0, lib.stream_for(t)) == _lib.E_BADARG
    small = lib.stem_conv7s2_wgrad_scratch_doubles(1, 3, 64, 2, 2, 7, 7)
    assert lib._dll.bbd_stem_conv7s2_wgrad(p, p, p, _lib.ptr(s), small - 1, 1, 3, 64, 2, 2, 0, lib.stream_for(t)) == _lib.E_BADARG
    with pytest.raises(_lib.BbdError):
        ops.stem_conv_fwd(torch.zeros(1, 4, 8, 8, device=DEV), torch.zeros(64, 4, 7, 7, device=DEV))
    with pytest.raises(_lib.BbdError):
        ops.stem_conv_fwd(torch.zeros(1, 3, 8, 8, device=DEV), torch.zeros(32, 3, 7, 7, device=DEV))
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(s.any())               # nothing was launched

    # the predicate refuses them even when the table holds their row, so a module with such a conv1 keeps MIOpen
    monkeypatch.setattr(ops, "STEMCONV_ROUTES", {(C, H, H, d) for C in (1, 3, 4, 6, 12) for H in (8, 32) for d in ("fwd", "wgrad")})
    x3 = torch.zeros(2, 3, 8, 8, device=DEV)
    assert ops.stem_conv_routed(x3, torch.zeros(64, 3, 7, 7, device=DEV), "fwd")
    assert not ops.stem_conv_routed(x3, torch.zeros(32, 3, 7, 7, device=DEV), "fwd")
    assert not ops.stem_conv_routed(x3, torch.zeros(64, 3, 3, 3, device=DEV), "wgrad")
    assert not ops.stem_conv_routed(torch.zeros(2, 4, 8, 8, device=DEV), torch.zeros(64, 4, 7, 7, device=DEV), "fwd")
    assert not ops.stem_conv_routed(torch.zeros(0, 3, 8, 8, device=DEV), torch.zeros(64, 3, 7, 7, device=DEV), "fwd")
    assert not ops.stem_conv_routed(x3.half(), torch.zeros(64, 3, 7, 7, device=DEV).half(), "fwd")
    assert not ops.stem_conv_routed(torch.zeros(2, 3, 8, 16, device=DEV)[..., ::2], torch.zeros(64, 3, 7, 7, device=DEV), "fwd")
    from baseboostdepth_amd import networks
    backend = ops.default_backend()
    names = []
    real = backend.run
    monkeypatch.setattr(backend, "run", lambda name, *a: (names.append(name), real(name, *a))[1])
    torch.manual_seed(2)
    enc = networks.ResnetEncoder(18, False, 4).to(DEV).train()                # conv1 with 12 input channels
    feats = enc(torch.rand(2, 12, 32, 32, device=DEV))
    sum(f.sum() for f in feats).backward()
    assert enc.encoder.conv1.weight.grad is not None and not [n for n in names if n.startswith("bbd_stem_conv7s2")]


def _deterministic_convolutions(monkeypatch):
    """as tests/test_gpu_conv_wgrad.py: MIOpen's solvers that add with atomics are not chosen, so today's path repeats"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def _encoder_run(enc, image):
    for p in enc.parameters():
        p.grad = None
    feats = enc(image)
    sum((f * (i + 1.0)).sum() for i, f in enumerate(feats)).backward()
    res = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    res.update({"feature %d" % i: f.detach().clone() for i, f in enumerate(feats)})
    return res


@pytest.mark.parametrize("images", [1, 2])
def test_encoder_with_the_routes_on_and_off(monkeypatch, images):
    """One ResnetEncoder(18) at 64 x 128, batch 2, its conv1 routed in both directions: no feature and no parameter gradient
    is further from a float64 run of the same module than twice the switched-off path's distance; with the weight gradient
    alone routed, everything but conv1's weight gradient has the bits of the switched-off path."""
    ops, _ = _ops()
    _deterministic_convolutions(monkeypatch)
    from baseboostdepth_amd import networks
    C = 3 * images
    backend = ops.default_backend()
    names = []
    real = backend.run
    monkeypatch.setattr(backend, "run", lambda name, *a: (names.append(name), real(name, *a))[1])
    torch.manual_seed(5)
    enc = networks.ResnetEncoder(18, False, images).to(DEV).train()
    image = torch.rand(2, C, 64, 128, device=DEV)
    both = {(C, 64, 128, "fwd"), (C, 64, 128, "wgrad")}

    monkeypatch.setattr(ops, "STEMCONV_ROUTES", both)
    del names[:]
    on = _encoder_run(enc, image)
    assert names.count("bbd_stem_conv7s2_fwd") == 1 and names.count("bbd_stem_conv7s2_wgrad") == 1
    monkeypatch.setattr(ops, "STEMCONV_ROUTES", {(C, 64, 128, "wgrad")})
    del names[:]
    wgrad_only = _encoder_run(enc, image)
    assert names.count("bbd_stem_conv7s2_fwd") == 0 and names.count("bbd_stem_conv7s2_wgrad") == 1
    monkeypatch.setattr(ops, "STEMCONV_ROUTES", both)
    monkeypatch.setattr(ops, "FUSED_STEMCONV", False)
    del names[:]
    off = _encoder_run(enc, image)
    assert not [n for n in names if n.startswith("bbd_stem_conv7s2")]
    enc64 = networks.ResnetEncoder(18, False, images).to(DEV).double().train()
    enc64.load_state_dict(enc.state_dict())
    ref = _encoder_run(enc64, image.double())
    del enc, enc64

    assert sorted(on) == sorted(off) == sorted(wgrad_only) == sorted(ref)
    for name in off:
        if name != "encoder.conv1.weight":
            assert torch.equal(wgrad_only[name], off[name]), name
    worst = []
    for name in sorted(on):
        e_on = float((on[name].to(F64) - ref[name]).abs().max())
        e_off = float((off[name].to(F64) - ref[name]).abs().max())
        print("%-44s error against float64: routes on %.3e, off %.3e" % (name, e_on, e_off))
        if e_on > 2.0 * e_off:
            worst.append((name, e_on, e_off))
    e_w = float((wgrad_only["encoder.conv1.weight"].to(F64) - ref["encoder.conv1.weight"]).abs().max())
    e_off = float((off["encoder.conv1.weight"].to(F64) - ref["encoder.conv1.weight"]).abs().max())
    print("conv1 weight gradient alone routed: error %.3e, off %.3e" % (e_w, e_off))
    assert e_w <= 2.0 * e_off
    assert not worst, worst
