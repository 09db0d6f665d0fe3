"""GPU tier: the finest decoder level's up-sample + pad + 3x3 convolution in sub-pixel form (ops.up2_conv3x3,
csrc/bbd_up2conv.hip) against the composition in float64 on the device,

    F.conv2d(F.pad(F.interpolate(F.elu(z + b), scale_factor=2), (1, 1, 1, 1), mode="reflect"), w)

and its autograd gradients for a random grad_out.  The bounds are derived, not tuned (include/bbd_hip.h):

    forward    |out - out64| <= c * 2^-24 * S, c = BBD_UP2CONV_ROUNDINGS (<= 152), S the same expression on |ELU(z + b)|, |w|
    grad_z     |gz - gz64|   <= (n + 4) * 2^-24 * S', S' the float64 adjoint on absolute values, n the number of products
               that reach the element (the adjoint on all-ones tensors; border elements receive more)
    grad_bias  within the sum of its elements' grad_z bounds plus one rounding

The forward tile of the kernel is 8 source rows x 32 source columns (BBD_UP2CONV_TR x BBD_UP2CONV_TC), a backward strip 16
source pixels of one row; the case 9 x 33 is one source pixel larger than the tile in each direction."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
TILE = (8, 32)

#        N  h   w   input
CASES = [(1, 1, 1, "wide"),          # every tap clamps
         (1, 1, 2, "wide"),
         (2, 2, 3, "wide"),          # odd sizes, both parities at both borders
         (1, 3, 17, "wide"),         # one pixel past a 16-pixel MFMA block
         (2, 5, 33, "mean100"),      # z = 100 + randn
         (2, 17, 40, "saturated"),   # z = -6 + randn: ELU' about e^-6
         (1, TILE[0] + 1, TILE[1] + 1, "wide")]


def _ops():
    from baseboostdepth_amd import ops, _lib
    return ops, _lib


def _inputs(case):
    N, h, w, kind = case
    gen = torch.Generator().manual_seed(10000 * N + 100 * h + w)
    z = torch.randn(N, 16, h, w, generator=gen)
    z = {"wide": 3.0 * z, "mean100": 100.0 + z, "saturated": z - 6.0}[kind]
    bias = 0.5 * torch.randn(16, generator=gen)
    weight = 0.2 * torch.randn(16, 16, 3, 3, generator=gen)
    gout = torch.randn(N, 16, 2 * h, 2 * w, generator=gen)
    return z.to(DEV), bias.to(DEV), weight.to(DEV), gout.to(DEV)


def _up_pad_conv(y, w):
    return F.conv2d(F.pad(F.interpolate(y, scale_factor=2, mode="nearest"), (1, 1, 1, 1), mode="reflect"), w)


def _adjoint64(y_like, w, gout):
    """gradient of _up_pad_conv with respect to its input, in float64"""
    y = torch.zeros_like(y_like, dtype=F64).requires_grad_(True)
    _up_pad_conv(y, w.to(F64)).backward(gout.to(F64))
    return y.grad


_REFERENCE = {}


def _reference(case):
    """float64 forward, gradients and bounds of a case: computed once, shared, left unchanged"""
    if case not in _REFERENCE:
        _, _lib = _ops()
        z, bias, weight, gout = _inputs(case)
        z64 = z.to(F64).requires_grad_(True)
        b64 = bias.to(F64).requires_grad_(True)
        w64 = weight.to(F64).requires_grad_(True)
        y64 = F.elu(z64 + b64.view(1, -1, 1, 1))
        out64 = _up_pad_conv(y64, w64)
        out64.backward(gout.to(F64))
        u = 2.0 ** -24
        fwd_bound = _lib.UP2CONV_ROUNDINGS * u * _up_pad_conv(y64.detach().abs(), weight.to(F64).abs())
        v = (z64 + b64.view(1, -1, 1, 1)).detach()
        elu_grad = torch.where(v > 0, torch.ones_like(v), torch.exp(v))
        n = _adjoint64(z, torch.ones_like(weight), torch.ones_like(gout))
        gz_bound = (n + 4) * u * _adjoint64(z, weight.abs(), gout.abs()) * elu_grad
        gb_bound = gz_bound.sum((0, 2, 3)) + u * b64.grad.abs()
        _REFERENCE[case] = tuple(t.detach() for t in (out64, z64.grad, b64.grad, w64.grad, fwd_bound, gz_bound, gb_bound))
    return _REFERENCE[case]


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_h%d_w%d_%s" % c)
def test_forward_and_gradients_against_float64(case):
    ops, _lib = _ops()
    assert _lib.UP2CONV_ROUNDINGS <= 152
    N, h, w, _ = case
    backend = ops.default_backend()
    assert backend.lib.up2conv3x3_supported(N, 16, 16, h, w) == 1
    z, bias, weight, gout = _inputs(case)
    out64, gz64, gb64, _, fwd_bound, gz_bound, gb_bound = _reference(case)

    zz, bb = z.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    out = ops.up2_conv3x3(zz, bb, weight)
    assert out.shape == (N, 16, 2 * h, 2 * w) and out.dtype == F32 and torch.equal(zz.detach(), z)
    out.backward(gout)
    gz, gb = zz.grad, bb.grad
    e_out, e_gz, e_gb = (out.detach().to(F64) - out64).abs(), (gz.to(F64) - gz64).abs(), (gb.to(F64) - gb64).abs()
    print("N%d h%d w%d %s: largest error / bound: forward %.4f, grad_z %.4f, grad_bias %.4f"
          % (case + (_ratio(e_out, fwd_bound), _ratio(e_gz, gz_bound), _ratio(e_gb, gb_bound))))
    assert bool((e_out <= fwd_bound).all())
    assert bool((e_gz <= gz_bound).all())
    assert bool((e_gb <= gb_bound).all())

    # equal bits from a second launch, and from one whose outputs and scratch were NaN before
    run, ptr = backend.run, _lib.ptr
    doubles = backend.lib.up2conv3x3_scratch_doubles(N, 16, 16, h, w)
    assert doubles == 16 * N * h
    for _ in range(2):
        out2 = torch.full_like(out, float("nan"))
        gz2, gb2 = torch.full_like(gz, float("nan")), torch.full_like(gb, float("nan"))
        scratch = torch.full((doubles,), float("nan"), device=DEV, dtype=F64)
        run("bbd_up2conv3x3_fwd", z, ptr(z), ptr(bias), ptr(weight), ptr(out2), N, 16, 16, h, w)
        run("bbd_up2conv3x3_bwd", gout, ptr(gout), ptr(z), ptr(bias), ptr(weight), ptr(gz2), ptr(gb2), ptr(scratch), doubles,
            N, 16, 16, h, w)
        assert torch.equal(out2, out.detach()) and torch.equal(gz2, gz) and torch.equal(gb2, gb)
        assert not bool(torch.isnan(scratch).any())


def test_supported_says_no_and_the_calls_refuse():
    ops, _lib = _ops()
    backend = ops.default_backend()
    lib = backend.lib
    t = torch.zeros(4096, device=DEV)
    s = torch.zeros(4096, device=DEV, dtype=F64)
    for N, C, K, h, w in ((1, 24, 16, 4, 4), (1, 16, 8, 4, 4), (1, 16, 16, 0, 4), (1, 16, 16, 4, 0), (0, 16, 16, 4, 4)):
        assert lib.up2conv3x3_supported(N, C, K, h, w) == 0 and lib.up2conv3x3_scratch_doubles(N, C, K, h, w) == 0
        p = _lib.ptr(t)
        assert lib._dll.bbd_up2conv3x3_fwd(p, p, p, p, N, C, K, h, w, lib.stream_for(t)) == _lib.E_BADARG
        assert lib._dll.bbd_up2conv3x3_bwd(p, p, p, p, p, p, _lib.ptr(s), 4096, N, C, K, h, w, lib.stream_for(t)) == _lib.E_BADARG
    # a scratch that is too small
    p = _lib.ptr(t)
    assert lib._dll.bbd_up2conv3x3_bwd(p, p, p, p, p, p, _lib.ptr(s), 31, 1, 16, 16, 2, 2, lib.stream_for(t)) == _lib.E_BADARG
    with pytest.raises(_lib.BbdError):
        ops.up2_conv3x3(torch.zeros(1, 24, 4, 4, device=DEV), torch.zeros(24, device=DEV), torch.zeros(16, 24, 3, 3, device=DEV))
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(s.any())             # nothing was launched


def _deterministic_convolutions(monkeypatch):
    """as tests/test_gpu_conv_wgrad.py: MIOpen's solvers that add with atomics are not chosen, so today's path repeats"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def _composition(z, bias, weight, gout):
    """today's line of the decoder and its gradients"""
    from baseboostdepth_amd import layers, ops
    block = layers.ConvBlock(16, 16).to(DEV)
    block.conv.conv.weight = torch.nn.Parameter(weight.clone())
    zz, bb = z.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    out = block.conv_raw(ops.upcat_pad_act(zz, bb, None))
    out.backward(gout)
    return out.detach(), zz.grad, bb.grad, block.conv.conv.weight.grad


@pytest.mark.parametrize("wgrad_routed", [False, True], ids=["miopen", "bbd_wgrad"])
def test_weight_gradient_has_the_bits_of_the_composition(monkeypatch, wgrad_routed):
    ops, _lib = _ops()
    _deterministic_convolutions(monkeypatch)
    case = CASES[5]
    N, h, w, _ = case
    if wgrad_routed:
        monkeypatch.setattr(ops, "WGRAD_ROUTES", set(ops.WGRAD_ROUTES) | {(16, 16, 2 * h, 2 * w)})
    z, bias, weight, gout = _inputs(case)
    assert ops.conv3x3_wgrad_routed(torch.empty(N, 16, 2 * h + 2, 2 * w + 2, device=DEV), weight) == (wgrad_routed and ops.FUSED_WGRAD)
    _, _, _, want = _composition(z, bias, weight, gout)
    ww = weight.clone().requires_grad_(True)
    ops.up2_conv3x3(z, bias, ww).backward(gout)                  # z and bias ask for no gradient: the data launch is skipped
    assert torch.equal(ww.grad, want)
    gw64 = _reference(case)[3]
    print("weight gradient, %s: max |error| %.3e of max |gradient| %.3e"
          % ("bbd_conv3x3_wgrad" if wgrad_routed else "MIOpen", float((ww.grad.to(F64) - gw64).abs().max()), float(gw64.abs().max())))


def _decoder_run(module, inputs):
    xs = [t.clone().requires_grad_(True) for t in inputs]
    for p in module.parameters():
        p.grad = None
    out = module(xs)
    sum((out[("disp", s)] * (s + 1.0)).sum() for s in range(4)).backward()
    res = {n: p.grad.clone() for n, p in module.named_parameters()}
    res.update({"disp %d" % s: out[("disp", s)].detach().clone() for s in range(4)})
    res.update({"feature %d" % i: t.grad for i, t in enumerate(xs)})
    return res


def _decoder(dtype=F32):
    from baseboostdepth_amd import networks
    torch.manual_seed(3)
    enc = [64, 64, 128, 256, 512]
    dec = networks.DepthDecoder(enc, [0, 1, 2, 3]).to(DEV).train()
    feats = [torch.randn(2, c, 32 >> i, 64 >> i, device=DEV) for i, c in enumerate(enc)]
    return enc, dec, feats


LEVEL0 = (16, 16, 32, 64)           # (C, K, h, w) of level 0 of a DepthDecoder at a 64 x 128 image


def test_routing_and_the_switches(monkeypatch):
    """An unrouted shape, a strided or fp16 input and each of the three switches take today's path and give today's bits;
    a routed pair launches the new entry points, one forward and one backward."""
    ops, _lib = _ops()
    _deterministic_convolutions(monkeypatch)
    backend = ops.default_backend()
    names = []
    real = backend.run
    monkeypatch.setattr(backend, "run", lambda name, *a: (names.append(name), real(name, *a))[1])
    new = {"bbd_up2conv3x3_fwd", "bbd_up2conv3x3_bwd"}

    z = torch.randn(2, 16, 32, 64, device=DEV)
    bias, weight = torch.randn(16, device=DEV), torch.randn(16, 16, 3, 3, device=DEV)
    assert not ops.up2_conv3x3_routed(z, bias, weight)                                   # supported, not measured
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", {LEVEL0, (24, 16, 32, 64)})
    assert ops.up2_conv3x3_routed(z, bias, weight)
    assert not ops.up2_conv3x3_routed(z[:, :, :, :32], bias, weight)                      # unrouted shape
    assert not ops.up2_conv3x3_routed(torch.randn(2, 16, 32, 128, device=DEV)[..., ::2], bias, weight)      # strided
    assert not ops.up2_conv3x3_routed(z.half(), bias.half(), weight.half())              # fp16
    assert not ops.up2_conv3x3_routed(z, None, weight)
    assert not ops.up2_conv3x3_routed(torch.randn(2, 24, 32, 64, device=DEV), torch.randn(24, device=DEV),
                                      torch.randn(16, 24, 3, 3, device=DEV))              # in the table, not supported

    enc, dec, feats = _decoder()
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", set())
    del names[:]
    today = _decoder_run(dec, feats)                                                     # unrouted: today's path
    assert not new & set(names)
    copies = (names.count("bbd_upcat_pad_act_fwd"), names.count("bbd_upcat_pad_act_bwd"))
    assert copies == (5, 5)                                                              # one pair per decoder level
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", {LEVEL0})
    del names[:]
    _decoder_run(dec, feats)
    assert names.count("bbd_up2conv3x3_fwd") == 1 and names.count("bbd_up2conv3x3_bwd") == 1
    # the copy is made once, in the backward, for the weight gradient; the composition's backward launch is gone
    assert (names.count("bbd_upcat_pad_act_fwd"), names.count("bbd_upcat_pad_act_bwd")) == (5, 4)
    for switch in ("FUSED_UP2CONV", "FUSED_DECODER_GLUE", "FUSED_NN"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            del names[:]
            got = _decoder_run(dec, feats)
            assert not new & set(names), switch
            if switch == "FUSED_UP2CONV":
                for name in today:
                    assert torch.equal(got[name], today[name]), name
    del dec


def test_depth_decoder_with_the_switch_on_and_off(monkeypatch):
    """One DepthDecoder at a 64 x 128 image, batch 2, level 0 routed: disparities 1..3 have equal bits with the switch on
    and off; disparity 0 and every gradient are no further from a float64 run of the same module than twice the
    switched-off path's distance (the two sides differ in the rounding order of one layer only)."""
    ops, _lib = _ops()
    _deterministic_convolutions(monkeypatch)
    from baseboostdepth_amd import networks
    enc, dec, feats = _decoder()
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", {LEVEL0})
    on = _decoder_run(dec, feats)
    monkeypatch.setattr(ops, "FUSED_UP2CONV", False)
    off = _decoder_run(dec, feats)
    dec64 = networks.DepthDecoder(enc, [0, 1, 2, 3]).to(DEV).double().train()
    dec64.load_state_dict(dec.state_dict())
    ref = _decoder_run(dec64, [t.double() for t in feats])
    del dec, dec64
    for s in (1, 2, 3):
        assert torch.equal(on["disp %d" % s], off["disp %d" % s])
    worst = []
    for name in sorted(on):
        e_on = float((on[name].to(F64) - ref[name]).abs().max())
        e_off = float((off[name].to(F64) - ref[name]).abs().max())
        print("%-32s error against float64: switch on %.3e, off %.3e" % (name, e_on, e_off))
        if e_on > 2.0 * e_off:
            worst.append((name, e_on, e_off))
    assert not worst, worst
