"""GPU tier: the ConvBlock weight gradient from the NCHW tensors (ops.conv3x3_wgrad, csrc/bbd_wgrad.hip) against the
float64 weight gradient of F.conv2d, computed in double on the device.

The bound is derived, not tuned (include/bbd_hip.h): every fp32 accumulator is an fma chain of at most R = BBD_WGRAD_RUN
products before it is widened, everything after that is float64 and one last rounding to fp32, so element by element

    |dw - dw64| <= (R + 1) * 2^-24 * S,    S = sum |grad_z| |xp|  (the same gradient on the absolute values, in float64).

Each case also asks for equal bits from two launches and from a launch whose scratch blocks were NaN before."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64

#        K   C   N  H   W    large mean
CASES = [(16, 16, 1, 1, 4, False),       # one partial strip
         (16, 16, 2, 3, 16, False),      # exactly one strip per row
         (16, 16, 1, 2, 18, False),      # tail of 2, rows not 16-byte aligned
         (16, 32, 3, 5, 36, False),      # two channel blocks, odd rows
         (32, 64, 2, 4, 40, False),      # the upconv(1,0) form: 4 roles
         (32, 96, 1, 6, 20, False),      # the upconv(1,1) form: 6 roles
         (16, 16, 2, 48, 160, False),    # 10 workgroups, two fp32 runs per wave: the partial reduction
         (16, 32, 2, 7, 50, True)]       # xp = 100 + noise


def _ops():
    from baseboostdepth_amd import ops, _lib
    return ops, _lib


def _wgrad64(xp, gz, K):
    """weight gradient of F.conv2d(xp, w) for the upstream gradient gz, in float64 on the device"""
    w = torch.zeros(K, xp.shape[1], 3, 3, device=xp.device, dtype=F64, requires_grad=True)
    F.conv2d(xp.to(F64), w, None).backward(gz.to(F64))
    return w.grad


def _bound(xp, gz, K, run):
    return (run + 1) * 2.0 ** -24 * _wgrad64(xp.abs(), gz.abs(), K)


def _inputs(case):
    K, C, N, H, W, large = case
    gen = torch.Generator().manual_seed(1000 * K + 100 * C + 10 * H + W)
    xp = torch.randn(N, C, H + 2, W + 2, generator=gen)
    if large:
        xp = xp + 100.0
    return xp.to(DEV), torch.randn(N, K, H, W, generator=gen).to(DEV)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "K%d_C%d_N%d_H%d_W%d%s" % (c[:5] + ("_mean100" if c[5] else "",)))
def test_weight_gradient_against_float64(case):
    ops, _lib = _ops()
    K, C, N, H, W, _ = case
    lib = ops.default_backend().lib
    assert lib.conv3x3_wgrad_supported(N, C, K, H, W) == 1
    xp, gz = _inputs(case)
    ref, bound = _wgrad64(xp, gz, K), _bound(xp, gz, K, _lib.WGRAD_RUN)
    got = ops.conv3x3_wgrad(xp, gz)
    assert got.shape == (K, C, 3, 3) and got.dtype == F32
    err = (got.to(F64) - ref).abs()
    print("K%d C%d N%d H%d W%d: max error / bound %.4f, max error / S %.3e"
          % (K, C, N, H, W, float((err / bound).max()), float((err / (bound / ((_lib.WGRAD_RUN + 1) * 2.0 ** -24))).max())))
    assert bool((err <= bound).all())
    # the same bits again, and with NaN in every block the allocator hands the scratch from
    again = ops.conv3x3_wgrad(xp, gz)
    assert torch.equal(got, again)
    del again
    doubles = lib.conv3x3_wgrad_scratch_doubles(N, C, K, H, W)
    assert doubles >= 9 * C * K
    poison = [torch.full((doubles,), float("nan"), device=DEV, dtype=F64) for _ in range(2)]
    torch.cuda.synchronize()
    del poison                                                   # back to the caching allocator, still NaN
    third = ops.conv3x3_wgrad(xp, gz)
    assert torch.equal(got, third)
    # and through the C ABI with a scratch that IS NaN
    scratch = torch.full((doubles,), float("nan"), device=DEV, dtype=F64)
    fourth = torch.empty_like(got)
    ops.default_backend().run("bbd_conv3x3_wgrad", xp, _lib.ptr(xp), _lib.ptr(gz), _lib.ptr(fourth), _lib.ptr(scratch),
                              N, C, K, H, W)
    assert torch.equal(got, fourth) and not bool(torch.isnan(scratch).any())


def test_supported_says_no_and_the_call_refuses():
    ops, _lib = _ops()
    lib = ops.default_backend().lib
    for N, C, K, H, W in ((1, 24, 16, 4, 4), (1, 16, 8, 4, 4), (1, 16, 16, 0, 4), (1, 16, 16, 4, 0), (0, 16, 16, 4, 4)):
        assert lib.conv3x3_wgrad_supported(N, C, K, H, W) == 0
        assert lib.conv3x3_wgrad_scratch_doubles(N, C, K, H, W) == 0
    xp, gz = torch.randn(1, 24, 6, 6, device=DEV), torch.randn(1, 16, 4, 4, device=DEV)
    with pytest.raises(_lib.BbdError):
        ops.conv3x3_wgrad(xp, gz)


def _deterministic_convolutions(monkeypatch):
    """MIOpen's split-K solvers add with atomics and do not repeat their bits; with `cudnn.deterministic` PyTorch-ROCm
    sets MIOPEN_CONVOLUTION_ATTRIB_DETERMINISTIC and they are not chosen (as in tests/test_gpu_trainer.py), so a
    gradient that takes today's path can be held to today's bits."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def _conv_grads(xp, w, gz):
    from baseboostdepth_amd import layers
    block = layers.ConvBlock(w.shape[1], w.shape[0]).to(w.device)
    block.conv.conv.weight = torch.nn.Parameter(w.clone())
    block.conv.conv.weight.requires_grad_(w.requires_grad)
    x = xp.detach().requires_grad_(True)                         # (no clone: a strided input stays strided)
    block.conv_raw(x).backward(gz)
    return x.grad, block.conv.conv.weight.grad


def test_routing_and_fallback(monkeypatch):
    """Unsupported channels, a strided or fp16 input and BBD_FUSED_WGRAD=0 take today's path and give today's gradients;
    a routed pair launches the new call; a weight that asks for no gradient launches nothing."""
    ops, _lib = _ops()
    _deterministic_convolutions(monkeypatch)
    calls = []
    real = ops.conv3x3_wgrad
    monkeypatch.setattr(ops, "conv3x3_wgrad", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    monkeypatch.setattr(ops, "WGRAD_ROUTES", set(ops.WGRAD_ROUTES) | {(16, 16, 6, 20), (24, 16, 6, 20)})
    gen = torch.Generator().manual_seed(7)

    def today(xp, w, gz):
        x = xp.detach().requires_grad_(True)
        ww = w.detach().clone().requires_grad_(True)
        F.conv2d(x, ww, None).backward(gz)
        return x.grad, ww.grad

    def tensors(C, K, dtype=F32):
        xp = torch.randn(2, C, 8, 22, generator=gen).to(DEV, dtype)
        w = (0.1 * torch.randn(K, C, 3, 3, generator=gen)).to(DEV, dtype).requires_grad_(True)
        return xp, w, torch.randn(2, K, 6, 20, generator=gen).to(DEV, dtype)

    # routed: the new call, the data gradient MIOpen's
    xp, w, gz = tensors(16, 16)
    assert ops.conv3x3_wgrad_routed(xp, w)
    gx, gw = _conv_grads(xp, w, gz)
    assert calls == [xp.shape]
    tx, tw = today(xp, w, gz)
    assert torch.equal(gx, tx) and bool(((gw.to(F64) - _wgrad64(xp, gz, 16)).abs() <= _bound(xp, gz, 16, _lib.WGRAD_RUN)).all())
    # no gradient asked of the weight: nothing launched
    del calls[:]
    gx, gw = _conv_grads(xp, w.detach(), gz)
    assert calls == [] and gw is None and torch.equal(gx, tx)
    # today's path, today's gradients: (24 channels are in the table but not supported)
    strided = torch.randn(2, 16, 8, 44, generator=gen).to(DEV)[..., ::2]
    wide = torch.randn(2, 16, 8, 23, generator=gen).to(DEV)
    for xq, wq, gq in (tensors(24, 16), (strided, w, gz), tensors(16, 16, torch.float16), (wide, w, None)):
        assert not ops.conv3x3_wgrad_routed(xq, wq)
        if gq is None:
            continue
        gx, gw = _conv_grads(xq, wq, gq)
        tx, tw = today(xq, wq, gq)
        assert calls == [] and torch.equal(gx, tx) and torch.equal(gw, tw)
    monkeypatch.setattr(ops, "FUSED_WGRAD", False)
    assert not ops.conv3x3_wgrad_routed(xp, w)
    gx, gw = _conv_grads(xp, w, gz)
    tx, tw = today(xp, w, gz)
    assert calls == [] and torch.equal(gx, tx) and torch.equal(gw, tw)


def test_the_measured_layers_are_routed_at_any_batch():
    ops, _lib = _ops()
    lib = ops.default_backend().lib
    for C, K, H, W in sorted(ops.WGRAD_ROUTES):
        assert lib.conv3x3_wgrad_supported(12, C, K, H, W) == 1 and lib.conv3x3_wgrad_supported(1, C, K, H, W) == 1
    xp = torch.empty(1, 16, 194, 642, device=DEV)
    w = torch.empty(16, 16, 3, 3, device=DEV)
    assert ops.conv3x3_wgrad_routed(xp, w) == ops.FUSED_WGRAD
    assert not ops.conv3x3_wgrad_routed(torch.empty(1, 16, 98, 322, device=DEV), w)       # supported, not measured


def test_depth_decoder_with_the_switch_on_and_off(monkeypatch):
    """One backward of a DepthDecoder, batch 2, on ResNet-18 features from 32 x 64 down to 2 x 4 (a pyramid whose coarsest
    map is 1 pixel high cannot take the reflection border), with the four fine convolutions routed (their small shapes are
    put into the table for this test) and with the switch off: every other gradient, the disparities and the feature
    gradients have equal bits, the routed weights meet the bound against a float64 run of the same module."""
    ops, _lib = _ops()
    _deterministic_convolutions(monkeypatch)
    from baseboostdepth_amd import networks
    torch.manual_seed(3)
    enc = [64, 64, 128, 256, 512]
    dec = networks.DepthDecoder(enc, [0, 1, 2, 3]).to(DEV).train()
    feats = [torch.randn(2, c, 32 >> i, 64 >> i, device=DEV) for i, c in enumerate(enc)]
    routes = {(16, 16, 64, 128): "decoder.9", (32, 16, 32, 64): "decoder.8", (64, 32, 16, 32): "decoder.6",
              (96, 32, 32, 64): "decoder.7"}
    monkeypatch.setattr(ops, "WGRAD_ROUTES", set(routes))
    seen, calls = {}, []
    real = ops.conv3x3_wgrad

    def spy(xp, gz, K=None, backend=None):
        calls.append(tuple(gz.shape))
        seen[(xp.shape[1], gz.shape[1]) + tuple(gz.shape[2:])] = (xp.detach().clone(), gz.detach().clone())
        return real(xp, gz, K, backend)

    monkeypatch.setattr(ops, "conv3x3_wgrad", spy)

    def run(module, inputs):
        xs = [t.clone().requires_grad_(True) for t in inputs]
        for p in module.parameters():
            p.grad = None
        out = module(xs)
        sum((out[("disp", s)] * (s + 1.0)).sum() for s in range(4)).backward()
        grads = {n: p.grad.clone() for n, p in module.named_parameters()}
        grads.update({"disp %d" % s: out[("disp", s)].detach().clone() for s in range(4)})
        return grads, [t.grad for t in xs]

    on, on_x = run(dec, feats)
    assert set(seen) == set(routes) and len(calls) == 4
    monkeypatch.setattr(ops, "FUSED_WGRAD", False)
    off, off_x = run(dec, feats)
    again, again_x = run(dec, feats)
    assert len(calls) == 4                                       # the switch off: no launch of the new call
    routed = {name + ".conv.conv.weight" for name in routes.values()}
    assert routed <= set(on)
    # equal bits everywhere but in the routed weights (deterministic convolution solvers: see _deterministic_convolutions)
    for name, a, b, c in ([(n, on[n], off[n], again[n]) for n in on if n not in routed]
                          + [("feature %d" % i, a, b, c) for i, (a, b, c) in enumerate(zip(on_x, off_x, again_x))]):
        assert torch.equal(b, c), "two runs without the new call differ in " + name
        assert torch.equal(a, b), name
    dec64 = networks.DepthDecoder(enc, [0, 1, 2, 3]).to(DEV).double().train()
    dec64.load_state_dict(dec.state_dict())                      # the same parameters, widened
    ref, _ = run(dec64, [t.double() for t in feats])
    for shape, name in routes.items():
        xp, gz = seen[shape]
        key = name + ".conv.conv.weight"
        bound = _bound(xp, gz, shape[1], _lib.WGRAD_RUN)
        err = (on[key].to(F64) - ref[key]).abs()
        mi = (off[key].to(F64) - ref[key]).abs()
        print("%s %s: max error / bound %.4f (MIOpen's gradient on the same measure: %.4f)"
              % (name, shape, float((err / bound).max()), float((mi / bound).max())))
        assert bool((err <= bound).all()), name
