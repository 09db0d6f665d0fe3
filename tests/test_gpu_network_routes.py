"""GPU tier: which C entry points the encoder and the decoders launch, in order ("which path a layer takes").

Every case records the names that go through `ops.default_backend().run` during one forward and one backward of a
module and compares them with the list written down here.  The lists were recorded before the routing conditions of
layers.py, networks/ and networksvit/hr_decoder.py moved into predicates beside the ops; this file uses only names
that existed then, so it passes on both sides of that change: the launches, their order and (decoder cases, two runs
with equal bits) the order of everything between them are the same.

The second part pins the plane limit the Python predicates share with the C entry points: 65 535 planes launch and have
the stock modules' bits, 65 536 take the stock modules and launch nothing."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVEL0 = (16, 16, 32, 64)                   # (C, K, h, w) of level 0 of a DepthDecoder at a 64 x 128 image
WGRADS = {(16, 16, 64, 128), (32, 16, 32, 64)}      # (C, K, H, W) of its upconv(0,1) and upconv(0,0)


def _ops():
    from baseboostdepth_amd import ops, _lib
    return ops, _lib


@pytest.fixture
def launches(monkeypatch):
    """the list every launch's entry-point name is appended to (without its `bbd_`)"""
    ops, _ = _ops()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    backend = ops.default_backend()
    names, real = [], backend.run
    monkeypatch.setattr(backend, "run", lambda name, *a: (names.append(name[len("bbd_"):]), real(name, *a))[1])
    return names


def _names(text):
    return text.split()


def _show(case, names):
    lines, line = [], ""
    for n in names:
        if len(line) + len(n) > 100:
            lines.append(line)
            line = ""
        line += n + " "
    print("ROUTES | %s | %d launches\n    %s" % (case, len(names), "\n    ".join(lines + [line])))


# ------------------------------------------------------------------------------------------------ DepthDecoder
def _decoder(enc=(64, 64, 128, 256, 512), N=2, H=64, W=128, dtype=torch.float32):
    from baseboostdepth_amd import networks
    torch.manual_seed(3)
    dec = networks.DepthDecoder(list(enc), range(4)).to(DEV).to(dtype).train()
    feats = [torch.randn(N, c, H >> (i + 1), W >> (i + 1), device=DEV).to(dtype) for i, c in enumerate(enc)]
    return dec, feats


def _decoder_run(dec, feats):
    """disparities, feature gradients and every parameter gradient of one forward and backward"""
    xs = [t.clone().requires_grad_(True) for t in feats]
    for p in dec.parameters():
        p.grad = None
    out = dec(xs)
    sum((out[("disp", s)].float() * (s + 1.0)).sum() for s in range(4)).backward()
    res = {n: p.grad.clone() for n, p in dec.named_parameters()}
    res.update({"disp %d" % s: out[("disp", s)].detach().clone() for s in range(4)})
    res.update({"feature %d" % i: t.grad for i, t in enumerate(xs)})
    return res


def _decoder_case(case, launches, want, repeatable=True, **kw):
    """The recorded list is `want`, twice, and the two runs agree bit for bit.  (`repeatable` False: with FUSED_NN off
    every pad and up-sampling is ATen's, whose backward adds with atomics - two runs of that path differ in the last
    bits whatever this package does, so only the lists are compared.  Seen, not only expected: on the commit before the
    predicates moved the two runs of that case differed, first in the gradient of decoder.0.conv.conv.weight.)"""
    dec, feats = _decoder(**kw)
    with torch.backends.cudnn.flags(deterministic=True):
        del launches[:]
        first = _decoder_run(dec, feats)
        once = list(launches)
        del launches[:]
        second = _decoder_run(dec, feats)
    _show(case, once)
    assert once == _names(want), case
    assert list(launches) == once, case
    assert sorted(first) == sorted(second)
    for name in first:
        assert not repeatable or torch.equal(first[name], second[name]), (case, name)


# recorded on the commit before the predicates moved
D1 = """
reflect_pad1_fwd upcat_pad_act_fwd bias_elu_pad_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
upcat_pad_act_fwd bias_elu_fwd disp_head_fwd disp_head_bwd bias_elu_bwd upcat_pad_act_bwd
disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd
disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd bias_elu_pad_bwd upcat_pad_act_bwd reflect_pad1_bwd
"""
D2 = """
reflect_pad1_fwd upcat_pad_act_fwd bias_elu_pad_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
up2conv3x3_fwd bias_elu_fwd disp_head_fwd disp_head_bwd bias_elu_bwd up2conv3x3_bwd
upcat_pad_act_fwd conv3x3_wgrad conv3x3_wgrad disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd
disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd
bias_elu_pad_bwd upcat_pad_act_bwd reflect_pad1_bwd
"""
D3_UP2CONV_OFF = """
reflect_pad1_fwd upcat_pad_act_fwd bias_elu_pad_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
upcat_pad_act_fwd bias_elu_fwd disp_head_fwd disp_head_bwd bias_elu_bwd conv3x3_wgrad
upcat_pad_act_bwd conv3x3_wgrad disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd disp_head_bwd
bias_elu_pad_bwd upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd bias_elu_pad_bwd
upcat_pad_act_bwd reflect_pad1_bwd
"""
D3_WGRAD_OFF = """
reflect_pad1_fwd upcat_pad_act_fwd bias_elu_pad_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd
up2conv3x3_fwd bias_elu_fwd disp_head_fwd disp_head_bwd bias_elu_bwd up2conv3x3_bwd
upcat_pad_act_fwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd
upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd bias_elu_pad_bwd
upcat_pad_act_bwd reflect_pad1_bwd
"""
D3_GLUE_OFF = """
reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd
upcat_pad1_fwd bias_elu_fwd disp_head_fwd reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd
disp_head_fwd reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd disp_head_fwd
reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd disp_head_fwd disp_head_bwd bias_elu_bwd
conv3x3_wgrad upcat_pad1_bwd bias_elu_bwd conv3x3_wgrad reflect_pad1_bwd disp_head_bwd bias_elu_bwd
upcat_pad1_bwd bias_elu_bwd reflect_pad1_bwd disp_head_bwd bias_elu_bwd upcat_pad1_bwd bias_elu_bwd
reflect_pad1_bwd disp_head_bwd bias_elu_bwd upcat_pad1_bwd bias_elu_bwd reflect_pad1_bwd
bias_elu_bwd upcat_pad1_bwd bias_elu_bwd reflect_pad1_bwd
"""
D4 = """
reflect_pad1_fwd bias_elu_fwd bias_elu_fwd reflect_pad1_fwd upcat_pad_act_fwd bias_elu_pad_fwd
disp_head_fwd upcat_pad_act_fwd bias_elu_pad_fwd disp_head_fwd upcat_pad_act_fwd bias_elu_pad_fwd
disp_head_fwd upcat_pad_act_fwd bias_elu_fwd disp_head_fwd disp_head_bwd bias_elu_bwd
upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd
upcat_pad_act_bwd disp_head_bwd bias_elu_pad_bwd upcat_pad_act_bwd reflect_pad1_bwd bias_elu_bwd
bias_elu_bwd reflect_pad1_bwd
"""


def test_depth_decoder_defaults(launches):
    _decoder_case("D1", launches, D1)


def test_depth_decoder_level0_routed(launches, monkeypatch):
    ops, _ = _ops()
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", {LEVEL0})
    monkeypatch.setattr(ops, "WGRAD_ROUTES", set(WGRADS))
    _decoder_case("D2", launches, D2)
    assert {"up2conv3x3_fwd", "up2conv3x3_bwd", "conv3x3_wgrad"} <= set(_names(D2))


@pytest.mark.parametrize("switch,want", [("FUSED_UP2CONV", D3_UP2CONV_OFF), ("FUSED_WGRAD", D3_WGRAD_OFF),
                                         ("FUSED_DECODER_GLUE", D3_GLUE_OFF), ("FUSED_NN", "")])
def test_depth_decoder_level0_routed_one_switch_off(launches, monkeypatch, switch, want):
    ops, _ = _ops()
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", {LEVEL0})
    monkeypatch.setattr(ops, "WGRAD_ROUTES", set(WGRADS))
    monkeypatch.setattr(ops, switch, False)
    _decoder_case("D3 %s off" % switch, launches, want, repeatable=switch != "FUSED_NN")


def test_depth_decoder_level_that_a_predicate_refuses(launches):
    """128 images: level 4 concatenates 256 + 256 channels, 65 536 planes; it un-glues itself, the four below stay glued."""
    _decoder_case("D4", launches, D4, enc=(8, 8, 8, 256, 8), N=128, H=64, W=64)


def test_depth_decoder_fp16_launches_nothing(launches):
    dec, feats = _decoder(dtype=torch.float16)
    _decoder_run(dec, feats)
    assert launches == []


# ------------------------------------------------------------------------------------------------ ResnetEncoder
E1 = """
bn_act_grouped_fwd maxpool3s2_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
maxpool3s2_bwd bn_act_grouped_bwd
"""
E2 = """
stem_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd stem_bwd
"""
E3_NO_FEATURE = """
stem_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd stem_bwd
"""
E3_STEM_OFF = """
bn_act_grouped_fwd maxpool3s2_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd bn_act_grouped_fwd
bn_act_grouped_fwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd bn_act_grouped_bwd
maxpool3s2_bwd bn_act_grouped_bwd
"""
E3_BN_OFF = """
maxpool3s2_fwd maxpool3s2_bwd
"""
E3_EVAL = """
maxpool3s2_fwd
"""


def _encoder(H, W):
    from baseboostdepth_amd import networks
    torch.manual_seed(4)
    enc = networks.ResnetEncoder(18, False).to(DEV).train()
    return enc, torch.rand(2, 3, H, W, device=DEV)


def _encoder_run(enc, image, launches):
    del launches[:]
    feats = enc(image)
    if torch.is_grad_enabled():
        sum(f.sum() for f in feats if f is not None).backward()
    return list(launches)


def _stem_elems(image):
    """elements per channel of the whole batch (one call group) in conv1's output"""
    return image.shape[0] * (image.shape[2] // 2) * (image.shape[3] // 2)


def test_encoder_below_the_stem_threshold(launches):
    _, _lib = _ops()
    enc, image = _encoder(64, 128)
    assert _stem_elems(image) <= _lib.STEM_MIN_ELEMS
    got = _encoder_run(enc, image, launches)
    _show("E1", got)
    assert got == _names(E1)
    assert "maxpool3s2_fwd" in got and "stem_fwd" not in got


def test_encoder_above_the_stem_threshold(launches):
    _, _lib = _ops()
    enc, image = _encoder(128, 256)
    assert _stem_elems(image) > _lib.STEM_MIN_ELEMS
    got = _encoder_run(enc, image, launches)
    _show("E2", got)
    assert got == _names(E2)
    assert "stem_fwd" in got and "maxpool3s2_fwd" not in got


def test_encoder_without_the_stem_feature(launches):
    enc, image = _encoder(128, 256)
    enc.stem_feature = False
    got = _encoder_run(enc, image, launches)
    _show("E3 stem_feature False", got)
    assert got == _names(E3_NO_FEATURE)


def test_encoder_with_the_stem_switch_off(launches, monkeypatch):
    ops, _ = _ops()
    enc, image = _encoder(128, 256)
    monkeypatch.setattr(ops, "FUSED_STEM", False)
    got = _encoder_run(enc, image, launches)
    _show("E3 FUSED_STEM off", got)
    assert got == _names(E3_STEM_OFF)


def test_encoder_with_the_batchnorm_switch_off(launches):
    from baseboostdepth_amd.networks.encoder import FusedBatchNorm2d
    enc, image = _encoder(128, 256)
    before = FusedBatchNorm2d.fused
    FusedBatchNorm2d.fused = False
    try:
        got = _encoder_run(enc, image, launches)
    finally:
        FusedBatchNorm2d.fused = before
    _show("E3 FusedBatchNorm2d.fused False", got)
    assert got == _names(E3_BN_OFF)


def test_encoder_in_eval_mode(launches):
    enc, image = _encoder(128, 256)
    enc.eval()
    with torch.no_grad():
        got = _encoder_run(enc, image, launches)
    _show("E3 eval", got)
    assert got == _names(E3_EVAL)
    assert not [n for n in got if n.startswith(("bn_", "stem_"))]


# ------------------------------------------------------------------------------------------------ MonoViT's decoder
H1 = """
reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd
upcat_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd
reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd
reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd
reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd
reflect_pad1_fwd bias_elu_fwd reflect_pad1_fwd bias_elu_fwd upcat_pad1_fwd bias_elu_fwd dispconv_fwd
dispconv_fwd dispconv_fwd dispconv_fwd dispconv_bwd dispconv_bwd dispconv_bwd dispconv_bwd
bias_elu_bwd upcat_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd
reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd
reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd
reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd
upcat_pad1_bwd bias_elu_bwd reflect_pad1_bwd bias_elu_bwd upcat_pad1_bwd bias_elu_bwd
reflect_pad1_bwd bias_elu_bwd upcat_pad1_bwd bias_elu_bwd reflect_pad1_bwd
"""


def _hr_decoder_run(launches):
    """The default constructor (MonoViT's widths) on the smallest pyramid its forward takes: 2 x 2 at the coarsest level
    (a reflection border needs two pixels), doubling up to 32 x 32."""
    from baseboostdepth_amd import networksvit
    torch.manual_seed(5)
    dec = networksvit.DepthDecoder().to(DEV).train()
    widths = [dec.num_ch_enc[0]] + list(dec.ch_enc[1:])
    feats = [torch.randn(1, c, 32 >> i, 32 >> i, device=DEV, requires_grad=True) for i, c in enumerate(widths)]
    del launches[:]
    out = dec(feats)
    sum((out[("disp", s)] * (s + 1.0)).sum() for s in range(4)).backward()
    return list(launches)


def test_hr_decoder_defaults(launches):
    got = _hr_decoder_run(launches)
    _show("H1", got)
    assert got == _names(H1)


def test_hr_decoder_with_the_switch_off(launches, monkeypatch):
    ops, _ = _ops()
    monkeypatch.setattr(ops, "FUSED_NN", False)
    assert _hr_decoder_run(launches) == []


# ------------------------------------------------------------------------------------------------ the plane limit
def _distinct_planes(planes):
    """[1, planes, 2, 2]: every plane a permutation of four distinct values (no tied maxima)"""
    gen = torch.Generator().manual_seed(9)
    order = torch.rand(planes, 4, generator=gen).argsort(1).float()
    scale = 1.0 + torch.arange(planes).float().remainder(7.0).reshape(-1, 1)
    return ((order - 1.5) * scale).reshape(1, planes, 2, 2).to(DEV)


def _small_integers(*shape):
    """gradients whose sums are exact in float32 whatever the order (the stock pad backward adds with atomics)"""
    gen = torch.Generator().manual_seed(10)
    return torch.randint(-8, 9, shape, generator=gen).float().to(DEV)


def _both_ways(module, x, grad):
    xx = x.clone().requires_grad_(True)
    out = module(xx)
    out.backward(grad)
    return out.detach(), xx.grad


@pytest.mark.parametrize("which", ["reflect_pad1", "maxpool3s2"])
def test_the_most_planes_a_launch_takes_and_one_more(launches, which):
    from baseboostdepth_amd import layers
    from baseboostdepth_amd.networks.encoder import MaxPool3s2
    ours, stock = {"reflect_pad1": (layers.ReflectionPad1(), nn.ReflectionPad2d(1)),
                   "maxpool3s2": (MaxPool3s2(), nn.MaxPool2d(3, 2, 1))}[which]
    x = _distinct_planes(65535)
    grad = _small_integers(1, 65535, *((4, 4) if which == "reflect_pad1" else (1, 1)))
    want, want_grad = _both_ways(stock, x, grad)
    if which == "maxpool3s2":                                   # the reference alone: one arg-max per window
        assert bool(((x == want).sum((2, 3)) == 1).all())
    del launches[:]
    got, got_grad = _both_ways(ours, x, grad)
    assert launches == [which + "_fwd", which + "_bwd"]
    assert torch.equal(got, want) and torch.equal(got_grad, want_grad)

    x = _distinct_planes(65536)
    grad = _small_integers(1, 65536, *grad.shape[2:])
    want, want_grad = _both_ways(stock, x, grad)
    del launches[:]
    got, got_grad = _both_ways(ours, x, grad)
    assert launches == []
    assert torch.equal(got, want) and torch.equal(got_grad, want_grad)
