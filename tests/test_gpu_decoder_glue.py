"""GPU tier: the depth decoder's glue with the ConvBlocks' bias + ELU inside (ops.upcat_pad_act, ops.bias_elu_pad;
csrc/bbd_nn.hip, bbd_upcat_pad_act_* / bbd_bias_elu_pad_*) against the composition it replaces.

Every activation and every gradient but the bias's is the composition's bit for bit (torch.equal): the kernels keep its
expressions and their order.  The bias gradient adds the same numbers in another order and is measured against float64
like the other glue kernels (tests/test_gpu_nn_f64.py): its error may be bound(error of the composition).  Each case also
goes through gpu_f64_common.check: three runs with equal bits, one after NaN-filled allocator blocks, every tensor
against the float64 formula.

Shapes: those of the issue, and one more per op whose rows are longer than one 64-lane sweep of the 16-bytes-per-lane
form (w = 260: 65 lanes of four columns; W = 260 likewise) - the listed ones cross a sweep with one element per lane only."""
import pytest
import torch

import nn_f64_ref as R
from gpu_f64_common import DEV, check as _check

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

UPCAT_ACT_CASES = [(1, 1, 0, 1, 1), (2, 3, 2, 1, 3), (1, 2, 1, 3, 1), (2, 4, 4, 16, 32), (1, 2, 3, 5, 33), (1, 1, 1, 2, 65),
                   (1, 1, 1, 2, 260)]
BIAS_ELU_PAD_CASES = [(1, 1, 2, 2), (2, 3, 3, 3), (1, 2, 2, 7), (1, 2, 5, 66), (3, 70, 4, 36), (2, 4, 48, 64), (1, 1, 3, 260)]


def _ops():
    from baseboostdepth_amd import ops
    return ops


def _glue_inputs(gen, shape):
    """(z, bias) by nn_f64_ref.bias_elu_inputs' recipe (channel scales 10^U(-4,1), the bias scaled alike, channel 0's
    bias 0).  From eight elements on, the first three of the tensor are set so that z + bias is exactly 0 (ELU' = 1 at
    y = 0), about -95 and about -1e3 (expm1f = -1 exactly, gradient exactly 0)."""
    N, C, H, W = shape
    scales = R.channel_scales(gen, C, 10.0, -4.0, 1.0)
    z = R.rounded(R.draw(gen, *shape) * scales.reshape(1, C, 1, 1))
    bias = R.rounded(0.5 * R.draw(gen, C) * scales)
    bias[0] = 0.0
    if z.numel() >= 8:
        flat = z.reshape(-1)                                   # a view: plane (0, 0) first
        chan = [(k // (H * W)) % C for k in range(3)]
        flat[0] = -bias[chan[0]]
        flat[1] = -95.0 - bias[chan[1]]
        flat[2] = -1e3 - bias[chan[2]]
    return z, bias


def _old_bias_elu(t, b):
    """The composition's first step, `ops.bias_elu_(t * 1.0, b)`.  That kernel takes planes of whole float4s only (the
    decoder's always are); for the other shapes of the lists above it runs on the planes lengthened to the next multiple
    of four, and the result is cut back: the same kernel's bits for every element, and the added elements get a zero
    gradient, so they add exact zeros to its bias gradient."""
    ops = _ops()
    N, C, H, W = t.shape
    if (H * W) % 4 == 0:
        return ops.bias_elu_(t * 1.0, b)
    longer = torch.nn.functional.pad(t.reshape(N, C, 1, H * W), (0, -(H * W) % 4))
    return ops.bias_elu_(longer, b)[..., :H * W].reshape(N, C, H, W)


def _upstream(gen, *shape):
    return R.rounded(R.draw(gen, *shape) * R.channel_scales(gen, shape[1], 10.0).reshape(1, -1, 1, 1))


def _views(names, bias_at):
    views = [(n, "channel", lambda r, i=i: R.nhwc(r[i])) for i, n in enumerate(names) if i != bias_at]
    return views + [("grad bias", "tensor", lambda r: r[bias_at])]


def _against_composition(case, new, old, formula, leaves, upstream, names, bias_at, scratch):
    """`new` / `old`: fn(*leaves) -> output(s).  Everything but the bias gradient equal bits; the bias gradient's error
    against float64 within bound(the composition's)."""
    got, ref = _check(case, new, formula, leaves, [], upstream, _views(names, bias_at), scratch)
    comp = R.forward_backward(old, leaves, [], upstream, DEV, F32)
    assert len(got) == len(comp) == len(names)
    for i, name in enumerate(names):
        if i != bias_at:
            assert torch.equal(got[i], comp[i]), (case, name)
    e_old, e_new = R.group_error(comp[bias_at], ref[bias_at], "tensor"), R.group_error(got[bias_at], ref[bias_at], "tensor")
    print("GLUE | %s | grad bias | composition %.2e | kernel %.2e | bound %.2e" % (case, e_old, e_new, R.bound(e_old)))
    assert e_new <= R.bound(e_old), (case, e_old, e_new)
    return got


# ------------------------------------------------------------------------------------------------ upcat_pad_act
@pytest.mark.parametrize("N,C1,C2,h,w", UPCAT_ACT_CASES)
def test_upcat_pad_act_is_the_composition(N, C1, C2, h, w):
    ops = _ops()
    gen = torch.Generator().manual_seed(N + 3 * C1 + 5 * C2 + 7 * h + 11 * w)
    z, bias = _glue_inputs(gen, (N, C1, h, w))
    skip = _upstream(gen, N, C2, 2 * h, 2 * w) if C2 else None
    up = _upstream(gen, N, C1 + C2, 2 * h + 2, 2 * w + 2)
    assert ops.upcat_pad_act_supported(z.to(DEV), bias.to(DEV), None if skip is None else skip.to(DEV))
    names = ["out", "grad z", "grad bias"] + (["grad skip"] if C2 else [])
    leaves = [z, bias] + ([skip] if C2 else [])

    def new(t, b, s=None):
        return ops.upcat_pad_act(t * 1.0, b, s)

    def old(t, b, s=None):
        return ops.upcat_pad(_old_bias_elu(t, b), s)

    def formula(t, b, s=None):
        return R.upcat_pad(R.bias_elu(t, b), s)
    got = _against_composition("upcat_pad_act %s" % ((N, C1, C2, h, w),), new, old, formula, leaves, [up], names, 2,
                               [2 * C1 * N * ((h + 3) // 4), C1])
    if z.numel() >= 8:
        y = got[0][0, 0, 1, 1:7:2].cpu()                       # padded (1, 1), (1, 3), (1, 5) show z[0, 0, 0, 0..2]
        assert y[0] == 0.0 and (w < 3 or (y[1] == -1.0 and y[2] == -1.0))
        assert w < 3 or got[1].reshape(-1)[1:3].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ bias_elu_pad
@pytest.mark.parametrize("which", ["both", "yp only", "y only"])
@pytest.mark.parametrize("shape", BIAS_ELU_PAD_CASES)
def test_bias_elu_pad_is_the_composition(shape, which):
    ops = _ops()
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(p * s for p, s in zip((1, 3, 5, 7), shape)))
    z, bias = _glue_inputs(gen, shape)
    ups = [_upstream(gen, N, C, H, W), _upstream(gen, N, C, H + 2, W + 2)]
    assert ops.bias_elu_pad_supported(z.to(DEV), bias.to(DEV))
    pick = {"both": slice(0, 2), "yp only": slice(1, 2), "y only": slice(0, 1)}[which]

    def new(t, b):
        return tuple(ops.bias_elu_pad(t * 1.0, b)[pick])

    def old(t, b):
        y = _old_bias_elu(t, b)
        return tuple((y, ops.reflect_pad1(y))[pick])

    def formula(t, b):
        y = R.bias_elu(t, b)
        return tuple((y, R.reflect_pad1(y))[pick])
    names = ["y", "yp"][pick] + ["grad z", "grad bias"]
    got = _against_composition("bias_elu_pad %s %s" % (shape, which), new, old, formula, [z, bias], ups[pick], names,
                               len(names) - 1, [2 * C * N * ((H + 3) // 4), C])
    if z.numel() >= 8 and which != "yp only":
        assert got[0].reshape(-1)[:3].tolist() == [0.0, -1.0, -1.0] and got[-2].reshape(-1)[1:3].tolist() == [0.0, 0.0]


def test_bias_elu_pad_writes_its_first_output_in_place():
    ops = _ops()
    gen = torch.Generator().manual_seed(5)
    z, bias = [t.to(DEV) for t in _glue_inputs(gen, (2, 3, 4, 8))]
    conv_out = z.clone()
    y, yp = ops.bias_elu_pad(conv_out, bias)
    assert y.data_ptr() == conv_out.data_ptr() and yp.shape == (2, 3, 6, 10)
    assert torch.equal(y, ops.bias_elu_(z.clone(), bias)) and torch.equal(yp, ops.reflect_pad1(y))


# ------------------------------------------------------------------------------------------------ the decoder
def _decoder_run(dec, feats, ups, glue, monkeypatch, counted=()):
    ops = _ops()
    calls = dict.fromkeys(counted, 0)
    with monkeypatch.context() as m:
        m.setattr(ops, "FUSED_DECODER_GLUE", glue)
        for name in counted:
            def counting(*args, _fn=getattr(ops, name), _name=name, **kwargs):
                calls[_name] += 1
                return _fn(*args, **kwargs)
            m.setattr(ops, name, counting)
        xs = [t.to(DEV).clone().requires_grad_(True) for t in feats]
        for p in dec.parameters():
            p.grad = None
        out = dec(xs)
        disps = [out[("disp", s)] for s in range(4)]
        sum((d * u.to(DEV)).sum() for d, u in zip(disps, ups)).backward()
        grads = {n: p.grad.clone() for n, p in dec.named_parameters()}
    return [d.detach() for d in disps], [t.grad for t in xs], grads, calls


def _block_biases(dec):
    """names of the ten ConvBlock biases (the decoder's first ten stages)"""
    return ["decoder.%d.conv.conv.bias" % i for i in range(10)]


COUNTED = ("bias_elu_", "reflect_pad1", "upcat_pad", "upcat_pad_act", "bias_elu_pad")


def test_depth_decoder_with_the_glue_switch_on_and_off(monkeypatch):
    """The decoder of test_depth_decoder_against_its_float64_copy (64 x 128 image, MIOpen's deterministic solvers) with
    ops.FUSED_DECODER_GLUE on and off: disparities, input gradients and every parameter gradient but the ConvBlock
    biases' equal bits; those biases against the float64 copy within bound(error of the switch-off run)."""
    from baseboostdepth_amd import networks
    H, W = 64, 128
    torch.manual_seed(4)
    dec = networks.DepthDecoder([64, 64, 128, 256, 512], [0, 1, 2, 3]).train()
    gen = torch.Generator().manual_seed(4)
    feats = [R.rounded(R.draw(gen, 2, c, H >> (i + 1), W >> (i + 1)).abs()) for i, c in enumerate([64, 64, 128, 256, 512])]
    ups = [R.rounded(R.draw(gen, 2, 1, H >> s, W >> s)) for s in range(4)]
    ref = R.float64_copy(dec)
    out = ref([t.double().requires_grad_(True) for t in feats])
    sum((out[("disp", s)] * ups[s].double()).sum() for s in range(4)).backward()
    ref_grads = {n: p.grad for n, p in ref.named_parameters()}
    dec = dec.to(DEV)
    with torch.backends.cudnn.flags(deterministic=True):
        off = _decoder_run(dec, feats, ups, False, monkeypatch, COUNTED)
        on = _decoder_run(dec, feats, ups, True, monkeypatch, COUNTED)
    assert off[3]["upcat_pad_act"] == 0 and off[3]["bias_elu_pad"] == 0 and off[3]["upcat_pad"] == 5
    assert on[3] == {"bias_elu_": 1, "reflect_pad1": 1, "upcat_pad": 0, "upcat_pad_act": 5, "bias_elu_pad": 4}
    for s in range(4):
        assert torch.equal(on[0][s], off[0][s]), "disparity %d" % s
    for i in range(5):
        assert torch.equal(on[1][i], off[1][i]), "gradient of feature %d" % i
    biases = _block_biases(dec)
    assert set(biases) <= set(on[2]) and len(on[2]) == 28
    failures = []
    for name in on[2]:
        if name not in biases:
            assert torch.equal(on[2][name], off[2][name]), name
            continue
        e_off = R.group_error(off[2][name], ref_grads[name], "tensor")
        e_on = R.group_error(on[2][name], ref_grads[name], "tensor")
        print("GLUE | decoder | %s | off %.2e | on %.2e | bound %.2e" % (name, e_off, e_on, R.bound(e_off)))
        if not e_on <= R.bound(e_off):
            failures.append((name, e_off, e_on))
    assert not failures, failures


def test_depth_decoder_keeps_the_old_path_where_a_predicate_refuses(monkeypatch):
    """128 images: level 4 concatenates 256 + 256 channels, 65 536 planes - one more than a launch takes.  That level runs
    as before (its ConvBlocks' bias gradients included, bit for bit), the four below it take the new path, and the
    results are those of the switch-off run.  (The other bias gradients: the test above.)"""
    from baseboostdepth_amd import networks
    ops = _ops()
    N, H, W, enc = 128, 64, 64, [8, 8, 8, 256, 8]
    torch.manual_seed(6)
    dec = networks.DepthDecoder(enc, [0, 1, 2, 3]).train().to(DEV)
    gen = torch.Generator().manual_seed(6)
    feats = [R.rounded(R.draw(gen, N, c, H >> (i + 1), W >> (i + 1)).abs()) for i, c in enumerate(enc)]
    ups = [R.rounded(R.draw(gen, N, 1, H >> s, W >> s)) for s in range(4)]
    z = torch.empty(N, 256, 2, 2, device=DEV)
    assert not ops.upcat_pad_act_supported(z, dec.decoder[0].conv.conv.bias, feats[3].to(DEV))
    assert ops.upcat_pad_act_supported(z[:127], dec.decoder[0].conv.conv.bias, feats[3][:127].to(DEV))
    assert not ops.bias_elu_pad_supported(torch.empty(1, 65536, 2, 2, device=DEV), torch.empty(65536, device=DEV))
    with torch.backends.cudnn.flags(deterministic=True):
        off = _decoder_run(dec, feats, ups, False, monkeypatch, COUNTED)
        on = _decoder_run(dec, feats, ups, True, monkeypatch, COUNTED)
    assert on[3] == {"bias_elu_": 3, "reflect_pad1": 2, "upcat_pad": 0, "upcat_pad_act": 4, "bias_elu_pad": 3}
    for s in range(4):
        assert torch.equal(on[0][s], off[0][s]), "disparity %d" % s
    for i in range(5):
        assert torch.equal(on[1][i], off[1][i]), "gradient of feature %d" % i
    later = _block_biases(dec)[2:]
    for name in on[2]:
        if name not in later:
            assert torch.equal(on[2][name], off[2][name]), name
