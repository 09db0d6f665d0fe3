"""CPU tier for the MonoViT token kernels' float64 references (tests/vit_f64_ref.py).

1. Each reference against this build's own eager module path in fp32 on the CPU (FactorAtt_ConvRelPosEnc, ConvPosEnc,
   ConvRelPosEnc, MHCABlock): a wrong reference must not be able to agree with a wrong kernel.
   Bound: EAGER_BOUND of every group's maximum.  The modules and the references are two orderings of the same fp32-exact
   formula; fp32 sums of at most ~10^3 terms differ from float64 by about sqrt(10^3) * 2^-24 = 2e-6, and a wrong formula
   (a dropped term, another axis, a missing scale) is off by 1e-2 or more.
2. The launch geometry the GPU cases rely on, through the library's host functions (no GPU needed)."""
import ctypes
import types

import pytest
import torch

import vit_f64_ref as R

EAGER_BOUND = 2e-5


@pytest.fixture(scope="module")
def dll():
    from baseboostdepth_amd.csrc.build import build
    lib = ctypes.CDLL(build())
    lib.bbd_factor_att_scratch_floats.restype = ctypes.c_long
    return lib


def _compare(names, kinds, got, want):
    assert len(got) == len(want) == len(names)
    for name, kind, a, b in zip(names, kinds, got, want):
        err = R.group_error(a, b, kind)
        assert err <= EAGER_BOUND, (name, err)


def _module_run(fn, x, params, upstream):
    """fp32 module path: outputs and gradients of x and of the module's parameters."""
    x = x.clone().requires_grad_(True)
    out = fn(x)
    grads = torch.autograd.grad((out * upstream).sum(), [x] + params)
    return [out.detach()] + list(grads)


def _crpe(Ch, heads, windows=None):
    from baseboostdepth_amd.networksvit.mpvit import ConvRelPosEnc
    crpe = ConvRelPosEnc(Ch, heads, windows or {3: 2, 5: 3, 7: 3})
    with torch.no_grad():
        for p in crpe.parameters():
            p.copy_(R.rounded(R.draw(torch.Generator().manual_seed(p.numel()), *p.shape) * 0.3))
    return crpe


@pytest.mark.parametrize("B,H,W,C,heads", [(2, 5, 7, 64, 8), (1, 2, 3, 96, 8), (2, 4, 5, 176, 8)])
def test_attention_reference_against_the_eager_module(B, H, W, C, heads):
    from baseboostdepth_amd.networksvit.mpvit import FactorAtt_ConvRelPosEnc
    gen = torch.Generator().manual_seed(C + H)
    torch.manual_seed(C)
    att = FactorAtt_ConvRelPosEnc(C, num_heads=heads, qkv_bias=True, shared_crpe=_crpe(C // heads, heads))
    with torch.no_grad():
        att.qkv.weight.mul_(4.0)          # k far enough from zero for a softmax that is not flat
    x = R.rounded(R.draw(gen, B, H * W, C))
    up = R.rounded(R.draw(gen, B, H * W, C))
    params = list(att.parameters())
    got = _module_run(lambda t: att(t, (H, W)), x, params, up)
    nconv = len(att.crpe.conv_list)

    def formula(x, wq, bq, wp, bp, *conv):
        qkv = R.linear(x, wq, bq)
        out = R.factor_attention_crpe(qkv, (H, W), conv[0::2], conv[1::2], heads, att.scale)
        return R.linear(out, wp, bp)
    leaves = [x, att.qkv.weight, att.qkv.bias, att.proj.weight, att.proj.bias]
    for c in att.crpe.conv_list:
        leaves += [c.weight, c.bias]
    want = R.forward_backward(formula, [t.detach() for t in leaves], [], [up], "cpu", torch.float64)
    order = {id(p): i for i, p in enumerate(leaves[1:])}
    want = want[:2] + [want[2 + order[id(p)]] for p in params]
    assert len(want) == 2 + 4 + 2 * nconv
    _compare(["out", "grad x"] + [n for n, _ in att.named_parameters()], ["channel", "channel"] + ["tensor"] * len(params), got, want)

    # the form that takes convv as given, against the same module with the convolutions' output handed in
    qkv = att.qkv(x).detach()
    convv = att.crpe.conv_v(qkv[:, :, 2 * C:], (H, W)).detach()
    a = R.factor_attention(qkv.double(), convv.double(), heads, att.scale)
    b = R.factor_attention_crpe(qkv.double(), (H, W), [c.weight.detach().double() for c in att.crpe.conv_list],
                                [c.bias.detach().double() for c in att.crpe.conv_list], heads, att.scale)
    assert R.group_error(a, b, "channel") <= EAGER_BOUND


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 12), (1, 1, 1, 5), (1, 7, 9, 70)])
def test_position_encoding_references_against_the_eager_modules(B, H, W, C):
    from baseboostdepth_amd.networksvit.mpvit import ConvPosEnc
    gen = torch.Generator().manual_seed(C)
    torch.manual_seed(C)
    x = R.rounded(R.draw(gen, B, H * W, C) * R.channel_scales(gen, C, 10.0))
    up = R.rounded(R.draw(gen, B, H * W, C))
    cpe = ConvPosEnc(C, k=3)
    params = list(cpe.parameters())
    got = _module_run(lambda t: cpe(t, (H, W)), x, params, up)
    want = R.forward_backward(lambda t, w, b: R.dwconv_tokens(t, (H, W), [w], [b], add_input=True),
                              [x, cpe.proj.weight.detach(), cpe.proj.bias.detach()], [], [up], "cpu", torch.float64)
    _compare(["y", "grad x", "grad weight", "grad bias"], ["channel", "channel", "tensor", "tensor"], got, want)


@pytest.mark.parametrize("B,H,W,Ch,heads,windows", [(2, 4, 6, 3, 8, None), (1, 2, 3, 5, 4, {3: 1, 5: 1, 7: 2}), (1, 5, 5, 4, 2, 7)])
def test_relative_position_encoding_reference_against_the_eager_module(B, H, W, Ch, heads, windows):
    gen = torch.Generator().manual_seed(Ch + heads)
    crpe = _crpe(Ch, heads, windows)
    N, C = H * W, Ch * heads
    q = R.rounded(R.draw(gen, B, heads, N, Ch))
    v = R.rounded(R.draw(gen, B, heads, N, Ch))
    got = crpe(q, v, (H, W)).detach()                                           # [B, h, N, Ch]
    conv = R.dwconv_tokens(v.double().transpose(1, 2).reshape(B, N, C), (H, W), [c.weight.detach().double() for c in crpe.conv_list],
                           [c.bias.detach().double() for c in crpe.conv_list])
    want = q.double() * conv.reshape(B, N, heads, Ch).transpose(1, 2)
    assert R.group_error(got.transpose(1, 2).reshape(B, N, C), want.transpose(1, 2).reshape(B, N, C), "channel") <= EAGER_BOUND


def test_block_references_against_the_eager_block_and_its_float64_copy():
    """MHCABlock = ConvPosEnc, LayerNorm, attention, residual + LayerNorm, MLP, residual: the composition of the
    references equals the fp32 block (EAGER_BOUND) and the block's own float64 copy (float64 rounding)."""
    from baseboostdepth_amd.networksvit.mpvit import MHCABlock, ConvPosEnc
    B, H, W, C, heads = 2, 3, 4, 64, 8
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    blk = MHCABlock(C, heads, mlp_ratio=2, shared_cpe=ConvPosEnc(C), shared_crpe=_crpe(C // heads, heads))
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    x = R.rounded(R.draw(gen, B, H * W, C) + 50.0 * R.draw(gen, B, H * W, 1))
    up = R.rounded(R.draw(gen, B, H * W, C))
    params = list(blk.parameters())
    got = _module_run(lambda t: blk(t, (H, W)), x, params, up)
    b64 = R.float64_copy(blk)
    copy64 = _module_run(lambda t: b64(t, (H, W)), x.double(), list(b64.parameters()), up.double())
    p = types.SimpleNamespace(**{n.replace(".", "_"): t for n, t in b64.named_parameters()})
    att = b64.factoratt_crpe

    def formula(t):
        t = R.dwconv_tokens(t, (H, W), [p.cpe_proj_weight], [p.cpe_proj_bias], add_input=True)
        _, z = R.residual_layernorm(t, None, None, p.norm1_weight, p.norm1_bias, blk.norm1.eps)
        qkv = R.linear(z, p.factoratt_crpe_qkv_weight, p.factoratt_crpe_qkv_bias)
        a = R.factor_attention_crpe(qkv, (H, W), [c.weight for c in att.crpe.conv_list], [c.bias for c in att.crpe.conv_list],
                                    heads, att.scale)
        a = R.linear(a, p.factoratt_crpe_proj_weight, p.factoratt_crpe_proj_bias)
        y, z = R.residual_layernorm(t, a, None, p.norm2_weight, p.norm2_bias, blk.norm2.eps)
        m = R.linear(torch.nn.functional.gelu(R.linear(z, p.mlp_fc1_weight, p.mlp_fc1_bias)), p.mlp_fc2_weight, p.mlp_fc2_bias)
        return R.residual_add(y, m, None)
    want = _module_run(formula, x.double(), list(b64.parameters()), up.double())
    names = ["out", "grad x"] + [n for n, _ in blk.named_parameters()]
    kinds = ["channel", "channel"] + ["tensor"] * len(params)
    _compare(names, kinds, got, want)
    for name, kind, a, b in zip(names, kinds, copy64, want):
        assert R.group_error(a, b, kind) <= 1e-12, name


def test_residual_and_mask_references():
    gen = torch.Generator().manual_seed(3)
    x, br = R.draw(gen, 3, 5, 8), R.draw(gen, 3, 5, 8)
    mask = torch.tensor([0.0, 1.25, 1.25], dtype=torch.float64)
    y = R.residual_add(x, br, mask)
    assert torch.equal(y[0], x[0]) and torch.equal(y[1:], x[1:] + 1.25 * br[1:])
    assert torch.equal(R.residual_add(x, br, None), x + br)
    w, b = R.draw(gen, 8), R.draw(gen, 8)
    y2, z = R.residual_layernorm(x, br, mask, w, b, 1e-6)
    assert torch.equal(y2, y)
    mean, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
    assert float((z - ((y - mean) / (var + 1e-6).sqrt() * w + b)).abs().max()) < 1e-13
    assert R.residual_layernorm(x, None, None, w, b, 1e-6)[0] is x


# ------------------------------------------------------------------------------------------------ launch geometry
def test_token_segments_cover_every_token(dll):
    """nseg * ceil(N / nseg) >= N for all B <= 128, N <= 4096, and the scratch size is B * nseg * (2C + C*Ch)."""
    seg = dll.bbd_factor_att_segments
    for B in range(1, 129):
        for N in range(1, 4097):
            nseg = seg(B, N)
            assert nseg >= 1 and nseg * ((N + nseg - 1) // nseg) >= N, (B, N, nseg)
    for B, N, C, Ch in [(16, 1025, 64, 8), (2, 37, 132, 33), (1, 19, 576, 18), (12, 7680, 64, 8), (128, 4096, 288, 36)]:
        assert dll.bbd_factor_att_scratch_floats(B, N, C, Ch) == B * seg(B, N) * (2 * C + C * Ch)


def test_smallest_case_with_empty_trailing_segments(dll):
    """B = 16, N = 1025: 64 segments of 17 tokens, so segments 61..63 hold no token - the GPU tier's empty-segment case."""
    nseg = dll.bbd_factor_att_segments(16, 1025)
    seg_tokens = (1025 + nseg - 1) // nseg
    assert (nseg, seg_tokens) == (64, 17)
    assert [s for s in range(nseg) if s * seg_tokens >= 1025] == [61, 62, 63]


def test_attention_predicate_accepts_what_the_launches_can_deliver(dll):
    ok = dll.bbd_factor_att_supported
    for dims in ((64, 96, 176, 216), (64, 128, 192, 256), (64, 128, 216, 288)):          # MPViT tiny / xsmall / small
        for C in dims:
            assert ok(C, C // 8), C
    assert ok(512, 16) and ok(576, 18)
    for C, Ch in ((768, 16), (1024, 12), (256, 1), (512, 2)):
        assert not ok(C, Ch), (C, Ch)
    # every shape of the GPU tier's attention cases is one the predicate accepts
    for C, heads in ((64, 8), (96, 8), (128, 8), (64, 1), (128, 2), (132, 4), (132, 33), (176, 8), (192, 8), (256, 8), (256, 32),
                     (180, 4), (192, 4), (132, 11), (160, 8), (156, 4), (172, 4), (512, 32), (576, 32), (216, 8)):
        assert ok(C, C // heads), (C, heads)
    # the row form is refused exactly where its padded tile passes 64 KiB: also with heads wider than 4 channels
    assert not ok(510, 5) and not ok(504, 6) and ok(504, 8) and ok(512, 4)
    assert not ok(768, 768 // 48)                                                        # the GPU tier's fallback case
    assert not ok(0, 1) and not ok(64, 0) and not ok(64, 7) and not ok(1028, 4)
