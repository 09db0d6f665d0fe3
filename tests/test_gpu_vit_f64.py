"""GPU tier: the MonoViT token kernels (csrc/bbd_vit.hip, csrc/bbd_tokens.hip) against float64 references, on every
dispatch path of their launch code.

Each case runs forward and backward through the public `ops.*` entry point and is measured as tests/vit_f64_ref.py
describes: per channel / per row / per parameter tensor, against the float64 result, and bounded by 8 x the error
of the eager fp32 formulation on the GPU on the same inputs (floor 8 * 2^-24).  Every case also runs a second time
(bit-equal: the kernels are deterministic) and a third time after allocator blocks of its scratch and output sizes
were filled with NaN and freed (bit-equal again: nothing reads what it did not write).

Measured on an MI355X (`layernorm_tokens` without passthrough measures like the passthrough form; y of the passthrough
form and grad x of residual_add are exact on both sides):

attention, per case: eager error, kernel error, kernel / eager for each tensor
(B, N, C, heads)                    out                   dq                    dk                    dv                    grad convv
(16, 1025, 64, 8)                   6.6e-07 3.6e-07 0.56  7.8e-07 4.7e-07 0.60  1.0e-06 1.2e-06 1.12  8.3e-07 4.7e-07 0.57  5.0e-08 5.0e-08 0.84
(2, 37, 96, 8)                      3.4e-07 3.2e-07 0.95  4.1e-07 5.9e-07 1.44  3.1e-06 3.0e-06 0.97  5.8e-07 4.7e-07 0.81  5.4e-08 5.4e-08 0.90
(2, 37, 128, 8)                     3.8e-07 4.1e-07 1.08  5.7e-07 4.3e-07 0.75  1.1e-06 8.0e-07 0.70  5.8e-07 3.6e-07 0.63  5.3e-08 5.3e-08 0.88
(2, 37, 64, 1)                      3.8e-07 3.4e-07 0.89  6.8e-07 7.1e-07 1.05  9.0e-07 9.9e-07 1.09  4.5e-07 4.8e-07 1.05  5.2e-08 5.2e-08 0.87
(2, 37, 128, 2)                     5.8e-07 4.6e-07 0.78  7.1e-07 6.3e-07 0.89  2.6e-06 2.0e-06 0.80  6.5e-07 5.3e-07 0.81  5.0e-08 5.0e-08 0.84
(2, 37, 132, 4)                     4.9e-07 4.0e-07 0.83  6.9e-07 9.2e-07 1.32  1.4e-06 2.0e-06 1.44  6.1e-07 4.6e-07 0.76  5.6e-08 5.6e-08 0.93
(2, 37, 132, 33)                    8.1e-07 7.8e-07 0.95  4.3e-07 4.2e-07 0.99  5.3e-07 7.2e-07 1.37  7.9e-07 5.3e-07 0.67  5.5e-08 5.5e-08 0.92
(2, 37, 176, 8)                     5.6e-07 3.3e-07 0.59  5.0e-07 4.1e-07 0.83  2.7e-06 1.8e-06 0.66  8.3e-07 5.7e-07 0.69  5.5e-08 5.5e-08 0.92
(2, 37, 192, 8)                     5.8e-07 3.9e-07 0.67  6.5e-07 3.5e-07 0.55  4.3e-06 1.6e-06 0.37  5.8e-07 6.5e-07 1.12  5.7e-08 5.7e-08 0.95
(2, 37, 256, 8)                     5.1e-07 5.7e-07 1.13  7.4e-07 4.6e-07 0.63  9.7e-07 2.3e-06 2.42  9.1e-07 6.7e-07 0.73  5.6e-08 5.6e-08 0.94
(2, 37, 256, 32)                    6.6e-07 6.7e-07 1.02  5.5e-07 6.1e-07 1.09  2.3e-06 2.5e-06 1.07  9.2e-07 8.3e-07 0.90  5.7e-08 5.7e-08 0.95
(2, 37, 180, 4)                     6.3e-07 6.6e-07 1.04  5.6e-07 5.8e-07 1.02  1.5e-06 2.4e-06 1.57  7.4e-07 5.2e-07 0.70  5.4e-08 5.4e-08 0.90
(2, 37, 192, 4)                     4.7e-07 5.1e-07 1.10  9.0e-07 4.3e-07 0.48  2.4e-06 4.9e-06 2.05  5.2e-07 5.1e-07 0.97  5.7e-08 5.7e-08 0.96
(2, 37, 132, 11)                    3.8e-07 3.2e-07 0.85  4.4e-07 4.5e-07 1.03  1.9e-06 2.0e-06 1.08  6.1e-07 4.0e-07 0.67  5.5e-08 5.5e-08 0.92
(2, 37, 160, 8)                     5.1e-07 3.7e-07 0.72  6.1e-07 5.5e-07 0.90  1.2e-06 2.5e-06 2.11  5.7e-07 4.1e-07 0.72  5.7e-08 5.7e-08 0.95
(2, 37, 156, 4)                     4.8e-07 3.5e-07 0.74  7.3e-07 7.0e-07 0.96  9.0e-07 1.5e-06 1.66  7.2e-07 6.7e-07 0.93  5.1e-08 5.1e-08 0.86
(2, 37, 172, 4)                     7.1e-07 5.0e-07 0.70  5.2e-07 3.3e-07 0.64  2.5e-06 4.0e-06 1.63  6.9e-07 6.3e-07 0.92  5.7e-08 5.7e-08 0.96
(1, 19, 512, 32)                    1.0e-06 1.3e-06 1.23  1.6e-06 1.8e-06 1.14  1.0e-05 3.5e-05 3.40  1.0e-06 5.2e-07 0.51  5.7e-08 5.7e-08 0.97
(1, 19, 576, 32)                    1.5e-06 1.2e-06 0.82  1.8e-06 2.0e-06 1.10  7.2e-05 6.7e-05 0.92  8.5e-07 1.3e-06 1.51  5.9e-08 5.9e-08 1.00
(1, 1, 64, 8)                       8.2e-07 6.8e-07 0.83  3.0e-07 1.8e-07 0.60     (rounding bound)   5.3e-07 5.1e-07 0.97  5.8e-08 5.8e-08 0.97
(3, 7, 216, 8)                      3.8e-07 3.5e-07 0.92  3.7e-07 4.6e-07 1.23  1.0e-06 1.7e-06 1.69  3.8e-07 5.8e-07 1.50  5.4e-08 5.4e-08 0.91
(2, 37, 96, 8) spike                2.7e-07 3.1e-07 1.15  7.0e-07 1.4e-06 1.97  3.7e-06 5.0e-06 1.34  6.8e-07 5.2e-07 0.77  4.8e-08 4.8e-08 0.81
(2, 37, 96, 8) constant             4.2e-07 3.2e-07 0.78  4.4e-07 4.2e-07 0.94  1.1e-06 5.5e-06 4.96  5.8e-07 4.1e-07 0.70  5.2e-08 5.2e-08 0.87
(2, 37, 96, 8) shift                3.2e-07 3.3e-07 1.03  3.4e-07 4.5e-07 1.33  1.2e-05 7.1e-06 0.62  4.4e-07 7.8e-07 1.79  5.3e-08 5.3e-08 0.90

attention with the position encoding inside, per case (conv gradients: the worst of the three windows)
(B, H, W, C, heads)                 out                   dq                    dk                    dv                    grad conv weight      grad conv bias
(16, 25, 41, 64, 8)                 9.2e-07 5.7e-07 0.62  7.6e-07 4.0e-07 0.52  9.3e-07 4.6e-07 0.50  7.4e-07 3.4e-07 0.46  1.4e-07 1.1e-07 0.79  4.0e-07 2.1e-07 0.52
(2, 5, 7, 216, 8)                   6.0e-07 4.1e-07 0.69  5.0e-07 7.8e-07 1.56  1.8e-05 8.7e-06 0.48  6.3e-07 7.1e-07 1.12  6.6e-08 9.6e-08 1.44  8.3e-08 1.6e-07 1.90
(1, 2, 3, 64, 8)                    6.7e-07 4.9e-07 0.73  2.7e-07 2.7e-07 1.00  6.8e-05 5.1e-05 0.75  3.8e-07 2.8e-07 0.74  1.0e-07 7.1e-08 0.69  5.4e-08 4.9e-08 0.82

every other operation, per tensor over its cases: eager error, kernel error, the worst kernel / eager and its case
operation                      tensor               cases  eager error         kernel error        worst kernel/eager (case)
fallback                       output                   1  1.2e-06 .. 1.2e-06  1.2e-06 .. 1.2e-06  1.00  fallback (768, 48 heads)
fallback                       grad x                   1  1.7e-06 .. 1.7e-06  1.7e-06 .. 1.7e-06  1.02  fallback (768, 48 heads)
fallback                       parameter gradients     10  6.5e-08 .. 6.8e-07  6.5e-08 .. 6.8e-07  1.14  fallback (768, 48 heads)
dwconv                         y                       15  2.9e-08 .. 5.5e-07  2.9e-08 .. 5.5e-07  1.24  dwconv (2, 32, 128, 8) k=3
dwconv                         grad x                  15  3.4e-08 .. 4.8e-07  3.4e-08 .. 3.5e-07  1.58  dwconv (1, 3, 5, 70) k=3
dwconv                         grad conv weight        15  7.9e-09 .. 2.7e-07  7.9e-09 .. 1.2e-07  1.00  dwconv (2, 7, 9, 130) k=7
dwconv                         grad conv bias          15  8.2e-10 .. 4.7e-07  8.2e-10 .. 1.3e-07  1.67  dwconv (4, 64, 128, 8) k=3
dwconv groups                  y                        2  2.9e-07 .. 3.0e-07  2.9e-07 .. 3.0e-07  1.00  dwconv groups (8,8,8,8) k=(3,5,7,3) add=1
dwconv groups                  grad x                   2  1.8e-07 .. 1.8e-07  1.5e-07 .. 2.3e-07  1.28  dwconv groups (8,8,8,8) k=(3,5,7,3) add=0
dwconv groups                  grad conv weight         8  5.5e-08 .. 9.0e-08  5.5e-08 .. 9.6e-08  1.11  dwconv groups (8,8,8,8) k=(3,5,7,3) add=1
dwconv groups                  grad conv bias           8  5.1e-08 .. 1.6e-07  5.9e-08 .. 1.6e-07  1.46  dwconv groups (8,8,8,8) k=(3,5,7,3) add=1
residual_layernorm             y                       30  3.2e-08 .. 5.9e-08  3.2e-08 .. 5.9e-08  0.99  tokens (1, 5, 1024) residual_layernorm
residual_layernorm             z                       30  8.9e-07 .. 7.8e-05  7.7e-07 .. 8.8e-06  1.04  tokens (1, 5, 4) residual_layernorm
residual_layernorm             grad x                  30  1.1e-07 .. 3.4e-05  6.9e-08 .. 2.4e-05  1.29  tokens (1, 5, 68) residual_layernorm
residual_layernorm             grad branch             30  5.6e-07 .. 4.4e-05  2.4e-07 .. 8.4e-06  2.71  tokens (1, 5, 64) residual_layernorm
residual_layernorm             grad weight             30  2.2e-07 .. 2.4e-05  2.2e-07 .. 2.0e-06  1.13  tokens (1, 5, 1024) residual_layernorm
residual_layernorm             grad bias               30  4.6e-09 .. 4.9e-07  4.6e-09 .. 2.0e-07  1.00  tokens (1, 5, 516) residual_layernorm
layernorm_tokens passthrough   z                       30  1.0e-06 .. 7.8e-05  4.8e-07 .. 2.0e-05  1.02  tokens (1, 5, 128) layernorm_tokens passthrough
layernorm_tokens passthrough   grad x                  30  9.4e-08 .. 1.6e-04  7.7e-08 .. 7.7e-05  1.32  tokens (1, 5, 512) layernorm_tokens passthrough
layernorm_tokens passthrough   grad weight             30  1.2e-07 .. 4.2e-05  1.0e-07 .. 4.2e-06  1.28  tokens grid-stride (16400, 260) layernorm_tokens passthrough
layernorm_tokens passthrough   grad bias               30  4.6e-09 .. 4.9e-07  4.6e-09 .. 2.0e-07  1.00  tokens (1, 5, 516) layernorm_tokens passthrough
residual_add                   y                       30  3.2e-08 .. 5.9e-08  3.2e-08 .. 5.9e-08  0.99  tokens (1, 5, 1024) residual_add
residual_add                   grad branch             30  4.0e-08 .. 6.0e-08  4.0e-08 .. 6.0e-08  1.00  tokens (3, 37, 128) residual_add
linear                         y                       24  4.8e-08 .. 1.2e-05  4.8e-08 .. 1.2e-05  1.00  linear rows=1 cout=260
linear                         grad x                  24  7.0e-08 .. 9.7e-07  7.0e-08 .. 9.7e-07  1.00  linear rows=16400 cout=128
linear                         grad weight             24  1.5e-08 .. 1.3e-06  1.5e-08 .. 1.3e-06  1.00  linear rows=16400 cout=68
linear                         grad bias               24  0.0e+00 .. 2.2e-07  0.0e+00 .. 2.2e-07  2.16  linear rows=16400 cout=68
encoder                        output                   2  3.3e-07 .. 8.4e-07  3.8e-07 .. 8.6e-07  1.15  encoder (64, 3 layers, 6x10)
encoder                        grad x                   2  6.8e-07 .. 1.4e-06  7.6e-07 .. 1.3e-06  1.12  encoder (64, 3 layers, 6x10)
encoder                        parameter gradients     76  5.7e-08 .. 9.9e-07  4.6e-08 .. 1.1e-06  1.74  encoder (176, 2 layers, 5x7)

dk where it is nothing but a cancelled difference is not in the tables: all 64 channels of the one-token case (the
reference is identically 0) and the 24 channels of the spike case that carry the +30 (at the spike token eager returns
exactly 0, an error of 100 %, and the kernel returns rounding noise 4.6e4 times the reference's 1e-13-sized value).  Those
are held to the fp32 rounding bound derived at `_dk_rounding_bound`: worst kernel error / bound 0.077 for one token, 0.197
for the spiked channels.  The 72 unspiked channels of the spike case keep the per-channel measure (dk 1.34 x eager above).

Row form (fa_context_rows_kernel), the case that reaches each CHP, both SOFTMAX forms (forward and backward) of each:
4 (2,37,132,33); 8 (2,37,256,32); 12 (2,37,132,11); 16 (1,19,512,32); 20 (2,37,160,8); 24 (2,37,176,8), (2,37,192,8);
28 (3,7,216,8); 32 (2,37,256,8); 36 (2,37,132,4); 40 (2,37,156,4); 44 (2,37,172,4); 48 (2,37,180,4), (2,37,192,4).
Entry form (fa_context_kernel) MAXO 2 (16,1025,64,8); 8 (2,37,96,8), (2,37,128,8); 24 (2,37,64,1); 48 (2,37,128,2), (1,19,576,32).

Before the LayerNorm forward took its mean in two steps (sum, then the mean of the deviations), grad weight measured
16.8 x eager at tokens (1, 5, 4) and 8.1 x at (3, 37, 4): the one kernel bug these cases found.
"""
import types

import pytest
import torch

import vit_f64_ref as R
from gpu_f64_common import DEV, check as _check, poison as _poison

pytestmark = pytest.mark.gpu
EPS = 1e-6


def _lib():
    from baseboostdepth_amd import ops
    return ops.default_backend().lib


def _params(weight, bias, **more):
    """What the ops read of an nn.Conv2d / nn.LayerNorm / nn.Linear, around leaf tensors of the test's own."""
    return types.SimpleNamespace(weight=weight, bias=bias, **more)


# ------------------------------------------------------------------------------------------------ attention
def _attention_views(C, dk_channels=None):
    """`dk_channels`: the k channels whose dk takes the per-channel measure (None: all of them)."""
    def dk(r):
        t = r[1][:, :, C:2 * C]
        return t if dk_channels is None else t[:, :, dk_channels]
    views = [("out", "channel", lambda r: r[0]), ("dq", "channel", lambda r: r[1][:, :, :C]),
             ("dk", "channel", dk), ("dv", "channel", lambda r: r[1][:, :, 2 * C:])]
    return views if dk_channels is None or len(dk_channels) else views[:2] + views[3:]


def _attention_scratch(B, N, C, Ch):
    return [_lib().factor_att_scratch_floats(B, N, C, Ch), B * C, B * C * Ch, B * N * C, B * N * 3 * C]


ATTENTION_CASES = [
    # entry-per-thread context form (C <= 128)
    (16, 1025, 64, 8, None),      # 64 segments of 17 tokens: segments 61..63 are empty; MAXO 2
    (2, 37, 96, 8, None),         # Ch = 12; MAXO 8
    (2, 37, 128, 8, None),        # MAXO 8, last C of the entry form
    (2, 37, 64, 1, None),         # one head of 64: MAXO 24
    (2, 37, 128, 2, None),        # MAXO 48
    # row-per-thread context form (128 < C <= 512)
    (2, 37, 132, 4, None),        # Ch = 33 -> CHP 36, first C past the switch, 60 idle threads
    (2, 37, 132, 33, None),       # CHP 4
    (2, 37, 176, 8, None),        # MPViT-tiny: Ch = 22 -> CHP 24
    (2, 37, 192, 8, None),        # MPViT-xsmall: CHP 24
    (2, 37, 256, 8, None),        # MPViT-xsmall: CHP 32
    (2, 37, 256, 32, None),       # CHP 8
    (2, 37, 180, 4, None),        # Ch = 45 -> CHP 48, three pad lanes
    (2, 37, 192, 4, None),        # CHP 48 without padding
    (2, 37, 132, 11, None),       # CHP 12
    (2, 37, 160, 8, None),        # CHP 20
    (2, 37, 156, 4, None),        # Ch = 39 -> CHP 40, one pad lane
    (2, 37, 172, 4, None),        # Ch = 43 -> CHP 44, one pad lane
    # largest accepted
    (1, 19, 512, 32, None),       # CHP 16; row-form LDS exactly 65 536 B
    (1, 19, 576, 32, None),       # entry form, 73 728 B: the first shape whose forward needs the opt-in
    # few tokens
    (1, 1, 64, 8, None),
    (3, 7, 216, 8, None),         # MPViT-small: Ch = 27 -> CHP 28
    # inputs that strain the softmax
    (2, 37, 96, 8, "spike"),
    (2, 37, 96, 8, "constant"),
    (2, 37, 96, 8, "shift"),
]


@pytest.mark.parametrize("B,N,C,heads,variant", ATTENTION_CASES)
def test_factorised_attention_against_float64(B, N, C, heads, variant):
    from baseboostdepth_amd import ops
    assert ops.factor_attention_supported(C, heads)
    Ch = C // heads
    scale = Ch ** -0.5
    gen = torch.Generator().manual_seed(1000 * C + N + heads)
    qkv, convv, gout, altered = R.attention_inputs(gen, B, N, C, variant, with_channels=True)
    # where dk is (almost) nothing but a cancelled difference - every channel of one token, the channels that carry a
    # spike - it is held to _dk_rounding_bound; every other channel keeps the per-channel measure
    cancelled = torch.arange(C) if N == 1 else altered.sort().values if variant == "spike" else altered[:0]
    measured = torch.tensor(sorted(set(range(C)) - set(cancelled.tolist())), dtype=torch.long)
    views = _attention_views(C, measured if len(cancelled) else None) + [("grad convv", "channel", lambda r: r[2])]
    case = "attention %s%s" % ((B, N, C, heads), " " + variant if variant else "")
    got, ref = _check(case, lambda a, c: ops.factor_attention(a, c, heads, scale), lambda a, c: R.factor_attention(a, c, heads, scale),
                      [qkv, convv], [], [gout], views, _attention_scratch(B, N, C, Ch))
    if len(cancelled):
        err = (got[1][:, :, C:2 * C].double().cpu() - ref[1][:, :, C:2 * C]).abs()
        worst = float((err / _dk_rounding_bound(qkv, gout, heads, scale))[:, :, cancelled].max())
        print("F64 | %s | dk of %d cancelled channels / rounding bound | - | %.2e | -" % (case, len(cancelled), worst))
        assert worst <= 1.0, worst


def _dk_rounding_bound(qkv, gout, heads, scale):
    """Element-wise bound on |dk - dk64| from fp32 rounding alone, for the channels whose dk the relative measure cannot
    judge: one token (softmax = 1, dk is identically zero: no denominator) and a +30 spike in k (at the spike token
    p = 1 - 1e-13 and dk = p (a - r) with a - r ~ 1e-13 |a|: eager returns exactly 0 there, 100 % off, and 8 x that asks
    for twelve digits of a difference of two fp32 sums).
    dk[n,x] = p[n,x] (a[n,x] - r[x]),  a = sum_j v[n,j] D[x,j],  r = sum_j ctx[x,j] D[x,j] / scale,  in float64 below.
    Roundings on the way, each at most 2^-24 of T = sum_j |v[n,j]| Dabs[x,j] + sum_j ctxabs[x,j] Dabs[x,j] / scale, where
    Dabs = scale sum_n |q g| and ctxabs = scale sum_n p |v| are the sums of the absolute terms (the textbook bound of
    an fp32 sum is relative to those, not to a result that may itself have cancelled):
      the two chains of Ch multiply-adds (2 Ch); ctx and D as sums over the N tokens, in whatever order (N); scale and
      1 / scale on ctx, D and r, the subtraction, the product with p, p's own exp / reciprocal / product (8); the fp32
      argument of the hardware exp, |k - kmax| 2^-24 relative in p.
    Bound: (2 Ch + N + 8 + |k - kmax|) 2^-24 p T.  A dropped token or channel is off by about T / N.
    Measured: kernel / bound = 0.077 for one token, 0.197 over the 24 spiked channels of the spike case."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    Ch = C // heads
    q, k, v = [t.reshape(B, N, heads, Ch) for t in qkv.double().split(C, dim=2)]
    g = gout.double().reshape(B, N, heads, Ch)
    p = k.softmax(dim=1)
    Dabs = scale * torch.einsum("bnhk,bnhv->bhkv", q.abs(), g.abs())
    ctxabs = scale * torch.einsum("bnhk,bnhv->bhkv", p, v.abs())
    T = torch.einsum("bnhv,bhkv->bnhk", v.abs(), Dabs) + ((ctxabs * Dabs).sum(-1) / scale)[:, None]
    count = 2 * Ch + N + 8 + (k.amax(dim=1, keepdim=True) - k)
    return (count * 2.0 ** -24 * p * T).reshape(B, N, C)


def test_unsupported_attention_shape_takes_the_eager_path(monkeypatch):
    """dim 768 with 48 heads (C * Ch = 12 288, but 184 320 B of LDS in the backward): the predicate refuses it, the block
    computes the attention with torch ops and matches float64 instead of failing in a launch."""
    from baseboostdepth_amd import ops
    from baseboostdepth_amd.networksvit.mpvit import FactorAtt_ConvRelPosEnc, ConvRelPosEnc
    assert not ops.factor_attention_supported(768, 48)
    B, H, W, C, heads = 2, 3, 4, 768, 48
    torch.manual_seed(7)
    att = FactorAtt_ConvRelPosEnc(C, num_heads=heads, qkv_bias=True, shared_crpe=ConvRelPosEnc(C // heads, heads, {3: 12, 5: 18, 7: 18}))
    with torch.no_grad():
        att.qkv.weight.mul_(4.0)
    _module_case("fallback (768, 48 heads)", att, B, H, W, C, monkeypatch, channels_last=False)


# ------------------------------------------------------------------------------------------------ attention + position encoding
@pytest.mark.parametrize("B,H,W,C,heads", [(16, 25, 41, 64, 8), (2, 5, 7, 216, 8), (1, 2, 3, 64, 8)])
def test_attention_with_position_encoding_against_float64(B, H, W, C, heads):
    """`factor_attention_crpe`: the v third of grad qkv receives the attention's dv and the convolutions' data gradient
    (`add_input & 2`); the convolution parameters' gradients come from the grouped weight-gradient launch."""
    from baseboostdepth_amd import ops
    N, Ch = H * W, C // heads
    scale = Ch ** -0.5
    gen = torch.Generator().manual_seed(C + N)
    qkv, _, gout = R.attention_inputs(gen, B, N, C)
    splits, ks = [2 * Ch, 3 * Ch, 3 * Ch], [3, 5, 7]
    ws, bs = R.conv_params(gen, splits, ks)
    n = len(splits)

    def kernel(a, *p):
        return ops.factor_attention_crpe(a, (H, W), [_params(w, b) for w, b in zip(p[:n], p[n:])], heads, scale)

    def formula(a, *p):
        return R.factor_attention_crpe(a, (H, W), p[:n], p[n:], heads, scale)
    views = _attention_views(C)
    for i, k in enumerate(ks):
        views += [("grad w%d" % k, "tensor", lambda r, i=i: r[2 + i]), ("grad b%d" % k, "tensor", lambda r, i=i: r[2 + n + i])]
    wgrad = _lib().dwconv_groups_wgrad_scratch_floats(B, H, W, n, ops._i32_array(splits), ops._i32_array(ks))
    _check("attention+crpe %s" % ((B, H, W, C, heads),), kernel, formula, [qkv] + ws + bs, [], [gout], views,
           _attention_scratch(B, N, C, Ch) + [wgrad])


# ------------------------------------------------------------------------------------------------ depth-wise convolution
def _dwconv_case(case, B, H, W, splits, ks, add, sliced):
    from baseboostdepth_amd import ops
    C, n = sum(splits), len(splits)
    gen = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + C + ks[0])
    width = 3 * C if sliced else C
    x = R.rounded(R.draw(gen, B, H * W, width) * R.channel_scales(gen, width, 10.0))
    gy = R.rounded(R.draw(gen, B, H * W, C) * R.channel_scales(gen, C, 10.0))
    ws, bs = R.conv_params(gen, splits, ks)
    cut = (lambda t: t[:, :, 2 * C:]) if sliced else (lambda t: t)          # the "v" third of qkv-like rows, read in place

    def kernel(t, *p):
        return ops.dwconv_tokens(cut(t), (H, W), [_params(w, b) for w, b in zip(p[:n], p[n:])], add_input=add)

    def formula(t, *p):
        return R.dwconv_tokens(cut(t), (H, W), p[:n], p[n:], add_input=add)
    views = [("y", "channel", lambda r: r[0]), ("grad x", "channel", lambda r: cut(r[1]))]
    for i, k in enumerate(ks):
        views += [("grad w%d.%d" % (k, i), "tensor", lambda r, i=i: r[2 + i]), ("grad b%d.%d" % (k, i), "tensor", lambda r, i=i: r[2 + n + i])]
    lib = _lib()
    wgrad = (lib.dwconv_groups_wgrad_scratch_floats(B, H, W, n, ops._i32_array(splits), ops._i32_array(ks)) if n > 1
             else lib.dwconv_wgrad_scratch_floats(B, H, W, C, ks[0]))
    got, _ = _check(case, kernel, formula, [x] + ws + bs, [], [gy], views, [wgrad, B * H * W * C])
    if sliced:
        assert not bool(got[1][:, :, :2 * C].any())          # nothing lands outside the slice


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("B,H,W,C", [
    (2, 1, 1, 5),           # one pixel: only the centre tap sees data
    (1, 3, 5, 70),          # W no multiple of 4 or 8, a second channel tile of 6
    (2, 7, 9, 130),         # a third channel tile of 2
    (2, 32, 128, 8),        # 1024 row segments: the weight gradient's partial rows reach WGRAD_MAX_ROWS, one segment per lane
    (4, 64, 128, 8),        # 4096 row segments: every lane strides over four
])
def test_depthwise_token_convolution_against_float64(B, H, W, C, k):
    _dwconv_case("dwconv %s k=%d" % ((B, H, W, C), k), B, H, W, [C], [k], add=(k == 3), sliced=False)


@pytest.mark.parametrize("add", [False, True])
def test_four_channel_groups_in_one_launch_against_float64(add):
    _dwconv_case("dwconv groups (8,8,8,8) k=(3,5,7,3) add=%d" % add, 2, 5, 7, [8, 8, 8, 8], [3, 5, 7, 3], add=add, sliced=True)


# ------------------------------------------------------------------------------------------------ LayerNorm / residual
def _layernorm_case(case, B, N, C, mask, constant_rows=()):
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(B * 100000 + N * 10 + C)
    x, branch, weight, bias, gy, gz = R.layernorm_inputs(gen, B, N, C, constant_rows)
    lib = _lib()
    scratch = [lib.token_ln_scratch_floats(B * N, C), 2 * B * N, B * N * C, C]
    y_z = [("y", "channel", lambda r: r[0]), ("z", "row", lambda r: r[1])]
    _check(case + " residual_layernorm",
           lambda t, br, w, b, m: ops.residual_layernorm(t, br, m, _params(w, b, eps=EPS)),
           lambda t, br, w, b, m: R.residual_layernorm(t, br, m, w, b, EPS), [x, branch, weight, bias], [mask], [gy, gz],
           y_z + [("grad x", "row", lambda r: r[2]), ("grad branch", "channel", lambda r: r[3]),
                  ("grad weight", "tensor", lambda r: r[4]), ("grad bias", "tensor", lambda r: r[5])], scratch)
    params = [("grad x", "row", lambda r: r[-3]), ("grad weight", "tensor", lambda r: r[-2]), ("grad bias", "tensor", lambda r: r[-1])]
    _check(case + " layernorm_tokens passthrough",
           lambda t, w, b: ops.layernorm_tokens(t, _params(w, b, eps=EPS), passthrough=True),
           lambda t, w, b: R.residual_layernorm(t, None, None, w, b, EPS), [x, weight, bias], [], [gy, gz], y_z + params, scratch)
    _check(case + " layernorm_tokens",
           lambda t, w, b: ops.layernorm_tokens(t, _params(w, b, eps=EPS)),
           lambda t, w, b: R.residual_layernorm(t, None, None, w, b, EPS)[1], [x, weight, bias], [], [gz],
           [("z", "row", lambda r: r[0])] + params, scratch)
    _check(case + " residual_add", lambda t, br, m: ops.residual_add(t, br, m), lambda t, br, m: R.residual_add(t, br, m),
           [x, branch], [mask], [gy],
           [("y", "channel", lambda r: r[0]), ("grad x", "channel", lambda r: r[1]), ("grad branch", "channel", lambda r: r[2])], scratch)


# 4: one float4; 64 / 128 / 256 / 512 / 1024: the lane groups (16 / 32 / 64 lanes, 1 / 2 / 4 float4 per lane) exactly full;
# 68, 96, 132, 176, 192, 260, 516: partly filled
@pytest.mark.parametrize("C", [4, 64, 68, 96, 128, 132, 176, 192, 256, 260, 512, 516, 1024])
@pytest.mark.parametrize("B,N", [(3, 37), (1, 5)])
def test_layernorm_and_residual_widths_against_float64(B, N, C):
    mask = torch.tensor([0.0, 1.25, 1.25]) if B == 3 else torch.tensor([1.25])
    _layernorm_case("tokens %s" % ((B, N, C),), B, N, C, mask)


@pytest.mark.parametrize("rows,C", [
    (65552, 64),        # 4097 workgroups' worth of rows (16 per workgroup): the forward's grid is capped at 4096 and strides
    (32776, 96),        # the same with 32 lanes per row (8 rows per workgroup)
    (16400, 260),       # 64 lanes per row, 4100 workgroups' worth; rows * C > 4 Mi: the backward's grid sits at its 1024 cap
])
def test_layernorm_grid_stride_against_float64(rows, C):
    B = 8
    mask = torch.tensor([1.25, 0.0, 1.25, 1.25, 1.25, 0.0, 1.25, 1.25])
    _layernorm_case("tokens grid-stride %s" % ((rows, C),), B, rows // B, C, mask)


def test_layernorm_of_constant_rows_against_float64():
    """Two rows hold 50 in every channel: the mean must come out as exactly 50 (the kernel forms it as sum * (1 / C)), or
    rstd = eps^-1/2 = 1000 multiplies the residue into z, where eager gives the bias exactly."""
    _layernorm_case("tokens constant rows (2, 9, 260)", 2, 9, 260, torch.tensor([1.25, 1.25]), constant_rows=[(0, 3), (1, 8)])


# ------------------------------------------------------------------------------------------------ column sum
@pytest.mark.parametrize("rows", [1, 3, 70, 16400])
@pytest.mark.parametrize("cout", [4, 64, 68, 128, 132, 260])          # 16 / 32 / 64 column lanes, each full and partly filled
def test_linear_bias_gradient_by_column_sum_against_float64(rows, cout):
    from baseboostdepth_amd import ops
    cin = 8
    gen = torch.Generator().manual_seed(rows + cout)
    x = R.rounded(R.draw(gen, 1, rows, cin))
    weight, bias = R.rounded(R.draw(gen, cout, cin) / 3.0), R.rounded(R.draw(gen, cout))
    g = R.rounded(R.draw(gen, 1, rows, cout) * R.channel_scales(gen, cout, 10.0) + 10.0)          # per-column offset of 10
    _check("linear rows=%d cout=%d" % (rows, cout),
           lambda t, w, b: ops.linear_tokens(t, _params(w, b, out_features=cout)), R.linear, [x, weight, bias], [], [g],
           [("y", "channel", lambda r: r[0]), ("grad x", "channel", lambda r: r[1]), ("grad weight", "tensor", lambda r: r[2]),
            ("grad bias", "tensor", lambda r: r[3])], [_lib().colsum_scratch_floats(rows, cout), cout])


# ------------------------------------------------------------------------------------------------ whole modules
def _module_case(case, module, B, H, W, C, monkeypatch, channels_last):
    """A module of networksvit.mpvit on GPU tokens with the fused paths on, against its float64 copy on the CPU; the
    yardstick is the same module with the fused paths off.  Output, grad x and every parameter gradient."""
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(C + H)
    with torch.no_grad():
        for p in module.parameters():                      # non-trivial LayerNorm / bias values
            p.add_(R.rounded(0.05 * R.draw(gen, *p.shape)))
    x = R.rounded(R.draw(gen, B, H * W, C))
    up = R.rounded(R.draw(gen, B, H * W, C) * R.channel_scales(gen, C, 10.0))
    names = ["output", "grad x"] + [n for n, _ in module.named_parameters()]
    kinds = ["channel", "channel"] + ["tensor"] * (len(names) - 2)

    def run(mod, device, dtype, fused):
        monkeypatch.setattr(ops, "FUSED_NN", fused)
        monkeypatch.setattr(ops, "FUSED_TOKEN_GLUE", fused)
        t = x.to(device=device, dtype=dtype).clone().requires_grad_(True)
        for p in mod.parameters():
            p.grad = None
        y = mod(t, (H, W))
        if channels_last:                                   # [B, C, H, W] feature map -> tokens
            y = y.permute(0, 2, 3, 1).reshape(B, H * W, C)
        (y * up.to(device=device, dtype=dtype)).sum().backward()
        return [y.detach(), t.grad] + [p.grad.clone() for p in mod.parameters()]
    ref = run(R.float64_copy(module), "cpu", torch.float64, False)
    module = module.to(DEV)
    with torch.backends.cudnn.flags(enabled=False):
        eager = run(module, DEV, torch.float32, False)
    got = run(module, DEV, torch.float32, True)
    again = run(module, DEV, torch.float32, True)
    _poison([t.numel() for t in got] + [B * H * W * 3 * C, 2 * B * H * W])
    third = run(module, DEV, torch.float32, True)
    failures = []
    for name, kind, r, e, g, g2, g3 in zip(names, kinds, ref, eager, got, again, third):
        if not (torch.equal(g, g2) and torch.equal(g, g3)):
            failures.append((name, "differs between calls"))
        e_err, k_err = R.group_error(e, r, kind), R.group_error(g, r, kind)
        print("F64 | %s | %s | %.2e | %.2e | %.2f" % (case, name, e_err, k_err, k_err / max(e_err, 2.0 ** -24)))
        if not k_err <= R.bound(e_err):
            failures.append((name, "eager %.3e kernel %.3e bound %.3e" % (e_err, k_err, R.bound(e_err))))
    assert not failures, (case, failures)


@pytest.mark.parametrize("dim,layers,H,W", [(64, 3, 6, 10), (176, 2, 5, 7)])
def test_encoder_path_with_fused_glue_against_its_float64_copy(dim, layers, H, W, monkeypatch):
    """MHCAEncoder with every fusion on: the blocks share their position encodings, so their weight-gradient launches add
    into one buffer per parameter (`accumulate = 1`) - the only case that exercises it against an independent reference."""
    from baseboostdepth_amd.networksvit.mpvit import MHCAEncoder
    torch.manual_seed(dim + layers)
    enc = MHCAEncoder(dim, num_layers=layers, num_heads=8, mlp_ratio=4, drop_path_list=[0.0] * layers)
    _module_case("encoder (%d, %d layers, %dx%d)" % (dim, layers, H, W), enc, 2, H, W, dim, monkeypatch, channels_last=True)
