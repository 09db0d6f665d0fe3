"""References for the MonoViT token kernels (csrc/bbd_vit.hip, csrc/bbd_tokens.hip): every operation as plain torch
ops, written from its formula.  The functions take whatever dtype / device their arguments have: on float64 CPU
tensors they are the reference, on fp32 tensors they are the eager formulation a kernel replaces (the yardstick of
its rounding error).  Gradients come from autograd.

The measure (`group_error`): max |T - T64| over a group divided by max |T64| over the same group, then the maximum
over the groups - per channel for activations and their gradients, per row for LayerNorm's z and grad x, per tensor
for parameter gradients.  No group may be empty or all-zero.  A kernel passes when its error is at most FACTOR times
the eager fp32 error of the same tensor on the same inputs, with a floor of FACTOR * 2^-24 (`bound`)."""
import copy

import torch
import torch.nn.functional as F

FACTOR = 8.0
FLOOR = FACTOR * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the operations
def factor_attention(qkv, convv, heads, scale):
    """out = scale * q (softmax_N(k)^T v) + q * convv per head; qkv [B, N, 3C] = q | k | v with head-major channels."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    Ch = C // heads
    q, k, v = qkv.reshape(B, N, 3, heads, Ch).permute(2, 0, 3, 1, 4)          # each [B, h, N, Ch]
    context = torch.einsum("bhnk,bhnv->bhkv", k.softmax(dim=2), v)            # softmax over the N tokens
    att = torch.einsum("bhnk,bhkv->bhnv", q, context)
    out = scale * att + q * convv.reshape(B, N, heads, Ch).transpose(1, 2)
    return out.transpose(1, 2).reshape(B, N, C)


def dwconv_tokens(x, size, weights, biases, add_input=False):
    """Depth-wise convolutions (one (weight [n,1,k,k], bias [n]) per consecutive channel group, zero padding k // 2)
    of the tokens [B, H*W, C] viewed as an NCHW image, optionally + x."""
    B, N, C = x.shape
    img = x.reshape(B, size[0], size[1], C).permute(0, 3, 1, 2)
    parts = torch.split(img, [w.shape[0] for w in weights], dim=1)
    out = torch.cat([F.conv2d(p, w, b, 1, w.shape[-1] // 2, 1, w.shape[0]) for p, w, b in zip(parts, weights, biases)], 1)
    if add_input:
        out = out + img
    return out.permute(0, 2, 3, 1).reshape(B, N, C)


def factor_attention_crpe(qkv, size, weights, biases, heads, scale):
    """The attention with convv = the depth-wise convolutions of its own v third."""
    C = qkv.shape[-1] // 3
    return factor_attention(qkv, dwconv_tokens(qkv[:, :, 2 * C:], size, weights, biases), heads, scale)


def residual_add(x, branch, mask):
    """x + branch * mask[b]  (`mask` [B]: the stochastic-depth scale, 0 or 1 / keep; None = 1)."""
    return x + (branch if mask is None else branch * mask.reshape(-1, 1, 1))


def residual_layernorm(x, branch, mask, weight, bias, eps):
    """(y, LayerNorm(y)) with y = x + branch * mask[b], or y = x for `branch is None`."""
    y = x if branch is None else residual_add(x, branch, mask)
    return y, F.layer_norm(y, (y.shape[-1],), weight, bias, eps)


def linear(x, weight, bias):
    return F.linear(x, weight, bias)


def float64_copy(module):
    """The module itself in float64 on the CPU (the modules take their eager path on CPU tensors)."""
    return copy.deepcopy(module).double().cpu()


# ------------------------------------------------------------------------------------------------ inputs
def draw(gen, *shape):
    """Standard normal values drawn in float64 (CPU generator) - scale / shift them, then `rounded` once."""
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def channel_scales(gen, C, base, lo=-2.0, hi=2.0):
    """[C] per-channel scales base ** U(lo, hi): a large channel cannot hide a wrong small one from a per-channel measure."""
    return base ** (lo + (hi - lo) * torch.rand(C, generator=gen, dtype=torch.float64))


def rounded(t):
    """Float64 values -> fp32 once: reference and kernel then see identical numbers."""
    return t.float()


def attention_inputs(gen, B, N, C, variant=None, with_channels=False):
    """(qkv [B,N,3C], convv [B,N,C], upstream gradient [B,N,C]) as fp32 (`with_channels`: and the k channels the variant altered): q, v, convv and the gradient with channel scales
    10^U(-2,2), k with 2^U(-2,2) (a wider k scale makes the softmax one-hot and measures cancellation, not the kernel).
    `variant`: "spike" = +30 on one token per (image, channel) in a quarter of the k channels; "constant" = four constant
    k columns; "shift" = +80 on all of k in four channels (overflows without the maximum subtracted)."""
    q = draw(gen, B, N, C) * channel_scales(gen, C, 10.0)
    k = draw(gen, B, N, C) * channel_scales(gen, C, 2.0)
    v = draw(gen, B, N, C) * channel_scales(gen, C, 10.0)
    chans = torch.empty(0, dtype=torch.long)
    if variant == "spike":
        chans = torch.randperm(C, generator=gen)[:C // 4]
        tok = torch.randint(0, N, (B, len(chans)), generator=gen)
        for b in range(B):
            k[b, tok[b], chans] += 30.0
    elif variant == "constant":
        chans = torch.randperm(C, generator=gen)[:4]
        k[:, :, chans] = draw(gen, B, 1, 4)
    elif variant == "shift":
        chans = torch.randperm(C, generator=gen)[:4]
        k[:, :, chans] += 80.0
    else:
        assert variant is None
    convv = draw(gen, B, N, C) * channel_scales(gen, C, 10.0)
    gout = draw(gen, B, N, C) * channel_scales(gen, C, 10.0)
    inputs = rounded(torch.cat([q, k, v], dim=2)), rounded(convv), rounded(gout)
    return inputs + (chans,) if with_channels else inputs


def conv_params(gen, splits, ks):
    """Depth-wise (weights, biases) for the channel groups `splits` with windows `ks`, fp32."""
    ws = [rounded(draw(gen, n, 1, k, k) / k) for n, k in zip(splits, ks)]
    bs = [rounded(0.5 * draw(gen, n)) for n in splits]
    return ws, bs


def layernorm_inputs(gen, B, N, C, constant_rows=()):
    """(x, branch, weight, bias, upstream gy, upstream gz) as fp32: x carries a row offset N(0, 50^2) (the mean is far
    from zero, the spread is 1), the gradients channel scales 10^U(-2,2).  `constant_rows`: rows (b, n) of x + branch
    that hold 50 in every channel (variance exactly 0, rstd = eps^-1/2)."""
    x = draw(gen, B, N, C) + 50.0 * draw(gen, B, N, 1)
    branch = draw(gen, B, N, C)
    for b, n in constant_rows:
        x[b, n] = 50.0
        branch[b, n] = 0.0
    weight = 1.0 + 0.5 * draw(gen, C)
    bias = 0.2 * draw(gen, C)
    gy = draw(gen, B, N, C) * channel_scales(gen, C, 10.0)
    gz = draw(gen, B, N, C) * channel_scales(gen, C, 10.0)
    return tuple(rounded(t) for t in (x, branch, weight, bias, gy, gz))


# ------------------------------------------------------------------------------------------------ running and measuring
def forward_backward(fn, leaves, consts, upstream, device, dtype):
    """fn(*leaves, *consts) -> a tensor or a tuple of tensors, on `device` in `dtype`; the loss is sum(out_i * upstream_i).
    Returns the outputs followed by the gradients of the leaves (None leaves / consts pass through as None)."""
    def put(t):
        return t.to(device=device, dtype=dtype) if torch.is_tensor(t) and t.is_floating_point() else t
    xs = [None if t is None else put(t).detach().clone().requires_grad_(True) for t in leaves]
    outs = fn(*xs, *[[put(u) for u in c] if isinstance(c, (list, tuple)) else put(c) for c in consts])
    outs = outs if isinstance(outs, tuple) else (outs,)
    loss = sum((o * put(u)).sum() for o, u in zip(outs, upstream))
    grads = torch.autograd.grad(loss, [x for x in xs if x is not None])
    grads = iter(grads)
    return [o.detach() for o in outs] + [None if x is None else next(grads) for x in xs]


def group_error(got, ref, kind):
    """The measure of the module docstring; `kind`: "channel" (groups = last axis), "row" (groups = all the other axes)
    or "tensor".  A NaN anywhere gives NaN, which fails every comparison."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff, mag = (got - ref).abs(), ref.abs()
    if kind == "channel":
        num, den = diff.reshape(-1, ref.shape[-1]).amax(0), mag.reshape(-1, ref.shape[-1]).amax(0)
    elif kind == "row":
        num, den = diff.amax(-1).reshape(-1), mag.amax(-1).reshape(-1)
    else:
        assert kind == "tensor"
        num, den = diff.max().reshape(1), mag.max().reshape(1)
    assert den.numel() > 0 and bool((den > 0).all()), "a group of the reference is all zero: it would be skipped"
    if bool(torch.isnan(num).any()):
        return float("nan")
    return float((num / den).max())


def bound(eager_error):
    return max(FACTOR * eager_error, FLOOR)
