"""References for the encoder / decoder glue kernels (csrc/bbd_nn.hip): every operation as plain torch ops, written from
its formula.  Like tests/vit_f64_ref.py the functions take whatever dtype / device their arguments have: on float64 CPU
tensors they are the reference, on fp32 tensors the eager yardstick.  Gradients come from autograd.

The measure is vit_f64_ref's: activations and their gradients per channel (NCHW's channel axis moved last, `nhwc`),
parameter gradients and running statistics per tensor, a kernel passes at `bound(eager error)`, no group all zero.

ReLU: fp32 and float64 disagree on the sign of a pre-activation z near 0, so
  forward   y = relu(z) is continuous and measured as usual;
  mask      with tau_c = bound(eager error of z in channel c) * max |z64| over channel c, the kernel's mask y_kernel > 0
            must equal z64 > 0 wherever |z64| > tau_c (`mask_report`); at most NEAR_TIE_CAP of a case's elements may lie
            inside |z64| <= tau_c;
  backward  reference and yardstick differentiate z * M with M = the kernel's own mask held constant (`mask=` of
            `batch_norm_act`), so that a near-tie cannot leak into the gradients."""
import torch
import torch.nn.functional as F

from vit_f64_ref import draw, rounded, channel_scales, forward_backward, group_error, bound, FACTOR, FLOOR  # noqa: F401
from vit_f64_ref import float64_copy  # noqa: F401

NEAR_TIE_CAP = 0.01
MOMENTUM, EPS = 0.1, 1e-5
BATCHES_BEFORE = 5

# launch constants of csrc/bbd_nn.hip, for the path predicates below
BN_SMALL_ELEMS = 8192
MAX_SPLIT = 64


# ------------------------------------------------------------------------------------------------ the operations
def batch_norm_act(x, w, b, res, rm, rv, momentum, eps, relu, rows=None, tracked=None, mask=None):
    """Training-mode BatchNorm2d (+ res) (+ ReLU) with statistics per call group: samples are split into consecutive
    groups of rows[g] (None: one group; a group may be empty), each normalised with its own biased variance.  The running
    statistics take one momentum update per group, in group order, for the first `tracked` groups (None: all), with the
    unbiased variance.  `mask` (bool, y's shape): y keeps the value relu(z) and gets the gradient of z * mask.
    Returns (y, running_mean, running_var, num_batches_tracked, z) - the statistics as new tensors."""
    N, C = x.shape[:2]
    rows = [N] if rows is None else list(rows)
    assert sum(rows) == N
    tracked = len(rows) if tracked is None else tracked
    zs, lo = [], 0
    for g, n in enumerate(rows):
        xg = x[lo:lo + n]
        lo += n
        if n == 0:
            zs.append(xg)
            continue
        cnt = n * xg.shape[2] * xg.shape[3]
        mean = xg.sum(dim=(0, 2, 3), keepdim=True) / cnt
        var = ((xg - mean) ** 2).sum(dim=(0, 2, 3), keepdim=True) / cnt
        zs.append((xg - mean) / torch.sqrt(var + eps) * w.reshape(1, C, 1, 1) + b.reshape(1, C, 1, 1))
        if g < tracked and rm is not None:
            unbiased = var.detach().reshape(C) * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
            rm = (1.0 - momentum) * rm + momentum * mean.detach().reshape(C)
            rv = (1.0 - momentum) * rv + momentum * unbiased
    z = torch.cat(zs)
    if res is not None:
        z = z + res
    y = z
    if relu:
        y = torch.relu(z)
        if mask is not None:
            zm = z * mask.to(device=z.device, dtype=z.dtype)
            y = y.detach() + (zm - zm.detach())
    return y, rm, rv, torch.tensor(BATCHES_BEFORE + tracked), z


def _reflect_index(n, device):
    i = torch.arange(-1, n + 1, device=device).abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def reflect_pad1(x):
    """out[.., py, px] = x[.., r(py - 1), r(px - 1)], r(i) = |i| below n and 2 (n - 1) - i from n on."""
    H, W = x.shape[-2:]
    return x[..., _reflect_index(H, x.device), :][..., _reflect_index(W, x.device)]


def maxpool3s2(x):
    """MaxPool2d(3, 2, 1) by ATen's rule: the window's in-image positions are scanned in row-major order, a value
    replaces the running maximum when it is greater or NaN - so the first maximum wins and a NaN sticks.  The output
    is gathered from the winning position, which is where autograd sends the gradient."""
    H, W = x.shape[-2:]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (1, 2, 1, 2), value=0.0)
    inside = F.pad(torch.ones(H, W, dtype=torch.bool, device=x.device), (1, 2, 1, 2), value=False)
    wins, valid = [], []
    for dy in range(3):
        for dx in range(3):
            wins.append(xp[..., dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
            valid.append(inside[dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
    stack = torch.stack(wins)
    best = stack[0].detach().clone()
    idx = torch.full(best.shape, -1, dtype=torch.long, device=x.device)
    for k in range(9):
        v = stack[k].detach()
        take = valid[k] & ((idx < 0) | (v > best) | torch.isnan(v))
        best = torch.where(take, v, best)
        idx = torch.where(take, torch.full_like(idx, k), idx)
    assert bool((idx >= 0).all())
    return torch.gather(stack, 0, idx[None])[0]


def upcat_pad(x, skip=None):
    """ReflectionPad2d(1)(cat(nearest x2 of x, skip))."""
    u = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return reflect_pad1(u if skip is None else torch.cat([u, skip], 1))


def bias_elu(v, bias):
    """ELU(v + bias[c]), alpha = 1: z for z > 0, exp(z) - 1 otherwise (as expm1: exp(z) - 1 has no digits left at small z)."""
    z = v + bias.reshape(1, -1, 1, 1)
    return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0)))


def dispconv(x, weight, bias):
    """Reflection pad, 3x3 convolution to one channel, bias."""
    return F.conv2d(reflect_pad1(x), weight, bias)


# ------------------------------------------------------------------------------------------------ launch paths
def pick_split(N, HW):
    s = min(max((N * HW + 4095) // 4096, 1), MAX_SPLIT)
    return min(s, (HW + 3) // 4)


def bn_path(shape, rows=None):
    """What the launch code does with this shape: (one launch?, vector layout?, slices of the largest group, how the
    split came about: "one" / "several" / "capped" / "plane")."""
    N, C, H, W = shape
    HW, biggest = H * W, max(rows) if rows else N
    raw = max((biggest * HW + 4095) // 4096, 1)
    split = pick_split(biggest, HW)
    how = "plane" if split < min(raw, MAX_SPLIT) else "capped" if raw > MAX_SPLIT else "one" if split == 1 else "several"
    return biggest * HW <= BN_SMALL_ELEMS, HW % 4 == 0, split, how


# ------------------------------------------------------------------------------------------------ cases
BN_SHAPES = [(2, 5, 1, 3), (3, 7, 5, 9), (4, 6, 8, 16), (2, 4, 48, 64), (2100, 3, 1, 2), (3, 5, 40, 72), (3, 5, 37, 79)]
BN_CAPPED = (4, 2, 256, 260)
BN_VARIANT_SHAPES = [(3, 7, 5, 9), (4, 6, 8, 16), (3, 5, 40, 72), (3, 5, 37, 79), BN_CAPPED]
BN_CONSTANT_SHAPES = [(4, 6, 8, 16), (3, 5, 37, 79)]


def bn_cases():
    """(shape, variant, residual, relu) of every single-group BatchNorm case of the GPU tier."""
    cases = [(s, "plain", res, relu) for s in BN_SHAPES for res in (False, True) for relu in (False, True)]
    cases.append((BN_CAPPED, "plain", False, True))
    for variant in ("offset", "outlier_first"):
        cases += [(s, variant, s != BN_CAPPED and i % 2 == 1, True) for i, s in enumerate(BN_VARIANT_SHAPES)]
    cases += [(s, "constant", res, True) for s in BN_CONSTANT_SHAPES for res in (False, True)]
    return cases


# (shape, rows, trailing padding groups, residual, relu) through ops.bn_call_groups
BN_GROUPED_CASES = [
    ((12, 6, 4, 10), [5, 3, 4], 0, True, True),
    ((7, 4, 30, 50), [1, 6], 0, False, True),          # two launches sized by group 1 (3 slices); group 0 has one
    ((16, 6, 4, 10), [5, 3, 4, 4], 1, False, True),
]
# (shape, rows, tracked, largest group handed to the launch) through ops.bn_call_groups_device
BN_DEVICE_CASE = ((9, 5, 6, 10), [3, 4, 0, 2], 2, 4)

REFLECT_SHAPES = [(1, 1, 2, 2), (2, 3, 3, 3), (1, 2, 2, 70)] + [(1, 2, 5, W) for W in (62, 63, 64, 65, 66)]
UPCAT_CASES = [(1, 1, 0, 1, 1), (2, 3, 2, 1, 33), (1, 2, 5, 33, 1), (2, 4, 4, 16, 32), (2, 3, None, 3, 5)]   # C2 0 / None: skip=None
MAXPOOL_SHAPES = [(2, 3, H, W) for H in (1, 2, 7, 8) for W in (1, 2, 7, 8)] + [(1, 2, 5, W) for W in (127, 128, 129, 130)]
BIAS_ELU_SHAPES = [(1, 1, 1, 4), (2, 5, 2, 4), (3, 70, 4, 513), (4, 4, 512, 1028)]          # (N, C, H, W): HW = 4, 8, 2052, 512 * 1028
DISPCONV_SHAPES = [(2, 5, 2, 3), (1, 7, 9, 2), (1, 5, 2, 4), (2, 16, 3, 8), (2, 3, 128, 260), (1, 256, 4, 8), (2, 1, 3, 4)]


# ------------------------------------------------------------------------------------------------ inputs
def bn_inputs(gen, shape, variant="plain", residual=False):
    """(x, weight, bias, residual or None, running_mean, running_var, upstream gradient) as fp32.  x per `variant`, every
    channel then multiplied by its scale 10^U(-2,2):
      plain          N(0.3, 1.7^2)
      offset         mean 50, std 0.5
      outlier_first  N(0, 1) with 1e4 as the first element of every channel
      constant       plain, and channel 1 holds one value (variance exactly 0, invstd = eps^-1/2); its beta is positive
                     so that relu(beta) is not an all-zero group
    The upstream gradient carries channel scales of its own."""
    N, C, H, W = shape
    if variant in ("plain", "constant"):
        x = 0.3 + 1.7 * draw(gen, *shape)
    elif variant == "offset":
        x = 50.0 + 0.5 * draw(gen, *shape)
    else:
        assert variant == "outlier_first"
        x = draw(gen, *shape)
        x[0, :, 0, 0] = 1e4
    if variant == "constant":
        x[:, 1] = x[0, 1, 0, 0]
    x = x * channel_scales(gen, C, 10.0).reshape(1, C, 1, 1)
    w = 1.0 + 0.3 * draw(gen, C)
    b = 0.3 * draw(gen, C)
    if variant == "constant":
        b[1] = b[1].abs() + 0.1
    res = draw(gen, *shape) if residual else None
    rm, rv = 0.5 * draw(gen, C), 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    gy = draw(gen, *shape) * channel_scales(gen, C, 10.0).reshape(1, C, 1, 1)
    return tuple(None if t is None else rounded(t) for t in (x, w, b, res, rm, rv, gy))


def bn_seed(shape, variant, residual, relu):
    return sum(s * p for s, p in zip(shape, (7, 101, 1009, 10007))) + 13 * len(variant) + 2 * residual + relu


def maxpool_inputs(gen, shape, special=None):
    """(x, upstream): values quantised to four levels, so most windows tie.  `special`: "-inf" / "nan" puts that value on a
    quarter of the positions (whole windows of it included)."""
    x = torch.randint(0, 4, shape, generator=gen).double() * 0.5 - 1.0
    if special is not None:
        hit = torch.rand(shape, generator=gen) < 0.25
        x[hit] = float("nan") if special == "nan" else float("-inf")
    OH, OW = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    up = draw(gen, shape[0], shape[1], OH, OW) * channel_scales(gen, shape[1], 10.0).reshape(1, -1, 1, 1)
    return rounded(x), rounded(up)


def bias_elu_inputs(gen, shape):
    """(v, bias, upstream): pre-activations with channel scales 10^U(-4,1), the bias scaled alike; exact 0, -0.0 and
    values below -90 among them (the bias of channel 0 is 0, so that they reach the ELU as they are)."""
    N, C, H, W = shape
    scales = channel_scales(gen, C, 10.0, -4.0, 1.0)
    v = draw(gen, *shape) * scales.reshape(1, C, 1, 1)
    bias = 0.5 * draw(gen, C) * scales
    bias[0] = 0.0
    flat = v[0, 0].reshape(-1)
    flat[0], flat[1], flat[2], flat[3] = 0.0, -0.0, -95.0, -1e3
    up = draw(gen, *shape) * channel_scales(gen, C, 10.0).reshape(1, C, 1, 1)
    return rounded(v), rounded(bias), rounded(up)


def dispconv_inputs(gen, shape):
    N, C, H, W = shape
    x = draw(gen, *shape) * channel_scales(gen, C, 10.0).reshape(1, C, 1, 1)
    w = draw(gen, 1, C, 3, 3) / (3.0 * C ** 0.5) / channel_scales(gen, C, 10.0, -1.0, 1.0).reshape(1, C, 1, 1)
    b = draw(gen, 1)
    up = draw(gen, N, 1, H, W)
    return rounded(x), rounded(w), rounded(b), rounded(up)


# shapes the modules must keep away from the kernels (layers.py); the GPU tier runs them with the kernel's entry point
# replaced by one that raises
FALLBACKS = {
    "reflect_pad1 planes": (1, 65536, 2, 2),
    "ConvBlock out_hw % 4": (2, 3, 5, 7),           # un-padded size of forward_padded's input
    "ConvBlock bias=None": (2, 3, 4, 6),            # a size the fused path takes, but for the missing bias
    "Conv3x3(257, 1)": (1, 257, 3, 4),
}


# ------------------------------------------------------------------------------------------------ measuring
BN_TENSORS = [("y", "channel"), ("running_mean", "tensor"), ("running_var", "tensor"), ("grad_x", "channel"),
              ("grad_w", "tensor"), ("grad_b", "tensor"), ("grad_res", "channel")]


def bn_run(fn, inp, device, dtype):
    """fn(x, w, b, res, running_mean, running_var) -> (y, running_mean, running_var, num_batches_tracked[, z]) with the
    inputs of `bn_inputs` on `device` in `dtype`; everything by name, gradients included (absent ones None)."""
    x, w, b, res, rm, rv, gy = inp
    out = forward_backward(fn, [x, w, b, res], [rm, rv], [gy], device, dtype)
    named = dict(zip(["y", "running_mean", "running_var", "num_batches_tracked", "z"], out[:-4]))
    named.update(zip(["grad_x", "grad_w", "grad_b", "grad_res"], out[-4:]))
    return named


def bn_formula(relu, rows=None, tracked=None, mask=None):
    return lambda x, w, b, res, rm, rv: batch_norm_act(x, w, b, res, rm, rv, MOMENTUM, EPS, relu, rows, tracked, mask)


def measured(t, kind):
    return nhwc(t) if kind == "channel" else t


def nhwc(t):
    """NCHW -> channel axis last, for group_error(..., "channel")."""
    return t.movedim(1, -1)


def channel_errors(got, ref):
    """Per channel of NCHW tensors: (max |got - ref|, max |ref|), float64 on the CPU."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    C = ref.shape[1]
    return (nhwc(got - ref).abs().reshape(-1, C).amax(0), nhwc(ref).abs().reshape(-1, C).amax(0))


def mask_report(y_kernel, z_eager, z64):
    """(elements outside the near-tie zone whose mask y_kernel > 0 differs from z64 > 0, share of elements inside the zone)."""
    z64 = z64.detach().double().cpu()
    num, den = channel_errors(z_eager, z64)
    tau = torch.tensor([bound(float(e)) for e in num / den], dtype=torch.float64) * den
    near = z64.abs() <= tau.reshape(1, -1, 1, 1)
    wrong = ((y_kernel.detach().cpu() > 0) != (z64 > 0)) & ~near
    return int(wrong.sum()), float(near.double().mean())
