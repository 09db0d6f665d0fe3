"""CPU tier for the float64 references of the encoder / decoder glue kernels (tests/nn_f64_ref.py).

1. Each reference against a second formulation in float64 that shares no code with it (F.batch_norm called group by
   group, F.pad, F.max_pool2d, F.interpolate + cat, F.elu, an explicit 9-tap sum): a wrong reference must not be able
   to agree with a wrong kernel.  Bound: SECOND_FORM of every group's maximum - two orderings of the same float64 formula.
2. The conditions the input builders promise, for every case of the GPU tier: no measured group is all zero, and the
   near-tie zone of the ReLU mask protocol holds at most NEAR_TIE_CAP of the elements (CPU eager fp32 stands in for
   the GPU's).
3. The dispatch paths the case lists reach, recomputed from the shapes (`pick_split`, the BN_SMALL_ELEMS test), and the
   library's own scratch sizes as a check of that recomputation."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import nn_f64_ref as R

SECOND_FORM = 1e-12
F64 = torch.float64


def _close(a, b, kind="tensor"):
    return R.group_error(a, b, kind) <= SECOND_FORM


# ------------------------------------------------------------------------------------------------ second formulations
@pytest.mark.parametrize("rows,tracked", [(None, None), ([3, 2, 4], None), ([3, 2, 4], 2)])
@pytest.mark.parametrize("res,relu", [(False, False), (True, True)])
def test_batch_norm_reference_against_batch_norm_called_group_by_group(rows, tracked, res, relu):
    gen = torch.Generator().manual_seed(5)
    inp = [None if t is None else t.double() for t in R.bn_inputs(gen, (9, 4, 3, 5), "plain", res)]
    got = R.bn_run(R.bn_formula(relu, rows, tracked), inp, "cpu", F64)

    def second(x, w, b, r, rm, rv):
        rm, rv, batches = rm.clone(), rv.clone(), torch.tensor(R.BATCHES_BEFORE)
        ys, lo = [], 0
        for g, n in enumerate(rows or [9]):
            track = tracked is None or g < tracked
            ys.append(F.batch_norm(x[lo:lo + n], rm if track else None, rv if track else None, w, b, True, R.MOMENTUM, R.EPS))
            batches = batches + int(track)
            lo += n
        y = torch.cat(ys)
        y = y if r is None else y + r
        return (F.relu(y) if relu else y), rm, rv, batches
    want = R.bn_run(second, inp, "cpu", F64)
    for name, kind in R.BN_TENSORS:
        if want[name] is None:
            assert got[name] is None and name == "grad_res"
            continue
        assert _close(R.measured(got[name], kind), R.measured(want[name], kind), kind), name
    assert int(got["num_batches_tracked"]) == int(want["num_batches_tracked"])


def test_batch_norm_reference_with_a_given_mask_differentiates_z_times_mask():
    gen = torch.Generator().manual_seed(6)
    x, w, b, res, rm, rv, gy = [t.double() for t in R.bn_inputs(gen, (3, 4, 2, 5), "plain", True)]
    mask = torch.rand(3, 4, 2, 5, generator=gen) < 0.5                  # any mask, not the reference's own
    got = R.bn_run(R.bn_formula(True, mask=mask), (x, w, b, res, rm, rv, gy), "cpu", F64)
    assert torch.equal(got["y"], torch.relu(got["z"]))
    assert torch.equal(got["grad_res"], gy * mask)
    lin = R.bn_run(R.bn_formula(False), (x, w, b, res, rm, rv, gy * mask), "cpu", F64)
    for name in ("grad_x", "grad_w", "grad_b"):
        assert _close(got[name], lin[name]), name
    empty = R.batch_norm_act(x, w, b, None, rm, rv, 0.1, 1e-5, False, rows=[2, 0, 1], tracked=1)
    one = R.batch_norm_act(x[:2], w, b, None, rm, rv, 0.1, 1e-5, False)
    assert torch.equal(empty[0][:2], one[0]) and torch.equal(empty[1], one[1]) and torch.equal(empty[2], one[2])


@pytest.mark.parametrize("shape", R.REFLECT_SHAPES)
def test_reflection_pad_reference_against_f_pad(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    x = R.draw(gen, *shape)
    up = R.draw(gen, shape[0], shape[1], shape[2] + 2, shape[3] + 2)
    got = R.forward_backward(R.reflect_pad1, [x], [], [up], "cpu", F64)
    want = R.forward_backward(lambda t: F.pad(t, (1, 1, 1, 1), mode="reflect"), [x], [], [up], "cpu", F64)
    assert torch.equal(got[0], want[0]) and _close(got[1], want[1])


@pytest.mark.parametrize("special", [None, "-inf", "nan"])
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES[:16:3] + R.MAXPOOL_SHAPES[16::2])
def test_max_pool_reference_against_f_max_pool2d_on_ties_and_nan(shape, special):
    gen = torch.Generator().manual_seed(sum(shape))
    x, up = [t.double() for t in R.maxpool_inputs(gen, shape, special)]
    got = R.forward_backward(R.maxpool3s2, [x], [], [up], "cpu", F64)
    want = R.forward_backward(lambda t: F.max_pool2d(t, 3, 2, 1), [x], [], [up], "cpu", F64)
    assert torch.equal(torch.isnan(got[0]), torch.isnan(want[0]))
    assert torch.equal(torch.nan_to_num(got[0], nan=7.0), torch.nan_to_num(want[0], nan=7.0))
    assert torch.equal(got[1], want[1])                                 # each output's gradient lands on one position


def test_max_pool_reference_takes_the_first_maximum_and_keeps_a_nan():
    x = torch.tensor([[[[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]]], dtype=F64, requires_grad=True)
    y = R.maxpool3s2(x)                                                 # windows centred on (0,0), (0,2), (2,0), (2,2)
    y.backward(torch.tensor([[[[1.0, 10.0], [100.0, 1000.0]]]], dtype=F64))
    assert y.flatten().tolist() == [1.0, 1.0, 1.0, 1.0]
    assert x.grad[0, 0].tolist() == [[1.0, 10.0, 0.0], [100.0, 1000.0, 0.0], [0.0, 0.0, 0.0]]
    z = torch.tensor([[[[0.0, float("nan")], [5.0, 9.0]]]], dtype=F64)
    assert bool(torch.isnan(R.maxpool3s2(z)).all())


@pytest.mark.parametrize("N,C1,C2,h,w", R.UPCAT_CASES)
def test_upsample_concat_pad_reference_against_the_three_torch_ops(N, C1, C2, h, w):
    gen = torch.Generator().manual_seed(N + C1 + h + w)
    x = R.draw(gen, N, C1, h, w)
    skip = R.draw(gen, N, C2, 2 * h, 2 * w) if C2 else None
    up = R.draw(gen, N, C1 + (C2 or 0), 2 * h + 2, 2 * w + 2)

    def second(t, s):
        u = F.interpolate(t, scale_factor=2, mode="nearest")
        return F.pad(u if s is None else torch.cat([u, s], 1), (1, 1, 1, 1), mode="reflect")
    got = R.forward_backward(R.upcat_pad, [x, skip], [], [up], "cpu", F64)
    want = R.forward_backward(second, [x, skip], [], [up], "cpu", F64)
    assert torch.equal(got[0], want[0]) and _close(got[1], want[1])
    assert (got[2] is None and want[2] is None) if not C2 else _close(got[2], want[2])


@pytest.mark.parametrize("shape", R.BIAS_ELU_SHAPES[:3])
def test_bias_elu_reference_against_f_elu(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    v, bias, up = [t.double() for t in R.bias_elu_inputs(gen, shape)]
    got = R.forward_backward(R.bias_elu, [v, bias], [], [up], "cpu", F64)
    want = R.forward_backward(lambda t, b: F.elu(t + b.reshape(1, -1, 1, 1)), [v, bias], [], [up], "cpu", F64)
    for a, b, kind in zip(got, want, ("channel", "channel", "tensor")):
        assert _close(R.measured(a, kind), R.measured(b, kind), kind)
    flat = got[0][0, 0].reshape(-1)
    assert flat[0] == 0.0 and flat[1] == 0.0 and flat[2] == -1.0 + torch.exp(torch.tensor(-95.0, dtype=F64)) and flat[3] == -1.0


def test_bias_elu_inputs_tell_expm1_from_exp_minus_one():
    """The small-scale channels are what a kernel computing expf(v) - 1 fails on: in fp32 that form misses the bound that the
    expm1 form sets more than ten times over."""
    gen = torch.Generator().manual_seed(sum(R.BIAS_ELU_SHAPES[2]))
    v, bias, _ = R.bias_elu_inputs(gen, R.BIAS_ELU_SHAPES[2])
    ref = R.bias_elu(v.double(), bias.double())
    z = v + bias.reshape(1, -1, 1, 1)
    naive = torch.where(z > 0, z, torch.exp(torch.clamp(z, max=0.0)) - 1.0)
    eager = R.group_error(R.nhwc(R.bias_elu(v, bias)), R.nhwc(ref), "channel")
    assert R.group_error(R.nhwc(naive), R.nhwc(ref), "channel") > 10 * R.bound(eager)


@pytest.mark.parametrize("shape", [s for s in R.DISPCONV_SHAPES if s[1] <= 16 and s[2] < 100])
def test_disparity_head_reference_against_a_nine_tap_sum(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    x, w, b, up = [t.double() for t in R.dispconv_inputs(gen, shape)]
    N, C, H, W = shape

    def second(t, k, c):
        p = F.pad(t, (1, 1, 1, 1), mode="reflect")
        acc = c.reshape(1, 1, 1, 1)
        for dy in range(3):
            for dx in range(3):
                acc = acc + (p[:, :, dy:dy + H, dx:dx + W] * k[0, :, dy, dx].reshape(1, C, 1, 1)).sum(1, keepdim=True)
        return acc
    got = R.forward_backward(R.dispconv, [x, w, b], [], [up], "cpu", F64)
    want = R.forward_backward(second, [x, w, b], [], [up], "cpu", F64)
    for a, c, kind in zip(got, want, ("channel", "channel", "tensor", "tensor")):
        assert _close(R.measured(a, kind), R.measured(c, kind), kind)


# ------------------------------------------------------------------------------------------------ input conditions
def _bn_conditions(inp, relu, rows=None, tracked=None):
    """No all-zero group among the measured tensors (group_error asserts it), the near-tie share under its cap."""
    ref = R.bn_run(R.bn_formula(relu, rows, tracked), inp, "cpu", F64)
    lo = 0
    for n in rows or [inp[0].shape[0]]:                                  # each call group is measured on its own
        for name, kind in R.BN_TENSORS:
            if ref[name] is not None and n > 0:
                t = R.measured(ref[name][lo:lo + n] if kind == "channel" else ref[name], kind)
                assert R.group_error(t, t, kind) == 0.0, name
        lo += n
    if relu:
        eager = R.bn_run(R.bn_formula(relu, rows, tracked), inp, "cpu", torch.float32)
        wrong, share = R.mask_report(ref["y"], eager["z"], ref["z"])
        assert wrong == 0 and share <= R.NEAR_TIE_CAP, share
        return share
    return 0.0


@pytest.mark.parametrize("shape,variant,res,relu", R.bn_cases())
def test_batch_norm_inputs_keep_their_conditions(shape, variant, res, relu):
    gen = torch.Generator().manual_seed(R.bn_seed(shape, variant, res, relu))
    inp = R.bn_inputs(gen, shape, variant, res)
    x = inp[0].double()
    if variant == "constant":
        assert bool((x[:, 1] == x[0, 1, 0, 0]).all()) and float(inp[2][1]) > 0
    if variant == "offset":
        ratio = x.mean(dim=(0, 2, 3)).abs() / x.std(dim=(0, 2, 3))
        assert float(ratio.min()) > 90
    if variant == "outlier_first":
        assert bool((x[0, :, 0, 0] == x.amax(dim=(0, 2, 3))).all())
    _bn_conditions(inp, relu)


def test_grouped_batch_norm_inputs_keep_their_conditions():
    for shape, rows, padding, res, relu in R.BN_GROUPED_CASES:
        gen = torch.Generator().manual_seed(R.bn_seed(shape, "grouped", res, relu))
        _bn_conditions(R.bn_inputs(gen, shape, "plain", res), relu, rows, len(rows) - padding)
    shape, rows, tracked, biggest = R.BN_DEVICE_CASE
    gen = torch.Generator().manual_seed(R.bn_seed(shape, "device", True, True))
    _bn_conditions(R.bn_inputs(gen, shape, "plain", True), True, rows, tracked)


def test_other_inputs_have_no_all_zero_group():
    def check(fn, leaves, upstream, kinds):
        out = R.forward_backward(fn, leaves, [], upstream, "cpu", F64)
        for t, kind in zip(out, kinds):
            if t is not None and t.numel():
                finite = torch.nan_to_num(t, nan=1.0, posinf=1.0, neginf=1.0)
                assert R.group_error(R.measured(finite, kind), R.measured(finite, kind), kind) == 0.0
    for shape in R.REFLECT_SHAPES:
        gen = torch.Generator().manual_seed(sum(shape))
        check(R.reflect_pad1, [R.draw(gen, *shape)], [R.draw(gen, shape[0], shape[1], shape[2] + 2, shape[3] + 2)], ["channel"] * 2)
    for shape in R.BIAS_ELU_SHAPES[:3]:
        v, bias, up = R.bias_elu_inputs(torch.Generator().manual_seed(sum(shape)), shape)
        check(R.bias_elu, [v, bias], [up], ["channel", "channel", "tensor"])
    for shape in R.DISPCONV_SHAPES:
        check(R.dispconv, list(R.dispconv_inputs(torch.Generator().manual_seed(sum(shape)), shape)[:3]),
              [R.dispconv_inputs(torch.Generator().manual_seed(sum(shape)), shape)[3]], ["channel", "channel", "tensor", "tensor"])


# ------------------------------------------------------------------------------------------------ dispatch paths
@pytest.fixture(scope="module")
def dll():
    from baseboostdepth_amd.csrc.build import build
    return ctypes.CDLL(build())


def test_split_recomputation_matches_the_library(dll):
    for N, C, H, W in R.BN_SHAPES + [R.BN_CAPPED] + [s for s, *_ in R.BN_GROUPED_CASES] + R.BIAS_ELU_SHAPES:
        assert dll.bbd_bn_scratch_doubles(N, C, H * W) == C * R.pick_split(N, H * W) * 2
        assert dll.bbd_bias_elu_scratch_doubles(N, C, H * W) == C * R.pick_split(N, H * W)
    for shape, rows, *_ in R.BN_GROUPED_CASES:
        N, C, H, W = shape
        assert dll.bbd_bn_grouped_scratch_doubles(max(rows), len(rows), C, H * W) == len(rows) * C * R.pick_split(max(rows), H * W) * 2


def test_batch_norm_cases_reach_every_dispatch_path():
    path = {s: R.bn_path(s) for s in R.BN_SHAPES + [R.BN_CAPPED]}
    assert path[(2, 5, 1, 3)] == (True, False, 1, "one") and path[(3, 7, 5, 9)] == (True, False, 1, "one")
    assert 2 % 4 and 3 % 4                                               # N no multiple of the 4 waves
    assert path[(4, 6, 8, 16)] == (True, True, 1, "one")
    assert path[(2, 4, 48, 64)] == (True, True, 2, "several")            # one launch looping over 2 slices
    assert path[(2100, 3, 1, 2)] == (True, False, 1, "plane")            # max_by_plane clamps 2 -> 1
    assert path[(3, 5, 40, 72)] == (False, True, 3, "several")
    assert path[(3, 5, 37, 79)] == (False, False, 3, "several")
    HW = 37 * 79
    length = (-(-HW // 3) + 3) & ~3
    assert 2 * length < HW < 3 * length and (HW - 2 * length) != length  # the last slice is ragged
    assert path[R.BN_CAPPED] == (False, True, R.MAX_SPLIT, "capped")
    cases = R.bn_cases()
    reached = {(R.bn_path(s)[0], R.bn_path(s)[1], res, relu) for s, v, res, relu in cases}
    assert reached >= {(one, vec, res, relu) for one in (True, False) for vec in (True, False) for res in (True, False)
                       for relu in (True, False)}                         # both launch forms x both layouts x all four tails
    assert {R.bn_path(s)[3] for s, *_ in cases} == {"one", "several", "capped", "plane"}
    for variant, shapes in (("offset", R.BN_VARIANT_SHAPES), ("outlier_first", R.BN_VARIANT_SHAPES), ("constant", R.BN_CONSTANT_SHAPES)):
        assert {s for s, v, *_ in cases if v == variant} == set(shapes)
        assert {R.bn_path(s)[:2] for s in shapes} == {(True, False), (True, True), (False, True), (False, False)} or variant == "constant"
    assert {R.bn_path(s)[:2] for s in R.BN_CONSTANT_SHAPES} == {(True, True), (False, False)}
    assert len(cases) == len(set(cases)) == 7 * 4 + 1 + 2 * 5 + 2 * 2


def test_grouped_cases_reach_the_host_and_the_device_table():
    (s0, r0, p0, *_), (s1, r1, p1, *_), (s2, r2, p2, *_) = R.BN_GROUPED_CASES
    assert R.bn_path(s0, r0)[0] and len(r0) > 1                          # one launch + the C-thread follow-up
    one, vec, split, how = R.bn_path(s1, r1)
    assert not one and split == 3 and s1[2] * s1[3] == 1500
    assert R.pick_split(r1[0], 1500) == 1 < split                        # group 0 leaves blocks of the grid idle
    assert r1[1] * 1500 > R.BN_SMALL_ELEMS >= r1[0] * 1500               # the launch form follows the biggest group
    assert p2 == 1 and sum(r2) == s2[0] and p0 == p1 == 0
    shape, rows, tracked, biggest = R.BN_DEVICE_CASE
    assert 0 in rows[1:-1] and tracked < len(rows) and all(n > 0 for n in rows[:tracked]) and biggest == max(rows)
    assert sum(rows) == shape[0]


def test_other_case_lists_reach_their_paths():
    assert (2, 3, 3, 3) in R.REFLECT_SHAPES and {s[3] for s in R.REFLECT_SHAPES} >= {2, 62, 63, 64, 65, 66, 70}
    assert {(s[2], s[3]) for s in R.MAXPOOL_SHAPES[:16]} == {(h, w) for h in (1, 2, 7, 8) for w in (1, 2, 7, 8)}
    assert {(s[3] - 1) // 2 + 1 for s in R.MAXPOOL_SHAPES[16:]} == {64, 65}   # OW on both sides of the 64 lanes
    N, C, H, W = R.BIAS_ELU_SHAPES[2]
    assert R.pick_split(N, H * W) == 2 and C > 64 and H * W == 2052
    N, C, H, W = R.BIAS_ELU_SHAPES[3]
    assert N * C * H * W // 4 > 8192 * 256 and H * W == 512 * 1028        # the forward's grid is capped and strides
    assert all(s[2] * s[3] % 4 == 0 for s in R.BIAS_ELU_SHAPES)
    assert {s[1] for s in R.DISPCONV_SHAPES} >= {1, 5, 16, 256}
    assert {s[3] % 4 == 0 for s in R.DISPCONV_SHAPES} == {True, False}
    N, C, H, W = (2, 3, 128, 260)
    assert (N, C, H, W) in R.DISPCONV_SHAPES and N * H * W // 4 > 64 * 256    # the weight kernel's second grid-stride turn
    assert (1, 5, 2, 4) in R.DISPCONV_SHAPES                                   # one strip per row: both neighbours reflect
    assert any(C2 == 0 for _, _, C2, _, _ in R.UPCAT_CASES) and any(C2 is None for _, _, C2, _, _ in R.UPCAT_CASES)
    # the four eager paths of the modules; that each shape does take its eager path is the GPU tier's to show
    assert set(R.FALLBACKS) == {"reflect_pad1 planes", "ConvBlock out_hw % 4", "ConvBlock bias=None", "Conv3x3(257, 1)"}
