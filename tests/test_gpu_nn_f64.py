"""GPU tier: the encoder / decoder glue kernels (csrc/bbd_nn.hip) against float64 references, on every dispatch path of
their launch code.

Each case runs forward and backward through the public `ops.*` entry point and is measured as tests/nn_f64_ref.py
describes: activations and their gradients per channel, parameter gradients and running statistics per tensor, against
the float64 result, bounded by 8 x the error of the eager fp32 formulation on the GPU on the same inputs (floor
8 * 2^-24).  ReLU follows the mask protocol of nn_f64_ref.  Every case also runs a second time (bit-equal) and a third
time after allocator blocks of its scratch and output sizes were filled with NaN and freed (bit-equal again).

Measured on an MI355X (forwards that are copies - reflect_pad1, upcat_pad, maxpool3s2 - and grad_res = dy * mask are exact
on both sides and show as 0).  Per operation and tensor over its cases: eager error, kernel error, the worst kernel / eager
and its case (the ratio's denominator is at least 2^-24):

operation          tensor               cases  eager error         kernel error        worst kernel/eager (case)
bn plain           y                       29  8.2e-08 .. 2.0e-07  7.6e-08 .. 1.4e-07  1.31  bn (4, 6, 8, 16) plain res=1 relu=1
bn plain           running_mean            29  1.2e-08 .. 4.0e-07  1.2e-08 .. 1.1e-07  1.19  bn (3, 5, 37, 79) plain res=1 relu=1
bn plain           running_var             29  4.1e-09 .. 1.6e-07  4.7e-10 .. 1.5e-07  1.85  bn (2100, 3, 1, 2) plain res=1 relu=1
bn plain           grad_x                  29  9.8e-08 .. 2.5e-07  8.9e-08 .. 2.1e-07  1.37  bn (3, 5, 40, 72) plain res=1 relu=1
bn plain           grad_w                  29  2.6e-08 .. 7.8e-07  1.0e-08 .. 8.3e-07  7.27  bn (3, 5, 37, 79) plain res=0 relu=0
bn plain           grad_b                  29  1.3e-08 .. 2.1e-06  7.7e-10 .. 2.4e-06  3.67  bn (2, 4, 48, 64) plain res=1 relu=0
bn plain           grad_res                14  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (2, 5, 1, 3) plain res=1 relu=0
bn offset          y                        5  1.4e-06 .. 6.9e-06  7.4e-07 .. 1.8e-06  0.68  bn (4, 6, 8, 16) offset res=1 relu=1
bn offset          running_mean             5  7.8e-09 .. 1.1e-07  1.3e-08 .. 1.0e-07  1.71  bn (4, 6, 8, 16) offset res=1 relu=1
bn offset          running_var              5  1.3e-08 .. 1.4e-07  2.1e-08 .. 1.3e-07  1.15  bn (4, 6, 8, 16) offset res=1 relu=1
bn offset          grad_x                   5  1.2e-07 .. 3.8e-07  9.3e-08 .. 2.8e-07  1.41  bn (3, 5, 37, 79) offset res=1 relu=1
bn offset          grad_w                   5  2.8e-07 .. 1.3e-05  2.8e-07 .. 5.1e-06  1.00  bn (3, 5, 40, 72) offset res=0 relu=1
bn offset          grad_b                   5  5.4e-08 .. 4.2e-05  3.1e-08 .. 1.1e-05  1.65  bn (3, 5, 40, 72) offset res=0 relu=1
bn offset          grad_res                 2  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (4, 6, 8, 16) offset res=1 relu=1
bn outlier_first   y                        5  3.7e-08 .. 1.5e-07  9.4e-08 .. 1.3e-07  2.23  bn (4, 2, 256, 260) outlier_first res=0 relu=1
bn outlier_first   running_mean             5  1.3e-08 .. 1.6e-07  7.2e-09 .. 8.2e-08  0.78  bn (3, 5, 37, 79) outlier_first res=1 relu=1
bn outlier_first   running_var              5  3.1e-08 .. 1.7e-07  3.1e-08 .. 1.7e-07  1.00  bn (4, 2, 256, 260) outlier_first res=0 relu=1
bn outlier_first   grad_x                   5  1.5e-07 .. 8.8e-04  1.4e-07 .. 5.1e-04  1.58  bn (3, 5, 40, 72) outlier_first res=0 relu=1
bn outlier_first   grad_w                   5  4.6e-09 .. 1.9e-07  1.9e-08 .. 1.1e-07  1.80  bn (4, 6, 8, 16) outlier_first res=1 relu=1
bn outlier_first   grad_b                   5  2.3e-08 .. 5.3e-07  4.6e-09 .. 1.6e-07  0.44  bn (3, 5, 40, 72) outlier_first res=0 relu=1
bn outlier_first   grad_res                 2  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (4, 6, 8, 16) outlier_first res=1 relu=1
bn constant        y                        4  9.1e-08 .. 1.3e-07  9.1e-08 .. 1.6e-07  1.35  bn (4, 6, 8, 16) constant res=0 relu=1
bn constant        running_mean             4  9.6e-09 .. 7.3e-08  9.6e-09 .. 7.3e-08  1.00  bn (4, 6, 8, 16) constant res=0 relu=1
bn constant        running_var              4  3.6e-08 .. 1.4e-07  1.5e-08 .. 5.3e-08  0.88  bn (3, 5, 37, 79) constant res=1 relu=1
bn constant        grad_x                   4  1.2e-07 .. 1.6e-07  1.0e-07 .. 1.6e-07  1.37  bn (3, 5, 37, 79) constant res=0 relu=1
bn constant        grad_w                   4  2.3e-08 .. 1.2e-07  6.6e-09 .. 8.9e-08  0.98  bn (3, 5, 37, 79) constant res=0 relu=1
bn constant        grad_b                   4  2.6e-08 .. 4.0e-08  2.6e-08 .. 1.4e-07  2.40  bn (3, 5, 37, 79) constant res=1 relu=1
bn constant        grad_res                 2  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (4, 6, 8, 16) constant res=1 relu=1
bn call groups     y                        9  9.8e-08 .. 2.1e-07  8.2e-08 .. 1.4e-07  1.12  bn grouped (12, 6, 4, 10) rows=[5, 3, 4] padding=0
bn call groups     running_mean             3  3.8e-08 .. 1.6e-07  2.8e-08 .. 1.6e-07  1.00  bn grouped (16, 6, 4, 10) rows=[5, 3, 4, 4] padding=1
bn call groups     running_var              3  3.6e-08 .. 9.0e-08  2.7e-08 .. 4.7e-08  0.79  bn grouped (7, 4, 30, 50) rows=[1, 6] padding=0
bn call groups     grad_x                   9  9.5e-08 .. 1.7e-07  8.4e-08 .. 1.4e-07  1.44  bn grouped (7, 4, 30, 50) rows=[1, 6] padding=0
bn call groups     grad_w                   3  9.1e-08 .. 2.1e-07  8.7e-08 .. 2.2e-07  2.01  bn grouped (16, 6, 4, 10) rows=[5, 3, 4, 4] padding=1
bn call groups     grad_b                   3  4.2e-08 .. 9.7e-08  4.2e-08 .. 9.3e-08  0.97  bn grouped (7, 4, 30, 50) rows=[1, 6] padding=0
bn call groups     grad_res                 3  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn grouped (12, 6, 4, 10) rows=[5, 3, 4] padding=0
bn device table    y                        3  8.6e-08 .. 1.1e-07  8.2e-08 .. 1.1e-07  1.00  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
bn device table    running_mean             1  1.5e-08 .. 1.5e-08  1.5e-08 .. 1.5e-08  0.25  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
bn device table    running_var              1  2.7e-08 .. 2.7e-08  2.7e-08 .. 2.7e-08  0.45  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
bn device table    grad_x                   3  8.8e-08 .. 1.1e-07  7.9e-08 .. 1.5e-07  1.45  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
bn device table    grad_w                   1  1.3e-07 .. 1.3e-07  1.3e-07 .. 1.3e-07  1.02  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
bn device table    grad_b                   1  2.4e-07 .. 2.4e-07  3.5e-08 .. 3.5e-08  0.15  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
bn device table    grad_res                 3  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn device table (9, 5, 6, 10) rows=[3, 4, 0, 2] tracked=2
reflect_pad1       y                        8  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  reflect_pad1 (1, 1, 2, 2)
reflect_pad1       grad x                   8  2.7e-08 .. 5.2e-08  2.7e-08 .. 6.5e-08  1.09  reflect_pad1 (1, 2, 5, 65)
upcat_pad          y                        5  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  upcat_pad (1, 1, 0, 1, 1)
upcat_pad          grad x                   5  6.6e-08 .. 8.8e-08  6.6e-08 .. 8.4e-08  1.00  upcat_pad (1, 1, 0, 1, 1)
upcat_pad          grad skip                3  4.2e-08 .. 5.8e-08  4.1e-08 .. 5.8e-08  0.98  upcat_pad (2, 4, 4, 16, 32)
maxpool3s2         grad x                  22  0.0e+00 .. 6.9e-08  0.0e+00 .. 6.9e-08  1.08  maxpool3s2 (2, 3, 7, 130) nan
bias_elu           y                        4  0.0e+00 .. 8.8e-08  0.0e+00 .. 8.8e-08  1.00  bias_elu (3, 70, 2052)
bias_elu           grad x                   4  0.0e+00 .. 7.5e-08  0.0e+00 .. 7.5e-08  1.00  bias_elu (3, 70, 2052)
bias_elu           grad bias                4  0.0e+00 .. 6.7e-07  0.0e+00 .. 8.2e-08  0.54  bias_elu (3, 70, 2052)
dispconv           y                       13  3.2e-08 .. 4.3e-07  6.0e-08 .. 5.8e-07  1.75  dispconv (1, 5, 2, 4)
dispconv           grad x                  11  6.2e-08 .. 2.0e-07  6.3e-08 .. 1.6e-07  1.02  dispconv (2, 5, 2, 3) bias=None
dispconv           grad weight             11  3.5e-08 .. 1.3e-06  3.4e-08 .. 1.1e-07  1.55  dispconv (1, 5, 2, 4)
dispconv           grad bias                7  1.9e-08 .. 5.4e-05  1.2e-09 .. 7.9e-06  1.07  dispconv (2, 1, 3, 4)
fallback modules   outputs                  4  0.0e+00 .. 3.5e-07  0.0e+00 .. 3.5e-07  1.00  fallback ConvBlock out_hw % 4 (2, 3, 5, 7)
fallback modules   grad inputs              4  4.0e-08 .. 4.6e-07  4.0e-08 .. 4.6e-07  1.00  fallback reflect_pad1 (1, 65536, 2, 2)
fallback modules   parameter gradients      5  3.2e-08 .. 8.2e-08  3.2e-08 .. 8.2e-08  1.00  fallback ConvBlock out_hw % 4 (2, 3, 5, 7)
decoder            outputs                  4  1.4e-07 .. 2.2e-07  1.4e-07 .. 1.8e-07  1.08  decoder 64x128
decoder            grad inputs              5  3.2e-07 .. 1.6e-06  3.4e-07 .. 2.0e-06  1.34  decoder 64x128
decoder            parameter gradients     28  9.0e-08 .. 1.4e-06  2.8e-08 .. 1.1e-06  1.59  decoder 64x128

ReLU mask, 33 cases: no element outside its near-tie zone is masked differently from float64; the largest share of a
case's elements inside the zone is 0.00262 (cap 0.01).

Before the forward statistics kept centred runs (stats_slice added x and x * x in fp32 and group_moments formed
E[x^2] - mean^2), the same cases measured, per variant: worst kernel / eager and its case

operation          tensor               cases  eager error         kernel error        worst kernel/eager (case)
bn offset          y                        5  1.4e-06 .. 6.9e-06  3.7e-06 .. 2.8e-05  18.90  bn (3, 5, 37, 79) offset res=1 relu=1
bn offset          running_mean             5  7.8e-09 .. 1.1e-07  1.3e-08 .. 1.0e-07  1.71  bn (4, 6, 8, 16) offset res=1 relu=1
bn offset          running_var              5  1.3e-08 .. 1.4e-07  1.5e-07 .. 8.0e-05  577.51  bn (3, 5, 37, 79) offset res=1 relu=1
bn offset          grad_x                   5  1.2e-07 .. 3.8e-07  4.4e-06 .. 4.0e-05  287.45  bn (3, 5, 37, 79) offset res=1 relu=1
bn offset          grad_w                   5  2.8e-07 .. 1.3e-05  1.9e-06 .. 2.3e-05  15.47  bn (4, 6, 8, 16) offset res=1 relu=1
bn offset          grad_b                   5  5.4e-08 .. 4.2e-05  3.1e-08 .. 1.1e-05  1.65  bn (3, 5, 40, 72) offset res=0 relu=1
bn offset          grad_res                 2  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (4, 6, 8, 16) offset res=1 relu=1
bn outlier_first   y                        5  3.7e-08 .. 1.5e-07  4.9e-08 .. 1.8e-07  2.62  bn (3, 5, 37, 79) outlier_first res=1 relu=1
bn outlier_first   running_mean             5  1.3e-08 .. 1.6e-07  7.2e-09 .. 1.1e-07  1.00  bn (3, 5, 37, 79) outlier_first res=1 relu=1
bn outlier_first   running_var              5  3.1e-08 .. 1.7e-07  4.4e-08 .. 1.7e-07  1.17  bn (3, 5, 40, 72) outlier_first res=0 relu=1
bn outlier_first   grad_x                   5  1.5e-07 .. 8.8e-04  1.3e-07 .. 8.0e-04  2.29  bn (3, 5, 40, 72) outlier_first res=0 relu=1
bn outlier_first   grad_w                   5  4.6e-09 .. 1.9e-07  4.6e-09 .. 2.0e-07  1.88  bn (3, 5, 40, 72) outlier_first res=0 relu=1
bn outlier_first   grad_b                   5  2.3e-08 .. 5.3e-07  4.6e-09 .. 1.6e-07  0.44  bn (3, 5, 40, 72) outlier_first res=0 relu=1
bn outlier_first   grad_res                 2  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (4, 6, 8, 16) outlier_first res=1 relu=1
bn constant        y                        4  9.1e-08 .. 1.3e-07  9.1e-08 .. 1.6e-07  1.35  bn (4, 6, 8, 16) constant res=0 relu=1
bn constant        running_mean             4  9.6e-09 .. 7.3e-08  9.6e-09 .. 7.3e-08  1.00  bn (4, 6, 8, 16) constant res=0 relu=1
bn constant        running_var              4  3.6e-08 .. 1.4e-07  3.6e-08 .. 1.7e-07  1.23  bn (3, 5, 37, 79) constant res=0 relu=1
bn constant        grad_x                   4  1.2e-07 .. 1.6e-07  1.2e-07 .. 7.9e-01  6771692.51  bn (3, 5, 37, 79) constant res=0 relu=1
bn constant        grad_w                   4  2.3e-08 .. 1.2e-07  2.0e-08 .. 1.1e-07  1.00  bn (3, 5, 37, 79) constant res=1 relu=1
bn constant        grad_b                   4  2.6e-08 .. 4.0e-08  2.6e-08 .. 1.4e-07  2.40  bn (3, 5, 37, 79) constant res=1 relu=1
bn constant        grad_res                 2  0.0e+00 .. 0.0e+00  0.0e+00 .. 0.0e+00  0.00  bn (4, 6, 8, 16) constant res=1 relu=1

`offset` (mean / std = 100) failed at all five shapes: the squares were rounded in fp32 before the subtraction, so the
variance lost (mean / std)^2 of its digits.  `constant` failed without a residual at both shapes: the variance of a
constant channel came out as rounding noise instead of 0, and at (3, 5, 37, 79) invstd - eps^-1/2 for an exact 0 - was wrong
enough to put grad_x 79 % off.  `outlier_first` passed before and passes now: it is the case a fix that shifts by the
first element and then adds fp32 squares would fail.  `plain` measured the same before and after - its largest ratio
too: grad_w of (3, 5, 37, 79) without residual or ReLU, 7.27 x eager (5.6e-07 against 7.8e-08, bound 6.2e-07), is the
backward's fp32 runs of g * xhat over a sum that cancels, in code this change did not touch.

Which case reaches which path (recomputed from the shapes in test_nn_f64_ref.py):
one launch, scalar layout, split 1: (2,5,1,3), (3,7,5,9); one launch, vector: (4,6,8,16); one launch looping over 2 slices:
(2,4,48,64); split clamped to 1 by the plane: (2100,3,1,2); two launches, vector, 3 slices: (3,5,40,72); two launches, scalar,
ragged last slice: (3,5,37,79); split capped at MAX_SPLIT: (4,2,256,260).  Call groups: rows [5,3,4] one launch + the C-thread
follow-up; rows [1,6] at HW = 1500 two launches sized by group 1 while group 0 has one slice; a trailing padding group;
the device table with an empty group and 2 of 4 groups tracked.  bias_elu (3,70,2052): split 2 and two blocks of the final
reduction; (4,4,512*1028): the forward's grid stride.  dispconv (2,3,128,260): the weight kernel's second grid-stride turn.
Eager paths of the modules: 65 536 planes for ReflectionPad1, out_hw % 4 != 0 and bias=None for ConvBlock.forward_padded,
Conv3x3(257, 1).
"""
import contextlib

import pytest
import torch

import nn_f64_ref as R
from gpu_f64_common import DEV, check as _check, poison as _poison

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _lib():
    from baseboostdepth_amd import ops
    return ops.default_backend().lib


def _judge(case, name, kind, got, eager, ref, failures):
    e_err, k_err = R.group_error(R.measured(eager, kind), R.measured(ref, kind), kind), R.group_error(R.measured(got, kind), R.measured(ref, kind), kind)
    print("F64 | %s | %s | %.2e | %.2e | %.2f" % (case, name, e_err, k_err, k_err / max(e_err, 2.0 ** -24)))
    if not k_err <= R.bound(e_err):
        failures.append((name, "eager %.3e kernel %.3e bound %.3e" % (e_err, k_err, R.bound(e_err))))


def _same(name, runs, failures):
    first = runs[0]
    for other, what in zip(runs[1:], ("differs between two calls", "differs after NaN-filled blocks")):
        if not ((first is None and other is None) or torch.equal(first, other)):
            failures.append((name, what))


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_case(case, inp, relu, rows=None, tracked=None, context=contextlib.nullcontext, biggest=None):
    """One BatchNorm case through ops.batch_norm_act (inside `context()`: the call groups): every tensor of R.BN_TENSORS,
    each call group's activations on their own, num_batches_tracked, the ReLU mask, three bit-equal runs."""
    from baseboostdepth_amd import ops
    N, C, H, W = inp[0].shape
    groups = rows or [N]

    def kernel(x, w, b, res, rm, rv):
        rm, rv = rm.clone(), rv.clone()
        batches = torch.full((), R.BATCHES_BEFORE, dtype=torch.int64, device=x.device)
        with context():
            y = ops.batch_norm_act(x, w, b, res, rm, rv, R.MOMENTUM, R.EPS, relu, num_batches_tracked=batches)
        return y, rm, rv, batches
    got = R.bn_run(kernel, inp, DEV, F32)
    again = R.bn_run(kernel, inp, DEV, F32)
    _poison([2 * _lib().bn_grouped_scratch_doubles(biggest or max(groups), len(groups), C, H * W), len(groups) * C, C, N * C * H * W])
    third = R.bn_run(kernel, inp, DEV, F32)
    mask = got["y"] > 0 if relu else None
    ref = R.bn_run(R.bn_formula(relu, rows, tracked, None if mask is None else mask.cpu()), inp, "cpu", F64)
    eager = R.bn_run(R.bn_formula(relu, rows, tracked, mask), inp, DEV, F32)
    failures = []
    for name, kind in R.BN_TENSORS:
        if ref[name] is None:
            assert got[name] is None
            continue
        _same(name, [got[name], again[name], third[name]], failures)
        if kind == "channel" and len(groups) > 1:
            lo = 0
            for g, n in enumerate(groups):
                if n:
                    _judge(case, "%s group %d" % (name, g), kind, got[name][lo:lo + n], eager[name][lo:lo + n], ref[name][lo:lo + n], failures)
                lo += n
        else:
            _judge(case, name, kind, got[name], eager[name], ref[name], failures)
    for run in (got, again, third):
        if int(run["num_batches_tracked"]) != int(ref["num_batches_tracked"]):
            failures.append(("num_batches_tracked", int(run["num_batches_tracked"]), int(ref["num_batches_tracked"])))
    if relu:
        wrong, share = R.mask_report(got["y"], eager["z"], ref["z"])
        print("F64 | %s | mask: wrong outside the near-tie zone %d, share inside %.5f" % (case, wrong, share))
        if wrong or share > R.NEAR_TIE_CAP:
            failures.append(("mask", wrong, share))
    assert not failures, (case, failures)
    return got


@pytest.mark.parametrize("shape,variant,res,relu", R.bn_cases())
def test_batch_norm_against_float64(shape, variant, res, relu):
    gen = torch.Generator().manual_seed(R.bn_seed(shape, variant, res, relu))
    _bn_case("bn %s %s res=%d relu=%d" % (shape, variant, res, relu), R.bn_inputs(gen, shape, variant, res), relu)


@pytest.mark.parametrize("shape,rows,padding,res,relu", R.BN_GROUPED_CASES)
def test_grouped_batch_norm_against_float64_of_separate_calls(shape, rows, padding, res, relu):
    """`ops.bn_call_groups`: every group against the float64 reference of a separate call on its rows; the running
    statistics and num_batches_tracked see the tracked groups only."""
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(R.bn_seed(shape, "grouped", res, relu))
    _bn_case("bn grouped %s rows=%s padding=%d" % (shape, rows, padding), R.bn_inputs(gen, shape, "plain", res), relu, rows,
             len(rows) - padding, lambda: ops.bn_call_groups(rows, padding_groups=padding))


def test_device_table_batch_norm_against_float64_of_separate_calls():
    """`ops.bn_call_groups_device`: the group table lives on the device, group 2 is empty, two of the four groups are tracked."""
    from baseboostdepth_amd import ops
    shape, rows, tracked, biggest = R.BN_DEVICE_CASE
    table = torch.full((ops.BN_MAX_GROUPS + 2,), shape[0], dtype=torch.int32)
    table[0] = 0
    table[1:len(rows) + 1] = torch.tensor(rows).cumsum(0)
    table[ops.BN_MAX_GROUPS + 1] = tracked
    table = table.to(DEV)
    gen = torch.Generator().manual_seed(R.bn_seed(shape, "device", True, True))
    _bn_case("bn device table %s rows=%s tracked=%d" % (shape, rows, tracked), R.bn_inputs(gen, shape, "plain", True), True, rows,
             tracked, lambda: ops.bn_call_groups_device(table, len(rows), biggest), biggest)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", [(3, 5, 37, 79), (4, 6, 8, 16)])
def test_relu_mask_of_the_backward_is_the_forward_s(shape, res):
    """Upstream gradient of exactly +-1: sums of them are integers, exact in fp32 and in the fp64 partials, so grad_b must
    equal sum(dy * (y_kernel > 0)) exactly - one element masked differently in the backward (the mask re-derived from x
    when there is no residual, read from the saved y otherwise) is off by 1.  grad_res is dy * (y_kernel > 0) bit for bit."""
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(R.bn_seed(shape, "sharp", res, True))
    x, w, b, r, rm, rv, _ = [None if t is None else t.to(DEV) for t in R.bn_inputs(gen, shape, "plain", res)]
    dy = (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1).to(DEV)
    leaves = [t.requires_grad_(True) for t in (x, w, b)] + ([r.requires_grad_(True)] if res else [])
    y = ops.batch_norm_act(x, w, b, r, rm, rv, R.MOMENTUM, R.EPS, True)
    grads = torch.autograd.grad(y, leaves, dy)
    kept = dy * (y.detach() > 0)
    assert 0.2 < float((y > 0).float().mean()) < 0.8
    assert torch.equal(grads[2], kept.sum(dim=(0, 2, 3)))
    if res:
        assert torch.equal(grads[3], kept)


# ------------------------------------------------------------------------------------------------ reflection pad, up-sample + concat + pad
def _nchw_views(names):
    return [(n, "channel", lambda r, i=i: R.nhwc(r[i])) for i, n in enumerate(names)]


@pytest.mark.parametrize("shape", R.REFLECT_SHAPES)
def test_reflection_pad_against_float64(shape):
    from baseboostdepth_amd import ops
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = R.rounded(R.draw(gen, *shape) * R.channel_scales(gen, C, 10.0).reshape(1, C, 1, 1))
    up = R.rounded(R.draw(gen, N, C, H + 2, W + 2) * R.channel_scales(gen, C, 10.0).reshape(1, C, 1, 1))
    got, ref = _check("reflect_pad1 %s" % (shape,), ops.reflect_pad1, R.reflect_pad1, [x], [], [up], _nchw_views(["y", "grad x"]),
                      [N * C * (H + 2) * (W + 2)])
    assert torch.equal(got[0].cpu().double(), ref[0])                    # the forward is a copy


@pytest.mark.parametrize("N,C1,C2,h,w", R.UPCAT_CASES)
def test_upsample_concat_pad_against_float64(N, C1, C2, h, w):
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(N + C1 + h + w)
    Ct = C1 + (C2 or 0)
    x = R.rounded(R.draw(gen, N, C1, h, w) * R.channel_scales(gen, C1, 10.0).reshape(1, C1, 1, 1))
    skip = R.rounded(R.draw(gen, N, C2, 2 * h, 2 * w)) if C2 else None
    up = R.rounded(R.draw(gen, N, Ct, 2 * h + 2, 2 * w + 2) * R.channel_scales(gen, Ct, 10.0).reshape(1, Ct, 1, 1))
    assert ops.upcat_pad_supported(x.to(DEV), None if skip is None else skip.to(DEV))
    names = ["y", "grad x"] + (["grad skip"] if C2 else [])
    got, ref = _check("upcat_pad %s" % ((N, C1, C2, h, w),), ops.upcat_pad, R.upcat_pad, [x, skip], [], [up], _nchw_views(names),
                      [N * Ct * (2 * h + 2) * (2 * w + 2)])
    assert torch.equal(got[0].cpu().double(), ref[0])


# ------------------------------------------------------------------------------------------------ max-pool
def _maxpool_case(case, shape, special):
    from baseboostdepth_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    x, up = R.maxpool_inputs(gen, shape, special)
    ref = R.forward_backward(R.maxpool3s2, [x], [], [up], "cpu", F64)
    eager = R.forward_backward(R.maxpool3s2, [x], [], [up], DEV, F32)
    runs = [R.forward_backward(ops.maxpool3s2, [x], [], [up], DEV, F32)]
    runs.append(R.forward_backward(ops.maxpool3s2, [x], [], [up], DEV, F32))
    _poison([t.numel() for t in runs[0]] + [runs[0][0].numel() // 4 + 1])          # y, grad x and the byte-sized window codes
    runs.append(R.forward_backward(ops.maxpool3s2, [x], [], [up], DEV, F32))
    failures = []
    y, y64 = runs[0][0].cpu().double(), ref[0]
    if not torch.equal(torch.isnan(y), torch.isnan(y64)):
        failures.append(("y", "NaN positions differ"))
    if not torch.equal(torch.nan_to_num(y, nan=7.0), torch.nan_to_num(y64, nan=7.0)):          # +-inf stay themselves
        failures.append(("y", "not the reference's values"))
    for i, name in enumerate(("y", "grad x")):
        for other, what in zip(runs[1:], ("differs between two calls", "differs after NaN-filled blocks")):
            if not torch.equal(torch.nan_to_num(runs[0][i], nan=7.0), torch.nan_to_num(other[i], nan=7.0)):
                failures.append((name, what))
    assert bool(torch.isfinite(ref[1]).all())                            # no NaN is fed upstream: the gradients are finite
    _judge(case, "grad x", "channel", runs[0][1], eager[1], ref[1], failures)
    routed = (runs[0][1].cpu() != 0) == (ref[1] != 0)                    # the gradient lands where the first maximum is
    if not bool(routed.all()):
        failures.append(("grad x", "%d positions routed differently" % int((~routed).sum())))
    assert not failures, (case, failures)


@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES)
def test_max_pool_with_ties_against_float64(shape):
    _maxpool_case("maxpool3s2 %s" % (shape,), shape, None)


@pytest.mark.parametrize("special", ["-inf", "nan"])
def test_max_pool_with_infinities_and_nan_against_float64(special):
    _maxpool_case("maxpool3s2 (2, 3, 7, 130) %s" % special, (2, 3, 7, 130), special)


# ------------------------------------------------------------------------------------------------ bias + ELU
@pytest.mark.parametrize("shape", R.BIAS_ELU_SHAPES)
def test_bias_elu_against_float64(shape):
    from baseboostdepth_amd import ops
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    v, bias, up = R.bias_elu_inputs(gen, shape)
    views = _nchw_views(["y", "grad x"]) + [("grad bias", "tensor", lambda r: r[2])]
    got, _ = _check("bias_elu %s" % ((N, C, H * W),), lambda t, b: ops.bias_elu_(t * 1.0, b), R.bias_elu, [v, bias], [], [up], views,
                    [2 * _lib().bias_elu_scratch_doubles(N, C, H * W), C])
    flat = got[0][0, 0].reshape(-1)[:4].cpu()
    assert flat.tolist() == [0.0, 0.0, -1.0, -1.0] and not bool(torch.signbit(flat[0]))


# ------------------------------------------------------------------------------------------------ disparity head
DISP_VIEWS = _nchw_views(["y", "grad x"]) + [("grad weight", "tensor", lambda r: r[2]), ("grad bias", "tensor", lambda r: r[3])]


@pytest.mark.parametrize("shape", R.DISPCONV_SHAPES)
def test_disparity_head_against_float64(shape):
    from baseboostdepth_amd import ops
    N, C, H, W = shape
    x, w, b, up = R.dispconv_inputs(torch.Generator().manual_seed(sum(shape)), shape)
    _check("dispconv %s" % (shape,), ops.dispconv, R.dispconv, [x, w, b], [], [up], DISP_VIEWS,
           [2 * _lib().dispconv_scratch_doubles(C), N * C * H * W, N * H * W, 9 * C])


@pytest.mark.parametrize("shape", [(2, 5, 2, 3), (2, 16, 3, 8)])
def test_disparity_head_without_bias_and_with_one_gradient_only(shape):
    from baseboostdepth_amd import ops
    N, C, H, W = shape
    x, w, b, up = R.dispconv_inputs(torch.Generator().manual_seed(sum(shape) + 1), shape)
    scratch = [2 * _lib().dispconv_scratch_doubles(C), N * C * H * W, N * H * W, 9 * C]
    _check("dispconv %s bias=None" % (shape,), lambda t, k: ops.dispconv(t, k, None), lambda t, k: R.dispconv(t, k, None),
           [x, w], [], [up], DISP_VIEWS[:3], scratch)
    _check("dispconv %s grad x only" % (shape,), ops.dispconv, R.dispconv, [x], [w, b], [up], DISP_VIEWS[:2], scratch)
    _check("dispconv %s grad weight only" % (shape,), lambda k, t, c: ops.dispconv(t, k, c), lambda k, t, c: R.dispconv(t, k, c),
           [w], [x, b], [up], [DISP_VIEWS[0], ("grad weight", "tensor", lambda r: r[1])], scratch)


# ------------------------------------------------------------------------------------------------ whole modules
def _module_case(case, module, inputs, upstream, call, monkeypatch, forbidden=(), repeatable=True):
    """`call(module, *inputs)` -> a tensor or a list of tensors, on the GPU with the fused paths on, against the module's
    float64 copy on the CPU; the yardstick is the same module with ops.FUSED_NN off.  Every output, the gradient of every
    input and of every parameter.  `forbidden`: names of ops.* that the fused run must not reach (a shape the kernels
    refuse has to take the eager path).  `repeatable`: three runs must agree bit for bit."""
    from baseboostdepth_amd import ops
    params = [n for n, _ in module.named_parameters()]

    def refuse(name):
        def fn(*args, **kwargs):
            raise AssertionError("%s: ops.%s was called" % (case, name))
        return fn

    def run(mod, device, dtype, fused):
        with monkeypatch.context() as m:
            m.setattr(ops, "FUSED_NN", fused)
            for name in (forbidden if fused else ()):
                m.setattr(ops, name, refuse(name))
            xs = [t.to(device=device, dtype=dtype).clone().requires_grad_(True) for t in inputs]
            for p in mod.parameters():
                p.grad = None
            out = call(mod, *xs)
            outs = list(out) if isinstance(out, (list, tuple)) else [out]
            sum((o * u.to(device=device, dtype=dtype)).sum() for o, u in zip(outs, upstream)).backward()
            return [o.detach() for o in outs] + [t.grad for t in xs] + [p.grad.clone() for p in mod.parameters()]
    ref = run(R.float64_copy(module), "cpu", F64, False)
    module = module.to(DEV)
    eager = run(module, DEV, F32, False)
    got = run(module, DEV, F32, True)
    again = run(module, DEV, F32, True)
    _poison([t.numel() for t in got])
    third = run(module, DEV, F32, True)
    n_act = len(ref) - len(params)
    names = ["output %d" % i for i in range(len(upstream))] + ["grad input %d" % i for i in range(len(inputs))] + params
    failures = []
    for i, name in enumerate(names):
        kind = "channel" if i < n_act else "tensor"
        if repeatable:
            _same(name, [got[i], again[i], third[i]], failures)
        for r in (got, again, third) if not repeatable else (got,):
            _judge(case, name, kind, r[i], eager[i], ref[i], failures)
    assert not failures, (case, failures)


def _scaled(gen, *shape):
    return R.rounded(R.draw(gen, *shape) * R.channel_scales(gen, shape[1], 10.0, -1.0, 1.0).reshape(1, -1, 1, 1))


def test_reflection_pad_module_takes_the_eager_path_past_65535_planes(monkeypatch):
    from baseboostdepth_amd.layers import ReflectionPad1
    shape = R.FALLBACKS["reflect_pad1 planes"]
    gen = torch.Generator().manual_seed(1)
    x, up = R.rounded(R.draw(gen, *shape)), R.rounded(R.draw(gen, shape[0], shape[1], shape[2] + 2, shape[3] + 2))
    _module_case("fallback reflect_pad1 %s" % (shape,), ReflectionPad1(), [x], [up], lambda m, t: m(t), monkeypatch, ["reflect_pad1"])


@pytest.mark.parametrize("which", ["ConvBlock out_hw % 4", "ConvBlock bias=None"])
def test_conv_block_on_a_padded_input_takes_the_eager_path(which, monkeypatch):
    from baseboostdepth_amd.layers import ConvBlock
    shape = R.FALLBACKS[which]
    N, C, H, W = shape
    torch.manual_seed(2)
    blk = ConvBlock(C, 4)
    if which.endswith("None"):
        blk.conv.conv.bias = None
    gen = torch.Generator().manual_seed(2)
    xp, up = _scaled(gen, N, C, H + 2, W + 2), _scaled(gen, N, 4, H, W)
    _module_case("fallback %s %s" % (which, shape), blk, [xp], [up], lambda m, t: m.forward_padded(t), monkeypatch, ["bias_elu_"])


def test_conv3x3_to_one_channel_falls_back_past_256_input_channels(monkeypatch):
    from baseboostdepth_amd.layers import Conv3x3
    shape = R.FALLBACKS["Conv3x3(257, 1)"]
    torch.manual_seed(3)
    conv = Conv3x3(shape[1], 1)
    gen = torch.Generator().manual_seed(3)
    x, up = _scaled(gen, *shape), R.rounded(R.draw(gen, shape[0], 1, shape[2], shape[3]))
    _module_case("fallback Conv3x3(257, 1) %s" % (shape,), conv, [x], [up], lambda m, t: m(t), monkeypatch, ["dispconv"])


DECODER_IMAGE = (64, 128)


def test_depth_decoder_against_its_float64_copy(monkeypatch):
    """DepthDecoder on a ResNet-18 pyramid with every fusion on (upcat_pad, bias_elu_, dispconv, reflect_pad1): the four
    disparities and every parameter gradient.  No ReLU in it, so no mask protocol.  The image is 64 x 128: the coarsest
    feature is then 2 x 4, the smallest a reflection border of one pixel admits (32 x 64 would leave it 1 x 2).
    MIOpen's default choice for the convolutions of the two coarsest levels (512 -> 256 at 2 x 4, 256 -> 256 at 4 x 8)
    returns other last bits from call to call, with the fusions on or off; the case asks MIOpen for its deterministic
    solvers, and the three runs must then agree bit for bit like every other case's."""
    from baseboostdepth_amd import networks
    H, W = DECODER_IMAGE
    torch.manual_seed(4)
    dec = networks.DepthDecoder([64, 64, 128, 256, 512], [0, 1, 2, 3]).train()
    gen = torch.Generator().manual_seed(4)
    feats = [R.rounded(R.draw(gen, 2, c, H >> (i + 1), W >> (i + 1)).abs()) for i, c in enumerate([64, 64, 128, 256, 512])]
    ups = [R.rounded(R.draw(gen, 2, 1, H >> s, W >> s)) for s in range(4)]
    with torch.backends.cudnn.flags(deterministic=True):
        _module_case("decoder %dx%d" % (H, W), dec, feats, ups, lambda m, *f: [m(list(f))[("disp", s)] for s in range(4)], monkeypatch)
