"""GPU tier: the disparity head with its sigmoid inside (`ops.disp_head`, bbd_disp_head_fwd / _bwd) against float64.

The reference is `torch.sigmoid(R.dispconv(...))` in float64 on the CPU, the yardstick the same formula in fp32 on the
GPU, the bound `R.bound` of the eager error - all through `gpu_f64_common.check`, which also runs every case three times
(the third after NaN-filled allocator blocks) and wants equal bits.

Shapes: `R.DISPCONV_SHAPES` (W % 4 != 0, C = 1, C = 256, 2-pixel images, the weight kernel's second grid-stride turn) and
RAGGED = (2, 13, 5, 12): 13 channels are three whole groups of the kernels' four-channel unrolling and one left over, so
the weight kernel's ragged last group runs, and 13 is no multiple of the 16 parts that divide the channels of a small
forward either; H = 5 leaves the last strip task with one row.  How far the channels are divided depends on the size
(forward: 16 parts below 16 384 tasks, 4 from there on; data gradient: up to C workgroups per strip below 65 536 strips):
every shape here but (2, 3, 128, 260) takes the finest division, that one the coarsest.

Measured on an MI355X (eager error, kernel error, ratio): the largest ratio is 2.65, grad bias of (2, 16, 3, 8)
(4.97e-08 against 1.58e-07, at the bound's floor of 4.77e-07); every other tensor is below 1.6.
"""
import pytest
import torch

import nn_f64_ref as R
from gpu_f64_common import check as _check
from test_gpu_nn_f64 import DECODER_IMAGE, _module_case, _nchw_views

pytestmark = pytest.mark.gpu

RAGGED = (2, 13, 5, 12)
HEAD_VIEWS = _nchw_views(["y", "grad x"]) + [("grad weight", "tensor", lambda r: r[2]), ("grad bias", "tensor", lambda r: r[3])]


def _formula(x, w, b):
    return torch.sigmoid(R.dispconv(x, w, b))


def _scratch(shape):
    from baseboostdepth_amd import ops
    N, C, H, W = shape
    return [2 * ops.default_backend().lib.dispconv_scratch_doubles(C), N * C * H * W, N * H * W, 9 * C]


@pytest.mark.parametrize("shape", R.DISPCONV_SHAPES + [RAGGED])
def test_disp_head_against_float64(shape):
    from baseboostdepth_amd import ops
    x, w, b, up = R.dispconv_inputs(torch.Generator().manual_seed(sum(shape) + 2), shape)
    _check("disp_head %s" % (shape,), ops.disp_head, _formula, [x, w, b], [], [up], HEAD_VIEWS, _scratch(shape))


@pytest.mark.parametrize("shape", [(2, 5, 2, 3), (2, 16, 3, 8), RAGGED])
def test_disp_head_without_bias_and_with_one_gradient_only(shape):
    from baseboostdepth_amd import ops
    x, w, b, up = R.dispconv_inputs(torch.Generator().manual_seed(sum(shape) + 3), shape)
    scratch = _scratch(shape)
    _check("disp_head %s bias=None" % (shape,), lambda t, k: ops.disp_head(t, k, None), lambda t, k: _formula(t, k, None),
           [x, w], [], [up], HEAD_VIEWS[:3], scratch)
    _check("disp_head %s grad x only" % (shape,), ops.disp_head, _formula, [x], [w, b], [up], HEAD_VIEWS[:2], scratch)
    _check("disp_head %s grad weight only" % (shape,), lambda k, t, c: ops.disp_head(t, k, c), lambda k, t, c: _formula(t, k, c),
           [w], [x, b], [up], [HEAD_VIEWS[0], ("grad weight", "tensor", lambda r: r[1])], scratch)


@pytest.mark.parametrize("shape", [(2, 5, 2, 3), RAGGED])
def test_dispconv_still_returns_the_convolution_itself(shape):
    """`ops.dispconv` shares the device code with the head; the sigmoid must stay out of it both ways."""
    from baseboostdepth_amd import ops
    x, w, b, up = R.dispconv_inputs(torch.Generator().manual_seed(sum(shape) + 4), shape)
    _check("dispconv %s" % (shape,), ops.dispconv, R.dispconv, [x, w, b], [], [up], HEAD_VIEWS, _scratch(shape))


def test_depth_decoder_through_the_head_against_its_float64_copy(monkeypatch):
    """`test_depth_decoder_against_its_float64_copy` with the four disparities required to come from `ops.disp_head`
    and none from `ops.dispconv` (64 x 128 image, MIOpen's deterministic solvers - see there)."""
    from baseboostdepth_amd import networks, ops
    H, W = DECODER_IMAGE
    torch.manual_seed(5)
    dec = networks.DepthDecoder([64, 64, 128, 256, 512], [0, 1, 2, 3]).train()
    gen = torch.Generator().manual_seed(5)
    feats = [R.rounded(R.draw(gen, 2, c, H >> (i + 1), W >> (i + 1)).abs()) for i, c in enumerate([64, 64, 128, 256, 512])]
    ups = [R.rounded(R.draw(gen, 2, 1, H >> s, W >> s)) for s in range(4)]
    calls, head = [], ops.disp_head

    def counted(x, weight, bias, backend=None):
        calls.append(tuple(x.shape))
        return head(x, weight, bias, backend)
    monkeypatch.setattr(ops, "disp_head", counted)
    with torch.backends.cudnn.flags(deterministic=True):
        _module_case("decoder head %dx%d" % (H, W), dec, feats, ups, lambda m, *f: [m(list(f))[("disp", s)] for s in range(4)],
                     monkeypatch, ["dispconv"])
    # three fused runs, each calling the decoder once per output it picks
    assert len(calls) == 3 * 4 * 4 and set(calls) == {(2, 16 << s, H >> s, W >> s) for s in range(4)}
