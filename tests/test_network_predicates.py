"""CPU tier: the predicates that say which path an encoder / decoder layer takes (ops.*_supported beside each fused op;
DESIGN.md, "which path a layer takes").  One truth table per predicate added with them, written down from the condition
the module held before (kept here as `old`), and on every row the predicate, the table and that condition agree."""
import pytest
import torch

F32, F16 = torch.float32, torch.float16


class Fake:
    """what a predicate asks of a tensor"""

    def __init__(self, *shape, cuda=True, dtype=F32):
        self.shape, self.is_cuda, self.dtype = torch.Size(shape), cuda, dtype

    def dim(self):
        return len(self.shape)


@pytest.fixture
def ops(monkeypatch):
    from baseboostdepth_amd import ops
    for name in ("FUSED_NN", "FUSED_STEM", "FUSED_DECODER_GLUE"):
        monkeypatch.setattr(ops, name, True)
    return ops


def _agree(rows, new, old):
    for want, args in rows:
        assert bool(new(*args)) is want, args[0].shape
        assert bool(old(*args)) is want, args[0].shape


def test_the_shared_names(ops):
    assert ops.MAX_PLANES == 65535 and ops.DISP_HEAD_MAX_CHANNELS == 256
    assert ops.hip_fp32() and ops.hip_fp32(Fake(1), None, Fake(2, 3))
    assert not ops.hip_fp32(Fake(1, cuda=False)) and not ops.hip_fp32(Fake(1), Fake(1, dtype=F16))
    assert not ops.hip_fp32(torch.zeros(1)) and not ops.hip_fp32(Fake(1, dtype=torch.float64))


def test_reflect_pad1(ops, monkeypatch):
    def old(x):             # layers.ReflectionPad1.forward
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and min(x.shape[2:]) >= 2 and ops.FUSED_NN
                and x.shape[0] * x.shape[1] <= 65535)
    rows = [(True, (Fake(2, 16, 8, 8),)), (True, (Fake(1, 65535, 2, 2),)), (True, (Fake(255, 257, 3, 2),)),
            (False, (Fake(1, 65536, 2, 2),)), (False, (Fake(256, 256, 8, 8),)),
            (False, (Fake(1, 1, 1, 2),)), (False, (Fake(1, 1, 2, 1),)), (True, (Fake(1, 1, 2, 2),)),
            (False, (Fake(4, 8, 8),)), (False, (Fake(2, 16, 8, 8, dtype=F16),)), (False, (Fake(2, 16, 8, 8, cuda=False),))]
    _agree(rows, ops.reflect_pad1_supported, old)
    monkeypatch.setattr(ops, "FUSED_NN", False)
    _agree([(False, r[1]) for r in rows], ops.reflect_pad1_supported, old)


def test_maxpool3s2(ops, monkeypatch):
    def old(x):             # networks.encoder.MaxPool3s2.forward
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and ops.FUSED_NN
                and x.shape[0] * x.shape[1] <= 65535)
    rows = [(True, (Fake(2, 64, 32, 64),)), (True, (Fake(1, 65535, 2, 2),)), (False, (Fake(1, 65536, 2, 2),)),
            (True, (Fake(1, 1, 1, 1),)), (True, (Fake(1, 1, 1, 2),)), (False, (Fake(64, 32, 64),)),
            (False, (Fake(2, 64, 32, 64, dtype=F16),)), (False, (Fake(2, 64, 32, 64, cuda=False),))]
    _agree(rows, ops.maxpool3s2_supported, old)
    monkeypatch.setattr(ops, "FUSED_NN", False)
    _agree([(False, r[1]) for r in rows], ops.maxpool3s2_supported, old)


def test_bias_elu_(ops, monkeypatch):
    def old(x, border):     # layers.ConvBlock._fused (border 0) and .forward_padded (border 1), the module's part taken out
        hw = (x.shape[2] - 2 * border) * (x.shape[3] - 2 * border)
        return x.is_cuda and x.dtype == torch.float32 and ops.FUSED_NN and hw % 4 == 0
    rows = [(True, (Fake(2, 16, 2, 2), 0)), (True, (Fake(2, 16, 1, 4), 0)), (True, (Fake(2, 16, 6, 6), 0)),
            (False, (Fake(2, 16, 1, 2), 0)), (False, (Fake(2, 16, 3, 3), 0)), (False, (Fake(2, 16, 5, 6), 0)),
            (True, (Fake(2, 16, 4, 4), 1)), (False, (Fake(2, 16, 5, 5), 1)), (True, (Fake(2, 16, 3, 6), 1)),
            (False, (Fake(2, 16, 4, 5), 1)), (True, (Fake(1, 65536, 2, 2), 0)),           # no plane limit: a 1-D grid
            (False, (Fake(2, 16, 2, 2, dtype=F16), 0)), (False, (Fake(2, 16, 2, 2, cuda=False), 0)),
            (False, (Fake(2, 16, 4, 4, dtype=F16), 1)), (False, (Fake(2, 16, 4, 4, cuda=False), 1))]
    _agree(rows, ops.bias_elu_supported, old)
    assert ops.bias_elu_supported(Fake(2, 16, 2, 2))
    monkeypatch.setattr(ops, "FUSED_NN", False)
    _agree([(False, r[1]) for r in rows], ops.bias_elu_supported, old)


def test_disparity_head(ops, monkeypatch):
    def old(x, in_channels):    # layers.Conv3x3._fused, the module's part (one output channel, a ReflectionPad1) taken out
        return (x.is_cuda and x.dtype == torch.float32 and ops.FUSED_NN and in_channels <= 256
                and min(x.shape[2:]) >= 2)

    def case(N, C, H, W, **kw):
        return Fake(N, C, H, W, **kw), C
    rows = [(True, case(2, 16, 8, 8)), (True, case(1, 256, 2, 2)), (False, case(1, 257, 2, 2)),
            (False, case(1, 16, 1, 2)), (False, case(1, 16, 2, 1)), (True, case(1, 1, 2, 2)),
            (False, case(2, 16, 8, 8, dtype=F16)), (False, case(2, 16, 8, 8, cuda=False))]
    _agree(rows, ops.disp_head_supported, old)
    monkeypatch.setattr(ops, "FUSED_NN", False)
    _agree([(False, r[1]) for r in rows], ops.disp_head_supported, old)


def test_batch_norm_act(ops, monkeypatch):
    def old(x):             # networks.encoder.FusedBatchNorm2d.forward, the module's part taken out
        return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    rows = [(True, (Fake(2, 64, 8, 8),)), (True, (Fake(1, 65536, 1, 1),)), (False, (Fake(2, 64, 8),)),
            (False, (Fake(2, 64, 8, 8, dtype=F16),)), (False, (Fake(2, 64, 8, 8, cuda=False),))]
    _agree(rows, ops.batch_norm_act_supported, old)
    monkeypatch.setattr(ops, "FUSED_NN", False)             # not this op's switch: FusedBatchNorm2d.fused is
    _agree(rows, ops.batch_norm_act_supported, old)


def test_the_module_keeps_its_own_part(ops):
    """`FusedBatchNorm2d.takes_fused_launches`: switch and mode of the module; `Conv3x3._fused` / `ConvBlock._fused`: what
    the layer is."""
    from baseboostdepth_amd import layers
    from baseboostdepth_amd.networks.encoder import FusedBatchNorm2d
    x = Fake(2, 8, 4, 4)
    bn = FusedBatchNorm2d(8)
    before = FusedBatchNorm2d.fused
    try:
        FusedBatchNorm2d.fused = True
        assert bn.takes_fused_launches(x) and not bn.takes_fused_launches(Fake(2, 8, 4, 4, cuda=False))
        assert not bn.eval().takes_fused_launches(x) and bn.train().takes_fused_launches(x)
        assert not FusedBatchNorm2d(8, affine=False).takes_fused_launches(x)
        assert not FusedBatchNorm2d(8, track_running_stats=False).takes_fused_launches(x)
        assert not FusedBatchNorm2d(8, momentum=None).takes_fused_launches(x)
        FusedBatchNorm2d.fused = False
        assert not bn.takes_fused_launches(x)
    finally:
        FusedBatchNorm2d.fused = before
    assert layers.Conv3x3(8, 1)._fused(x) and not layers.Conv3x3(8, 2)._fused(x)
    assert not layers.Conv3x3(8, 1, use_refl=False)._fused(x) and not layers.Conv3x3(300, 1)._fused(Fake(2, 300, 4, 4))
    block, head_block = layers.ConvBlock(8, 4), layers.ConvBlock(8, 1)
    assert block._fused(x) and block._fused(Fake(2, 8, 6, 6), 1) and not block._fused(Fake(2, 8, 5, 5))
    assert not head_block._fused(x) and head_block._fused(Fake(2, 8, 6, 6), 1)     # one channel: only behind a border
    block.conv.conv.bias = None
    assert not block._fused(x) and not block._fused(Fake(2, 8, 6, 6), 1)


def test_the_stem_takes_what_the_pool_and_the_library_take(ops, monkeypatch):
    def old(x):             # networks.encoder.ResnetEncoder._stem, the BatchNorm module's part taken out
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] * x.shape[1] <= 65535
                and ops.FUSED_NN and ops.FUSED_STEM and ops.stem_supported(x, ops.call_groups(x.shape[0]).biggest))
    rows = [(True, (Fake(12, 64, 96, 320),)), (False, (Fake(2, 64, 32, 64),)), (True, (Fake(2, 64, 64, 128),)),
            (False, (Fake(2, 64, 64, 126),)), (True, (Fake(1, 65535, 2, 8192),)), (False, (Fake(1, 65536, 2, 8192),)),
            (False, (Fake(12, 64, 96, 320, dtype=F16),)), (False, (Fake(12, 64, 96, 320, cuda=False),))]
    _agree(rows, ops.stem_routed, old)
    for switch in ("FUSED_NN", "FUSED_STEM"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            _agree([(False, r[1]) for r in rows], ops.stem_routed, old)


def test_every_switch_is_read_by_the_one_helper(monkeypatch):
    from baseboostdepth_amd import ops
    monkeypatch.delenv("BBD_SOME_SWITCH", raising=False)
    assert ops.switch("BBD_SOME_SWITCH") is True
    for value, want in (("0", False), ("1", True), ("", True), ("off", True)):
        monkeypatch.setenv("BBD_SOME_SWITCH", value)
        assert ops.switch("BBD_SOME_SWITCH") is want
