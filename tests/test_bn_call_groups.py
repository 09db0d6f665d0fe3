"""CPU tier: the one description of BatchNorm call groups (`ops.CallGroups`, `ops.bn_call_groups`,
`ops.bn_call_groups_device`, `ops.call_groups`) from the autograd functions down to the argument lists of the
`bbd_bn_act_grouped*` / `bbd_stem*` entry points, the host check of a packed group table (`ops.check_group_table`,
`pooled.PooledTables`) and the stand-alone walk of the C side's group resolution under the sanitizers
(tests/sanitize/bn_groups_main.cpp).  The kernels themselves: tests/test_gpu_nn.py, test_gpu_stem.py, test_gpu_pooled.py,
test_gpu_bn_call_groups.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from baseboostdepth_amd import ops, pooled, tuning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, C, H, W = 5, 3, 4, 8
ROWS, PADDING = [2, 1, 2], 1
DEV_G, DEV_BOUND = 8, 3


class Recorder:
    """A backend that launches nothing and keeps the argument lists."""
    name = "recorder"

    class lib:
        bn_grouped_scratch_doubles = staticmethod(lambda rows, G, C, HW: 6)

    def __init__(self):
        self.calls = []

    def _check(self, *tensors):
        pass

    def run(self, name, anchor, *args):
        self.calls.append((name, args))


def _device_table():
    table = torch.full((ops.BN_MAX_GROUPS + 2,), N, dtype=torch.int32)
    table[:len(ROWS) + 1] = torch.tensor([0, 2, 3, 5])
    table[ops.BN_MAX_GROUPS + 1] = len(ROWS) - PADDING
    return table


TABLE = _device_table()
# description -> (scope, entry-point infix, G, the integers behind the table forward, backward)
DESCRIPTIONS = {
    "none": (lambda: ops.bn_call_groups(None), "", 1, (1, 0), (1,)),
    "host": (lambda: ops.bn_call_groups(ROWS, padding_groups=PADDING), "", 3, (3, PADDING), (3,)),
    "device": (lambda: ops.bn_call_groups_device(TABLE, DEV_G, DEV_BOUND), "_dev", DEV_G, (DEV_G, DEV_BOUND), (DEV_G, DEV_BOUND)),
}


def _table_matches(arg, how):
    if how == "device":
        return arg.value == TABLE.data_ptr()
    return list(arg) == {"none": [0, N], "host": [0, 2, 3, 5]}[how]


@pytest.mark.parametrize("how", list(DESCRIPTIONS))
def test_batch_norm_act_hands_the_description_to_one_entry_point_each_way(how):
    scope, infix, G, fwd_ints, bwd_ints = DESCRIPTIONS[how]
    be = Recorder()
    x = torch.randn(N, C, H, W, requires_grad=True)
    w, b = torch.ones(C, requires_grad=True), torch.zeros(C, requires_grad=True)
    with scope():
        y = ops.batch_norm_act(x, w, b, None, torch.zeros(C), torch.ones(C), 0.1, 1e-5, True, backend=be,
                               num_batches_tracked=torch.zeros((), dtype=torch.int64))
    mean, invstd = y.grad_fn.saved_tensors[4:6]
    y.backward(torch.ones_like(y))            # (outside the scope: the backward has the description from the forward)
    (fname, fargs), (bname, bargs) = be.calls
    assert fname == "bbd_bn_act_grouped%s_fwd" % infix and bname == "bbd_bn_act_grouped%s_bwd" % infix
    # x, residual, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch | table
    assert _table_matches(fargs[11], how)
    assert fargs[12:] == fwd_ints + (N, C, H * W, 1e-5, 0.1, 1)
    # x, y, grad_y, gamma, beta, save_mean, save_invstd, grad_x, grad_residual, grad_gamma, grad_beta, scratch | table
    assert _table_matches(bargs[12], how)
    assert bargs[13:] == bwd_ints + (N, C, H * W, 1)
    assert mean.shape == (G, C) and invstd.shape == (G, C)
    assert fargs[5].value == mean.data_ptr() and bargs[5].value == mean.data_ptr()


@pytest.mark.parametrize("how", list(DESCRIPTIONS))
def test_stem_hands_the_description_to_one_entry_point_each_way(how):
    scope, infix, G, fwd_ints, bwd_ints = DESCRIPTIONS[how]
    be = Recorder()
    x = torch.randn(N, C, H, W, requires_grad=True)
    w, b = torch.ones(C, requires_grad=True), torch.zeros(C, requires_grad=True)
    with scope():
        y, p = ops.stem_bn_relu_pool(x, w, b, torch.zeros(C), torch.ones(C), 0.1, 1e-5, backend=be,
                                     num_batches_tracked=torch.zeros((), dtype=torch.int64))
    mean, invstd = p.grad_fn.saved_tensors[4:6]
    (y.sum() + p.sum()).backward()
    (fname, fargs), (bname, bargs) = be.calls
    assert fname == "bbd_stem%s_fwd" % infix and bname == "bbd_stem%s_bwd" % infix
    # x, gamma, beta, y, pooled, code, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, scratch | table
    assert _table_matches(fargs[12], how)
    assert fargs[13:] == fwd_ints + (N, C, H, W, 1e-5, 0.1)
    # x, grad_y, grad_pooled, code, gamma, beta, save_mean, save_invstd, grad_x, grad_gamma, grad_beta, scratch | table
    assert _table_matches(bargs[12], how)
    assert bargs[13:] == bwd_ints + (N, C, H, W)
    assert mean.shape == (G, C) and invstd.shape == (G, C) and p.shape == (N, C, H // 2, W // 2)
    assert fargs[6].value == mean.data_ptr() and bargs[6].value == mean.data_ptr()


# ------------------------------------------------------------------------------------------ the description object
def description_cases():
    """Every way a description can fail to describe a batch of N rows is a ValueError (never an assert: `python -O`)."""
    host = lambda rows, untracked=0: ops.CallGroups(tuple(rows), untracked, None, None, None)
    with pytest.raises(ValueError, match="does not describe this batch"):
        host([2, 2]).check(N)
    with pytest.raises(ValueError):
        host([3, 0, 2]).check(N)
    with pytest.raises(ValueError):
        ops.bn_call_groups([3, 0, 2])
    with pytest.raises(ValueError):
        host([1] * (ops.BN_MAX_GROUPS + 1)).check(ops.BN_MAX_GROUPS + 1)
    with pytest.raises(ValueError):
        ops.bn_call_groups([1] * (ops.BN_MAX_GROUPS + 1))
    with pytest.raises(ValueError):
        host([2, 3], untracked=2).check(N)
    with pytest.raises(ValueError):
        ops.bn_call_groups([2, 3], padding_groups=2)
    with pytest.raises(ValueError):
        ops.CallGroups(None, None, TABLE, DEV_G, N + 1).check(N)
    with pytest.raises(ValueError):
        ops.bn_call_groups_device(TABLE, ops.BN_MAX_GROUPS + 1, 2)
    with pytest.raises(ValueError):
        ops.bn_call_groups_device(TABLE[:8], 4, 2)
    with ops.bn_call_groups([2, 3]):
        with pytest.raises(ValueError, match="together"):
            with ops.bn_call_groups_device(TABLE, DEV_G, DEV_BOUND):
                pass
    with ops.bn_call_groups_device(TABLE, DEV_G, DEV_BOUND):
        with pytest.raises(ValueError, match="together"):
            with ops.bn_call_groups([2, 3]):
                pass
    # ... and in the autograd functions, before anything is allocated or launched
    be = Recorder()
    x, w, b = torch.randn(N, C, H, W), torch.ones(C), torch.zeros(C)
    for scope in (lambda: ops.bn_call_groups([2, 2]), lambda: ops.bn_call_groups_device(TABLE, DEV_G, N + 1)):
        with scope():
            with pytest.raises(ValueError):
                ops.batch_norm_act(x, w, b, None, None, None, 0.1, 1e-5, True, backend=be)
            with pytest.raises(ValueError):
                ops.stem_bn_relu_pool(x, w, b, None, None, 0.1, 1e-5, backend=be)
    if be.calls or ops.call_groups(N).rows != (N,):
        raise RuntimeError("a refused description reached a launch, or is still active")


def test_a_description_that_does_not_fit_is_a_value_error():
    description_cases()


def test_the_same_cases_raise_under_python_O():
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_bn_call_groups as t; assert False, 'asserts are on'; "
            "t.description_cases(); print('raised')" % (ROOT, os.path.join(ROOT, "tests")))
    done = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "raised", done.stderr[-2000:]


def test_accessors_of_both_descriptions():
    one = ops.call_groups(7)
    assert (one.G, one.biggest, one.infix, one.untracked) == (1, 7, "", 0)
    with ops.bn_call_groups(ROWS, padding_groups=PADDING):
        g = ops.call_groups(N)
        assert (g.G, g.biggest, g.infix) == (3, 2, "") and g.check(N) is g
        table, G, untracked = g.fwd_args()
        assert list(table) == [0, 2, 3, 5] and (G, untracked) == (3, PADDING) and len(g.bwd_args()) == 2
    with ops.bn_call_groups_device(TABLE, DEV_G, DEV_BOUND):
        g = ops.call_groups(N)
        assert (g.G, g.biggest, g.infix) == (DEV_G, DEV_BOUND, "_dev") and g.check(N) is g
        assert g.fwd_args()[1:] == g.bwd_args()[1:] == (DEV_G, DEV_BOUND)
    with pytest.raises(AttributeError):
        g.bound = 1


def test_the_slot_is_restored_after_nesting_and_after_an_exception():
    outer = ops.bn_call_groups([2, 3])
    with outer:
        assert ops.call_groups(5).rows == (2, 3)
        with ops.bn_call_groups([1, 1, 3], padding_groups=1):
            assert ops.call_groups(5).rows == (1, 1, 3) and ops.call_groups(5).untracked == 1
            with ops.bn_call_groups([5]):                 # one group or None: no groups
                assert ops.call_groups(5).rows == (5,)
            assert ops.call_groups(5).rows == (1, 1, 3)
        assert ops.call_groups(5).rows == (2, 3) and ops.call_groups(5).untracked == 0
        with pytest.raises(KeyError):
            with ops.bn_call_groups([4, 1]):
                raise KeyError("inside")
        assert ops.call_groups(5).rows == (2, 3)
    assert ops.call_groups(5).rows == (5,)
    with pytest.raises(KeyError):
        with ops.bn_call_groups_device(TABLE, DEV_G, DEV_BOUND):
            assert ops.call_groups(5).table is TABLE
            raise KeyError("inside")
    assert ops.call_groups(5).rows == (5,)


def test_the_stock_batch_norm_refuses_call_groups_with_a_runtime_error(monkeypatch):
    """`FusedBatchNorm2d` off its fused path cannot keep statistics per group: a programming error, raised also under -O."""
    from baseboostdepth_amd.networks.encoder import FusedBatchNorm2d
    bn = FusedBatchNorm2d(C).train()
    monkeypatch.setattr(bn, "fused", False)

    class OnDevice(torch.Tensor):                       # a host tensor that says it is on the GPU: the check is host logic
        is_cuda = True

    x = torch.randn(N, C, H, W).as_subclass(OnDevice)
    assert bn(x).shape == x.shape
    for scope in (ops.bn_call_groups(ROWS), ops.bn_call_groups_device(TABLE, DEV_G, DEV_BOUND)):
        with scope, pytest.raises(RuntimeError, match="fused BatchNorm"):
            bn(x)


# ------------------------------------------------------------------------------------------ the packed group table
def _tables(ms=(7, 5, 4, 3), caps_B=None):
    from baseboostdepth_amd.plan import get_plan
    B = len(ms)
    caps = pooled.Caps(caps_B or B)
    layout = pooled.Layout(caps)
    frames = list(range(-max(ms), max(ms) + 1))
    plan = get_plan([[0, m, -m] for m in ms], True, True)
    build = lambda: pooled.PooledTables(plan, frames, sorted(frames, key=abs), True, True, True, True, caps, layout, 32,
                                        tuning.padded_pose_rows(4 * B, 32), False)
    return build, layout


def test_group_table_check_takes_a_packed_table_and_refuses_edited_ones():
    build, layout = _tables()
    tab = build()
    good = layout.view(tab.host.numpy(), "groups").copy()
    MAXG = ops.BN_MAX_GROUPS
    ops.check_group_table(good, tab.G, tab.bound, tab.R)
    sizes = np.diff(good[:MAXG + 1])
    real = int((sizes > 0).sum())
    assert 2 <= real < tab.G and good[MAXG + 1] >= 1

    def edited(**at):
        bad = good.copy()
        for i, v in at.items():
            bad[int(i[1:])] = v
        return bad
    k = next(k for k in range(2, real + 1) if good[k] > tab.bound)
    over = edited(**{"i%d" % (MAXG + 1): 0})
    over[1:k] = good[k]                                # the first k groups become one of more than `bound` rows and empty ones
    cases = {
        "a group above the bound": over,
        "a decreasing row": edited(**{"i2": good[1] - 1}),
        "a tail that is not R": edited(**{"i%d" % MAXG: tab.R - 1}),
        "rows behind G that are not R": edited(**{"i%d" % tab.G: tab.R - 1}),
        "rows[0] != 0": edited(i0=1),
        "more tracked groups than groups": edited(**{"i%d" % (MAXG + 1): real + 1}),
        "a negative tracked count": edited(**{"i%d" % (MAXG + 1): -1}),
    }
    assert np.diff(over[:MAXG + 1]).max() > tab.bound and np.diff(over[:MAXG + 1]).min() >= 0
    ops.check_group_table(over, tab.G, int(good[k]), tab.R)              # (refused for its bound alone)
    for what, bad in cases.items():
        print(what)
        with pytest.raises(ValueError):
            ops.check_group_table(bad, tab.G, tab.bound, tab.R)
    with pytest.raises(ValueError):
        ops.check_group_table(good, real - 1, tab.bound, tab.R)          # a grid of fewer groups than the table has
    with pytest.raises(ValueError):
        ops.check_group_table(good, MAXG + 1, tab.bound, tab.R)


def test_a_batch_that_does_not_fit_falls_back_instead_of_killing_the_step():
    import types
    build, _ = _tables(caps_B=5)                     # plan.B != caps.B
    with pytest.raises(ValueError):
        build()
    ms = [7, 5, 4, 3]
    from baseboostdepth_amd.plan import get_plan
    opt = types.SimpleNamespace(batch_size=5, height=16, width=24, trimin=True, decomp=True, incremental_skip=True,
                                partial_skip=True, frame_ids=sorted(range(-7, 8), key=abs))
    tr = types.SimpleNamespace(opt=opt, device=torch.device("cpu"), pose_pad_rows=32, maxing_valid_frames=True)
    ps = pooled.PooledStep(tr)
    plan = get_plan([[0, m, -m] for m in ms], True, True)
    assert ps.tables_for(plan, {"frames": list(range(-7, 8))}) is None
    assert ps.stats["fallbacks"] == 1 and ps.stats["builds"] == 1
    assert ps.tables_for(plan, {"frames": list(range(-7, 8))}) is None         # cached: counted once
    assert ps.stats["fallbacks"] == 1


# ------------------------------------------------------------------------------------------ the C side, under the sanitizers
def test_group_resolution_of_the_entry_points_under_the_sanitizers(tmp_path):
    """The stand-alone walk (its own `main`, nothing loaded into Python) of csrc/bbd_bn_groups.h: accepted tables come back
    with the largest group and the launch fields filled, refused ones with 0, no read past a table, no write past a field."""
    exe = str(tmp_path / "bn_groups_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-static-libasan",
           "-static-libubsan", os.path.join(ROOT, "tests", "sanitize", "bn_groups_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    assert done.stdout.strip() == "bn call groups: ok"
