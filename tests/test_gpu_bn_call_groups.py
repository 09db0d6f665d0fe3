"""GPU tier: the ten BatchNorm / stem entry points behind their one body per direction (csrc/bbd_nn.hip,
csrc/bbd_bn_groups.h).  Every bad description of the call groups is refused with BBD_E_BADARG before anything is launched,
and a host list and a device table of the same groups give the same bits in both launch forms and in the stem.
(`batch_norm_act` host list against device table is also compared by tests/test_gpu_pooled.py at 13 x 8 x 12 x 20, one-launch
form, and 40 x 64 x 48 x 160, two-launch form; the stem's two descriptions are compared with each other only here.)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOM, EPS = 0.1, 1e-5


def _rows(*sizes):
    arr = (ctypes.c_int32 * (len(sizes) + 1))()
    for i, n in enumerate(sizes):
        arr[i + 1] = arr[i] + n
    return arr


def _entry_points(N, C, H, W):
    """name -> (arguments up to `scratch`, arguments behind the group arguments) on valid buffers of an [N,C,H,W] batch."""
    from baseboostdepth_amd import ops
    from baseboostdepth_amd._lib import ptr
    MAXG = ops.BN_MAX_GROUPS
    f = lambda *s: torch.zeros(*s, device=DEV)
    OH, OW = (H - 1) // 2 + 1, W // 2
    t = dict(x=f(N, C, H, W), y=f(N, C, H, W), gy=f(N, C, H, W), gx=f(N, C, H, W), gres=f(N, C, H, W), res=f(N, C, H, W),
             w=torch.ones(C, device=DEV), b=f(C), gw=f(C), gb=f(C), mean=f(MAXG, C), invstd=torch.ones(MAXG, C, device=DEV),
             rm=f(C), rv=torch.ones(C, device=DEV), nbt=torch.zeros((), dtype=torch.int64, device=DEV),
             scratch=torch.zeros(MAXG * C * 64 * 2, dtype=torch.float64, device=DEV), pooled=f(N, C, OH, OW),
             gp=f(N, C, OH, OW), code=torch.zeros(N, C, OH, OW, dtype=torch.uint8, device=DEV))
    p = lambda *names: tuple(ptr(t[n]) for n in names)
    bn_fwd = (p("x", "res", "w", "b", "y", "mean", "invstd", "rm", "rv", "nbt", "scratch"), (N, C, H * W, EPS, MOM, 1))
    bn_bwd = (p("x", "y", "gy", "w", "b", "mean", "invstd", "gx", "gres", "gw", "gb", "scratch"), (N, C, H * W, 1))
    stem_fwd = (p("x", "w", "b", "y", "pooled", "code", "mean", "invstd", "rm", "rv", "nbt", "scratch"), (N, C, H, W, EPS, MOM))
    stem_bwd = (p("x", "gy", "gp", "code", "w", "b", "mean", "invstd", "gx", "gw", "gb", "scratch"), (N, C, H, W))
    return t, {"bbd_bn_act_grouped_fwd": bn_fwd, "bbd_bn_act_grouped_bwd": bn_bwd, "bbd_bn_act_grouped_dev_fwd": bn_fwd,
               "bbd_bn_act_grouped_dev_bwd": bn_bwd, "bbd_stem_fwd": stem_fwd, "bbd_stem_bwd": stem_bwd,
               "bbd_stem_dev_fwd": stem_fwd, "bbd_stem_dev_bwd": stem_bwd}


@pytest.mark.parametrize("stem,shape", [(False, (4, 2, 4, 8)), (True, (4, 2, 48, 96))], ids=["batch_norm", "stem"])
def test_entry_points_refuse_every_bad_description_of_the_call_groups(stem, shape):
    """One bad group argument at a time on otherwise valid calls (which are taken: each runs once first); the largest group
    of the good description is 2, at 48 x 96 the two-launch form the stem needs.  A refused call launches nothing: the
    outputs keep their zeros."""
    from baseboostdepth_amd import ops, _lib
    from baseboostdepth_amd._lib import ptr
    N, C, H, W = shape
    lib = ops.default_backend().lib
    t, entries = _entry_points(*shape)
    stream = lib.stream_for(t["x"])
    MAXG = ops.BN_MAX_GROUPS
    table = torch.full((MAXG + 2,), N, dtype=torch.int32)
    table[:3] = torch.tensor([0, 2, N])
    table[MAXG + 1] = 2
    table = table.to(DEV)
    null = ctypes.c_void_p(0)
    wide = _rows(*([1] * (MAXG + 1)))                       # (a table of 33 groups exists in full: only G is wrong)
    host_bad = {"G=0": (_rows(2, 2), 0, 0), "G=33": (wide, MAXG + 1, 0), "rows[G] != N": (_rows(2, 1), 2, 0),
                "a zero-row group": (_rows(2, 0, 2), 3, 0), "NULL table": (null, 2, 0), "untracked = G": (_rows(2, 2), 2, 2)}
    dev_bad = {"G=0": (ptr(table), 0, 2), "G=33": (ptr(table), MAXG + 1, 2), "bound 0": (ptr(table), 2, 0),
               "bound N+1": (ptr(table), 2, N + 1), "NULL table": (null, 2, 2)}
    entries = {k: v for k, v in entries.items() if ("stem" in k) == stem}
    refused = 0
    for name, (head, tail) in entries.items():
        device, forward = "_dev_" in name, name.endswith("_fwd")
        good = (ptr(table), 2, 2) if device else (_rows(2, 2), 2, 0)
        cut = 3 if device or forward else 2                 # the host backward has no `untracked_groups`
        lib.call(name, *head, *good[:cut], *tail, stream)
        for t_ in ("y", "pooled", "gx"):
            t[t_].zero_()
        for what, bad in (dev_bad if device else host_bad).items():
            if what == "untracked = G" and not forward:
                continue
            with pytest.raises(_lib.BbdError, match="status %d$" % _lib.E_BADARG):
                lib.call(name, *head, *bad[:cut], *tail, stream)
            refused += 1
    # the two entry points without group arguments are the single group [N]: a batch of no rows is a group of no rows
    if not stem:
        for name in ("bbd_bn_act_fwd", "bbd_bn_act_bwd"):
            head, tail = entries[name.replace("act_", "act_grouped_")]
            lib.call(name, *head, *tail, stream)
            for t_ in ("y", "gx"):
                t[t_].zero_()
            with pytest.raises(_lib.BbdError, match="status %d$" % _lib.E_BADARG):
                lib.call(name, *head, 0, *tail[1:], stream)
            refused += 1
    torch.cuda.synchronize()
    assert refused == 6 + 5 + 5 + 5 + (0 if stem else 2)
    assert not t["y"].any() and not t["pooled"].any() and not t["gx"].any()


def _run(op, shape, scope):
    from baseboostdepth_amd import ops
    N, C, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + H)
    x = torch.randn(shape, device=DEV, generator=gen).requires_grad_(True)
    w = (torch.rand(C, device=DEV, generator=gen) + 0.5).requires_grad_(True)
    b = torch.randn(C, device=DEV, generator=gen).requires_grad_(True)
    res = torch.randn(shape, device=DEV, generator=gen).requires_grad_(True)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    with scope():
        if op == "stem":
            outs = ops.stem_bn_relu_pool(x, w, b, rm, rv, MOM, EPS, num_batches_tracked=nbt)
        else:
            outs = (ops.batch_norm_act(x, w, b, res, rm, rv, MOM, EPS, True, num_batches_tracked=nbt),)
    grads = [torch.randn(o.shape, device=DEV, generator=gen) for o in outs]
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    got = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    got.update(running_mean=rm, running_var=rv, num_batches_tracked=nbt, grad_x=x.grad, grad_weight=w.grad, grad_bias=b.grad)
    if op != "stem":
        got["grad_residual"] = res.grad
    return got


@pytest.mark.parametrize("op,shape", [("batch_norm_act", (5, 3, 8, 8)), ("batch_norm_act", (5, 3, 48, 96)),
                                      ("stem", (5, 3, 48, 96))])
def test_a_host_list_and_a_device_table_of_the_same_groups_give_the_same_bits(op, shape):
    """Rows [2, 1, 2] with one padding group against a device table of the same rows, trailing empty groups, a grid of 8
    groups, 2 tracked, bound 2; 8 x 8 is the one-launch form (2 * 64 <= 8192), 48 x 96 the two-launch form (2 * 4608)."""
    from baseboostdepth_amd import ops
    N = shape[0]
    table = torch.full((ops.BN_MAX_GROUPS + 2,), N, dtype=torch.int32)
    table[:4] = torch.tensor([0, 2, 3, 5])
    table[ops.BN_MAX_GROUPS + 1] = 2
    table = table.to(DEV)
    host = _run(op, shape, lambda: ops.bn_call_groups([2, 1, 2], padding_groups=1))
    dev = _run(op, shape, lambda: ops.bn_call_groups_device(table, 8, 2))
    assert int(host["num_batches_tracked"]) == 2
    for name in host:
        assert torch.equal(host[name], dev[name]), name
