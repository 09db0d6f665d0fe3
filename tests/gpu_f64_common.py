"""What the GPU tiers that measure kernels against float64 references share (tests/test_gpu_vit_f64.py,
tests/test_gpu_nn_f64.py): the NaN-filled allocator blocks and the three-run check of one case."""
import torch

import vit_f64_ref as R

DEV = "cuda:0"


def poison(sizes):
    """NaN into allocator blocks of the given float counts, freed again: the next torch.empty of such a size gets one."""
    blocks = [torch.full((int(n),), float("nan"), device=DEV) for n in sizes if n > 0 for _ in range(3)]
    torch.cuda.synchronize()
    del blocks


def check(case, kernel, formula, leaves, consts, upstream, views, scratch=()):
    """`kernel` and `formula`: fn(*leaves, *consts) -> output(s).  `views`: (name, kind, pick) with pick(results) -> the tensor
    to measure, results = outputs followed by the gradients of the leaves.  Prints eager error, kernel error and their
    ratio for every tensor, then asserts.  Returns (kernel results, float64 results)."""
    ref = R.forward_backward(formula, leaves, consts, upstream, "cpu", torch.float64)
    with torch.backends.cudnn.flags(enabled=False):          # ATen's own depth-wise kernels: no solver search
        eager = R.forward_backward(formula, leaves, consts, upstream, DEV, torch.float32)
    got = R.forward_backward(kernel, leaves, consts, upstream, DEV, torch.float32)
    again = R.forward_backward(kernel, leaves, consts, upstream, DEV, torch.float32)
    poison(list(scratch) + [t.numel() for t in got if t is not None])
    third = R.forward_backward(kernel, leaves, consts, upstream, DEV, torch.float32)
    failures = []
    for name, kind, pick in views:
        g = pick(got)
        if not torch.equal(g, pick(again)):
            failures.append((name, "differs between two calls"))
        if not torch.equal(g, pick(third)):
            failures.append((name, "differs after NaN-filled blocks"))
        e_err, k_err = R.group_error(pick(eager), pick(ref), kind), R.group_error(g, pick(ref), kind)
        print("F64 | %s | %s | %.2e | %.2e | %.2f" % (case, name, e_err, k_err, k_err / max(e_err, 2.0 ** -24)))
        if not k_err <= R.bound(e_err):
            failures.append((name, "eager %.3e kernel %.3e bound %.3e" % (e_err, k_err, R.bound(e_err))))
    assert not failures, (case, failures)
    return got, ref
