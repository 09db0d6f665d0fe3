"""CPU tier of the colour-mapped disparity: the host port of bbd_viz.hip (same bbd_viz_math.h) driven through
`ops.disp_viz`, against vectors captured from torch CPU + numpy + matplotlib (tools/make_golden_viz.py).
Acceptance rules: tests/viz_checks.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viz_checks  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import ops  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.fixture(scope="module")
def vectors():
    return np.load(viz_checks.GOLDEN)


def test_fixture_covers_the_required_regimes(vectors):
    small = big = up = down = same = 0
    for c in viz_checks.CASES:
        h, w = vectors[c + "/disp"].shape[2:]
        H0, W0 = (int(k) for k in vectors[c + "/size"])
        small += H0 + W0 <= 128
        big += H0 + W0 > 128
        up += H0 > h and W0 > w
        down += H0 < h and W0 < w
        same += (H0, W0) == (h, w)
    assert small and big and up and down and same
    assert vectors["constant/vmin"] == vectors["constant/vmax"]
    s = vectors["tied_max/s"]
    assert (s == s.max()).mean() > 0.05 and vectors["tied_max/vmax"] == s.max()


@pytest.mark.parametrize("name", viz_checks.CASES)
def test_host_port_matches_fixture(port, vectors, name):
    viz_checks.run_fixture_case(name, port, "cpu", vectors)


def test_constant_map_takes_entry_zero(port, vectors):
    col, _, st = viz_checks.run_fixture_case("constant", port, "cpu", vectors)
    lut = ops.magma_lut("cpu").numpy()
    assert st[0] == st[1] and (col == lut[0]).all()


def test_shipped_lut_equals_fixture_copy_and_matplotlib(vectors):
    lut = ops.magma_lut("cpu")
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
    assert np.array_equal(lut.numpy(), vectors["lut"])
    try:
        import matplotlib
    except ImportError:
        return
    want = (matplotlib.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    assert np.array_equal(lut.numpy(), want)


def test_product_does_not_import_matplotlib():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from baseboostdepth_amd import ops, inference; ops.magma_lut('cpu'); "
            "assert not any(m.split('.')[0] == 'matplotlib' for m in sys.modules), 'matplotlib imported'" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


def test_ragged_batch_equals_single_calls_and_float_switch(port, vectors):
    """Images of different original sizes in ONE call give the bits of one call each; want_float changes nothing."""
    names = ["big_up", "big_same"]                         # same network size 48 x 160
    disp = torch.from_numpy(np.concatenate([vectors[n + "/disp"] for n in names]))
    sizes = [tuple(int(k) for k in vectors[n + "/size"]) for n in names]
    col, fl, st = ops.disp_viz(disp, sizes, want_float=True, backend=port)
    col2, fl2, st2 = ops.disp_viz(disp, sizes, want_float=False, backend=port)
    assert fl2 is None and torch.equal(st, st2)
    for i, n in enumerate(names):
        one_c, one_f, one_s = ops.disp_viz(disp[i:i + 1], sizes[i:i + 1], want_float=True, backend=port)
        assert torch.equal(col[i], one_c[0]) and torch.equal(fl[i], one_f[0]) and torch.equal(st[i], one_s[0])
        assert torch.equal(col[i], col2[i])
        assert np.array_equal(fl[i].numpy(), vectors[n + "/s"])


@pytest.mark.parametrize("percentile,n", [(95.0, 20), (95.0, 21), (100.0, 37), (50.0, 2), (0.5, 1000), (95.0, 1)])
def test_percentile_rule_on_small_counts(port, percentile, n):
    """Virtual index, neighbours and float32 interpolation of np.percentile on counts where they are easy to see."""
    g = torch.Generator().manual_seed(n)
    disp = torch.rand(1, 1, 1, n, generator=g)
    _, fl, st = ops.disp_viz(disp, [(1, n)], percentile=percentile, want_float=True, backend=port)
    viz_checks.check_stats(fl[0].numpy(), st[0].numpy(), percentile)


def test_hip_backend_refuses_cpu_tensors():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    build()
    with pytest.raises(_lib.BbdError):
        ops.disp_viz(torch.rand(1, 1, 8, 8), [(16, 16)], backend=ops.HipBackend())
