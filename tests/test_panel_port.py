"""CPU tier of the training-log panel: the host port of bbd_panel.hip (same bbd_panel_math.h / bbd_math.h /
bbd_viz_math.h) driven through `ops.train_panel` and `ops.argmin_hist`, against the fused path's own materialised
warps, the fixtures' arrays and the numpy restatement of tests/panel_ref.py.  Everything is bytes or integers: the
tolerance is equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panel_checks as pc  # noqa: E402
import panel_ref  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, ops  # noqa: E402
from baseboostdepth_amd._lib import ptr  # noqa: E402
from baseboostdepth_amd.plan import STEREO  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.fixture(scope="module")
def cases(port):
    """Every golden case once: (case, trainer, inputs, outputs, panel of its warps, jobs)."""
    out = {}
    for name in pc.WARP_CASES:
        case, tr, inputs, outputs = pc.run_case(name, port, "cpu")
        panel, jobs, rows = pc.render_case_warps(tr, inputs, outputs, port)
        out[name] = (case, tr, inputs, outputs, panel.numpy(), jobs)
    return out


def test_cases_cover_error_warps_row_offsets_and_stereo(cases):
    kinds = {name: {k for k, *_ in c[5]} for name, c in cases.items()}
    assert "E" in kinds["tri_7765_32x64"] and max(p for *_, p in cases["tri_7765_32x64"][5]) > 8
    assert {f for _, f, *_ in cases["tri_0000_16x32"][5]} == {STEREO}
    assert kinds["md2_b2_32x64"] == {"T"}


@pytest.mark.parametrize("name", pc.WARP_CASES)
def test_warp_tiles_equal_the_fused_paths_materialised_warps(cases, name):
    case, tr, inputs, outputs, panel, jobs = cases[name]
    H, W = case.H, case.W
    assert panel.shape == (-(-len(jobs) // pc.COLS) * H, pc.COLS * W, 3)
    for i, (kind, f, j, b, p) in enumerate(jobs):
        want = pc.quantised(outputs[("color" if kind == "T" else "color_D", f, 0)])[j]
        assert np.array_equal(panel_ref.cell(panel, i // pc.COLS, i % pc.COLS, H, W), want), (kind, f, j)
    for i in range(len(jobs), panel.shape[0] // H * pc.COLS):          # the last row's unused cells
        assert not panel_ref.cell(panel, i // pc.COLS, i % pc.COLS, H, W).any()


@pytest.mark.parametrize("name", pc.WARP_CASES)
def test_warp_tiles_equal_the_fixtures_warp_arrays(cases, name):
    case, tr, inputs, outputs, panel, jobs = cases[name]
    seen = 0
    for i, (kind, f, j, b, p) in enumerate(jobs):
        key = "out/%s/%s/0" % ("color" if kind == "T" else "color_D", f)
        if case.has(key):
            want = pc.quantised(case.expected(key))[j]
            assert np.array_equal(panel_ref.cell(panel, i // pc.COLS, i % pc.COLS, case.H, case.W), want), key
            seen += 1
    assert seen > 0 or not any(k.startswith("out/color") for k in case.z.files)


@pytest.mark.parametrize("name", pc.WARP_CASES)
def test_color_tile_returns_the_fixtures_bytes(port, cases, name):
    case = cases[name][0]
    frame = case.z["in/color/0/0"]
    assert frame.dtype == np.uint8
    tiles = [(0, b, "color", case.inputs[("color", 0, 0)][b]) for b in range(case.B)]
    panel, _ = ops.train_panel(tiles, None, case.H, case.W, 1, case.B, port)
    for b in range(case.B):
        assert np.array_equal(panel_ref.cell(panel.numpy(), 0, b, case.H, case.W), frame[b].transpose(1, 2, 0))


def test_color_rounds_to_nearest_and_clamps(port):
    values = [-0.5, 0.0, 127.5 / 255, 1.0, 1.5]
    img = torch.tensor(values, dtype=torch.float32).repeat(21).view(3, 5, 7)
    panel, _ = ops.train_panel([(0, 0, "color", img)], None, 5, 7, 1, 1, port)
    want = np.array([0, 0, 128, 255, 255], dtype=np.uint8)[np.arange(105) % 5].reshape(3, 5, 7).transpose(1, 2, 0)
    assert np.array_equal(panel.numpy(), want)
    assert np.array_equal(panel_ref.color_tile(img.numpy()), want)


@pytest.mark.parametrize("name,which", [(n, w) for n in pc.scalar_planes() for w in (("plasma", "magma") if n in pc.BOTH_LUTS
                                                                                      else ("plasma",))])
def test_scalar_tile_equals_numpy(port, name, which):
    plane = pc.scalar_planes()[name]
    plasma, magma, _ = pc.luts()
    lut = plasma if which == "plasma" else magma
    panel, stats = ops.train_panel([(0, 0, "scalar", torch.from_numpy(plane), which)], None, 5, 7, 1, 1, port)
    want, (lo, hi) = panel_ref.scalar_tile(plane, lut)
    assert np.array_equal(panel.numpy(), want)
    got = stats.numpy()[0]
    if name == "all_nan":
        assert np.isnan(got).all()
    else:
        assert got[0] == np.nanmin(plane) and got[1] == np.nanmax(plane) and (lo, hi) == (got[0], got[1])
    if name in ("constant", "all_nan"):
        assert (panel.numpy() == lut[0]).all()
    if name == "one_nan":
        assert (panel.numpy()[2, 3] == lut[0]).all()
    if name == "own_max":
        assert (panel.numpy()[4, 6] == lut[255]).all()


@pytest.mark.parametrize("n_t,n_e", [(6, 6), (2, 0)])
def test_argmin_tile(port, n_t, n_e):
    ids = pc.argmin_map()
    palette = pc.luts()[2]
    panel, _ = ops.train_panel([(0, 0, "argmin", torch.from_numpy(ids), n_t, n_e)], None, 5, 7, 1, 1, port)
    assert np.array_equal(panel.numpy(), panel_ref.argmin_tile(ids, palette, n_t, n_e))
    assert (panel.numpy()[ids >= n_t + n_e] == 0).all() and (panel.numpy()[ids == 0] == palette[0]).all()


@pytest.mark.parametrize("size", pc.GRID_SIZES)
def test_grid_placement_and_the_empty_cell(port, size):
    H, W = size
    d = pc.grid_inputs(H, W)
    panel, stats = pc.render_grid(H, W, port, "cpu")
    panel = panel.numpy()
    assert panel.shape == (3 * H, 2 * W, 3) and panel.dtype == np.uint8
    plasma, magma, palette = pc.luts()
    want = {(0, 0): panel_ref.color_tile(d["img"].numpy()), (0, 1): panel_ref.scalar_tile(d["plane_a"].numpy(), plasma)[0],
            (1, 0): panel_ref.argmin_tile(d["ids"].numpy(), palette, 5, 4),
            (1, 1): panel_ref.scalar_tile(d["plane_b"].numpy(), magma)[0]}
    # the warp has no numpy restatement at this size: the same tile alone in a 1 x 1 grid (its golden-case checks are above)
    alone, _ = ops.train_panel([(0, 0, "warp", d["src"], d["depth"], 1)], d["pose"], H, W, 1, 1, port)
    want[(2, 1)] = alone.numpy()
    assert alone.numpy().any()
    assert np.array_equal(panel, panel_ref.place(want, 3, 2, H, W))
    assert not panel_ref.cell(panel, 2, 0, H, W).any()
    assert stats.numpy()[1, 0] == d["plane_a"].min() and stats.numpy()[3, 1] == np.nanmax(d["plane_b"].numpy())


def test_identical_calls_give_identical_bytes(port):
    a, sa = pc.render_grid(17, 33, port, "cpu")
    b, sb = pc.render_grid(17, 33, port, "cpu")
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_pose_row_out_of_range_renders_black(port):
    d = pc.grid_inputs(5, 7)
    for p in (3, 1000, -1):
        panel, _ = ops.train_panel([(0, 0, "warp", d["src"], d["depth"], p)], d["pose"], 5, 7, 1, 1, port)
        assert not panel.numpy().any()


def test_argmin_hist_equals_bincount(port):
    a = pc.hist_input()
    counts = ops.argmin_hist(a, port)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (3, _lib.MAX_CAND)
    assert torch.equal(counts, pc.bincount(a))
    assert int(counts.sum()) == a.numel() - 3            # the ids 20 and 255 (twice) go uncounted


def test_bad_arguments_return_badarg_and_leave_the_output_untouched(port):
    H, W = 5, 7
    d = pc.grid_inputs(H, W)
    desc = torch.tensor([[_lib.PANEL_COLOR, 0] + list(ops._addr_words(d["img"])) + [0, 0, 0, 0]], dtype=torch.int32)
    lut = ops.panel_luts("cpu")
    out = torch.full((H, W, 3), 77, dtype=torch.uint8)
    stats = torch.zeros(1, 2)
    scratch = torch.zeros(port.lib.train_panel_scratch_ints(1), dtype=torch.int32)
    null = ctypes.c_void_p(0)
    good = [ptr(desc), ptr(d["pose"]), ptr(lut), ptr(out), ptr(stats), ptr(scratch), 1, 3, H, W, 1, 1]
    for i in range(6):                                   # every pointer NULL in turn
        args = list(good)
        args[i] = null
        assert port.status("bbd_train_panel", *args) == -1
    for i in range(6, 12):                               # every count / size 0 and negative in turn
        for bad in (0, -3):
            args = list(good)
            args[i] = bad
            assert port.status("bbd_train_panel", *args) == -1
    assert (out == 77).all()
    assert port.status("bbd_train_panel", *good) == 0 and not (out == 77).all()
    counts = torch.full((1, 20), 9, dtype=torch.int32)
    a = torch.zeros(1, 2, 2, dtype=torch.uint8)
    for args in ([null, ptr(counts), 1, 4], [ptr(a), null, 1, 4], [ptr(a), ptr(counts), 0, 4], [ptr(a), ptr(counts), 1, 0]):
        assert port.status("bbd_argmin_hist", *args) == -1
    assert (counts == 9).all()
    assert port.lib.train_panel_scratch_ints(0) == 0 and port.lib.train_panel_scratch_ints(-1) == 0


def test_lut_file_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    plasma, magma, palette = pc.luts()
    for name, got, n in (("plasma", plasma, 256), ("magma", magma, 256), ("tab20", palette, 20)):
        want = (matplotlib.colormaps[name](np.arange(n))[:, :3] * 255).astype(np.uint8)
        assert np.array_equal(got, want), name
    assert tuple(ops.panel_luts("cpu").shape) == (_lib.PANEL_LUT_ROWS, 3)
