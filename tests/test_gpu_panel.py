"""GPU tier of the training-log panel: bbd_panel.hip against its host port (same headers) byte for byte, against the
HIP path's own materialised warps, and `Trainer.log` after a graph-replayed pooled step against an eager per-signature
trainer that materialises its warps."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panel_checks as pc  # noqa: E402
import panel_ref  # noqa: E402
from test_gpu_trainer import _deterministic_convolutions, make_opt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.mark.parametrize("name", pc.WARP_CASES)
def test_warp_tiles_equal_the_host_port_and_the_materialised_warps(hip, port, name):
    case, tr, inputs, outputs = pc.run_case(name, hip, DEV)
    panel, jobs, rows = pc.render_case_warps(tr, inputs, outputs, hip)
    again, _, _ = pc.render_case_warps(tr, inputs, outputs, hip)
    assert torch.equal(panel, again)                                     # identical calls, identical bytes
    panel = panel.cpu().numpy()
    _, trp, inp, outp = pc.run_case(name, port, "cpu")
    want, _, _ = pc.render_case_warps(trp, inp, outp, port)
    assert np.array_equal(panel, want.numpy())
    for i, (kind, f, j, b, p) in enumerate(jobs):                        # the HIP path's own `warped_out`
        own = pc.quantised(outputs[("color" if kind == "T" else "color_D", f, 0)])[j]
        assert np.array_equal(panel_ref.cell(panel, i // pc.COLS, i % pc.COLS, case.H, case.W), own), (kind, f, j)


@pytest.mark.parametrize("size", pc.GRID_SIZES)
def test_mixed_grid_equals_the_host_port(hip, port, size):
    H, W = size
    got, stats = pc.render_grid(H, W, hip, DEV)
    again, stats2 = pc.render_grid(H, W, hip, DEV)
    want, wstats = pc.render_grid(H, W, port, "cpu")
    assert torch.equal(got, again) and torch.equal(stats, stats2)
    assert np.array_equal(got.cpu().numpy(), want.numpy())
    assert np.array_equal(stats.cpu().numpy(), wstats.numpy())
    assert not panel_ref.cell(got.cpu().numpy(), 2, 0, H, W).any()


def test_scalar_and_argmin_tiles_equal_the_host_port(hip, port):
    from baseboostdepth_amd import ops
    planes = pc.scalar_planes()
    ids = torch.from_numpy(pc.argmin_map())

    def render(backend, dev):
        tiles, r = [], 0
        for name, plane in planes.items():
            for c, which in enumerate(("plasma", "magma")):
                tiles.append((r, c, "scalar", torch.from_numpy(plane).to(dev), which))
            r += 1
        tiles += [(r, 0, "argmin", ids.to(dev), 6, 6), (r, 1, "argmin", ids.to(dev), 2, 0)]
        return ops.train_panel(tiles, None, 5, 7, r + 1, 2, backend)

    got, stats = render(hip, DEV)
    want, wstats = render(port, "cpu")
    assert np.array_equal(got.cpu().numpy(), want.numpy())
    assert np.array_equal(stats.cpu().numpy(), wstats.numpy(), equal_nan=True)


def test_pose_row_out_of_range_renders_black(hip):
    from baseboostdepth_amd import ops
    d = {k: v.to(DEV) for k, v in pc.grid_inputs(5, 7).items()}
    panel, _ = ops.train_panel([(0, 0, "warp", d["src"], d["depth"], 3), (0, 1, "warp", d["src"], d["depth"], -1)],
                               d["pose"], 5, 7, 1, 2, hip)
    assert not panel.cpu().numpy().any()


def test_argmin_hist_equals_bincount(hip):
    from baseboostdepth_amd import ops
    a = pc.hist_input()
    assert torch.equal(ops.argmin_hist(a.to(DEV), hip).cpu(), pc.bincount(a))
    big = torch.randint(0, 24, (2, 96, 161), generator=torch.Generator().manual_seed(2)).to(torch.uint8)   # several workgroups
    assert torch.equal(ops.argmin_hist(big.to(DEV), hip).cpu(), pc.bincount(big))


def test_log_after_a_graph_replay_equals_the_eager_per_signature_trainer(monkeypatch, tmp_path):
    """--rand --trimin --decomp --incremental_skip --partial_skip on a synthetic batch, scratch weights, fixed seed: after
    a graph-replayed step in pooled form `Trainer.log` draws the panel an eager per-signature trainer with materialised
    warps draws on the same weights and batch; its warp tiles are that trainer's quantised `("color", f, 0)`; the log
    leaves the captured graphs alone.  (96 x 160, batch 4: the smallest shapes the pooled GPU tests already run - the
    networks do not take 32 x 64, where the decoder's coarsest map is 1 x 2 and ReflectionPad2d(1) has nothing to mirror.)"""
    from PIL import Image
    from baseboostdepth_amd.synthetic import synthetic_batch
    from baseboostdepth_amd.trainer import Trainer
    _deterministic_convolutions(monkeypatch)
    H, W, ms, scales = 96, 160, [7, 5, 4, 3], [0]

    def batch():
        b = synthetic_batch(ms, H, W, scales, device=DEV, seed=3)
        b["cutt"] = torch.tensor(1.35)
        return b

    def trainer(graph):
        opt = make_opt(H, W, len(ms), [0, 1, 2, 3], True)
        opt.rand, opt.train_log, opt.log_samples = True, "panels", 2
        opt.log_dir = str(tmp_path / ("graph" if graph else "eager"))
        if graph:
            opt.step_graph = True
        else:
            opt.pooled_step, opt.step_graph, opt.materialize_warps = False, False, True
        torch.manual_seed(5)
        tr = Trainer(opt)
        tr.opt.scales = list(scales)
        tr.set_train()
        return tr

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trg, bg = trainer(True), batch()
        outg, lossg = trg.train_step(bg)
        assert trg.graph_stats["replays"] == 1 and ("bbd", "pose_matrices") in outg
        keys = list(trg._graphs)
        row = trg.log("train", bg, outg, lossg)
        panel_g = trg.render_panel("train", bg, outg)
        assert list(trg._graphs) == keys and len(keys) == 1 and trg.graph_stats["captures"] == 1
        tre, be = trainer(False), batch()
        oute, losse = tre.train_step(be)
        assert ("bbd", "pose_matrices") not in oute and ("color", 7, 0) in oute
        panel_e = tre.render_panel("train", be, oute)
    assert torch.equal(panel_g, panel_e)
    panel = panel_g.cpu().numpy()
    png = np.asarray(Image.open(os.path.join(trg.log_path, "train", "panels", "step_%08d.png" % trg.step)))
    assert np.array_equal(png, panel)
    assert abs(row["argmin/true_pose"] + row["argmin/error_induced"] + row["argmin/identity"] - 1.0) < 1e-12
    assert row["loss"] == float(lossg["loss"].detach())
    plan, r = tre.plan, 0
    for b in range(2):
        assert np.array_equal(panel_ref.cell(panel, r, 0, H, W), pc.quantised(be[("color", 0, 0)])[b])
        r += 1
        for kind, f in plan.cand_names[b]:
            if kind != "T":
                continue
            j = plan.jobs[f].index(b)
            assert np.array_equal(panel_ref.cell(panel, r, 1, H, W), pc.quantised(oute[("color", f, 0)])[j]), (b, f)
            if ("E", f) in plan.cand_names[b]:
                assert np.array_equal(panel_ref.cell(panel, r, 2, H, W), pc.quantised(oute[("color_D", f, 0)])[j]), (b, f)
            r += 1
    assert panel.shape == (r * H, 4 * W, 3)
