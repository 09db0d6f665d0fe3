"""GPU tier of the semi-global stereo matcher and of `--depth_hints` (bbd_sgm.hip through the C ABI): on
every case of tests/sgm_checks.py the device equals the numpy reference and the host port byte for byte and a second
identical call gives the same bytes; the mirror property; a caller-owned scratch; the ABI's refusals; and one trainer
step with the term, eager against a replayed step graph.

No tolerance anywhere between device, port and reference: the matcher is integer arithmetic."""
import gc as pygc
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sgm_checks as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the smallest size the depth decoder builds (tests/test_gpu_geo.py)
H, W, B = 64, 128, 2


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.mark.parametrize("name", list(sc.CASES))
def test_device_matches_the_reference_and_the_port(hip, name):
    got = sc.run(name, hip, DEV)
    assert sc.same(got, sc.reference(name))                                   # byte for byte the numpy reference
    assert sc.same(got, sc.port_result(name))                                 # ... and the host port
    assert sc.same(got, sc.run(name, hip, DEV))                               # identical calls, identical bytes


def test_mirrored_inputs_give_the_mirror_image(hip):
    c = sc.make("two")
    flipped = dict(left=c["left"][..., ::-1].copy(), right=c["right"][..., ::-1].copy(), side=np.ones(2, np.int32))
    disp, count = sc.run("two", hip, DEV)
    mirrored, mcount = sc.run("two", hip, DEV, **flipped)
    assert np.array_equal(mirrored, disp[..., ::-1]) and np.array_equal(count, mcount)


def test_a_kept_scratch_with_stale_contents_changes_nothing(hip):
    from baseboostdepth_amd import ops
    c = sc.make("lanes2")
    left, right, side = (torch.from_numpy(c[k]).to(DEV) for k in ("left", "right", "side"))
    need = ops.sgm_scratch_bytes(*left.shape[:1], *left.shape[2:], c["D"], c["paths"])
    assert need == hip.lib.sgm_scratch_bytes(1, 9, 150, 128, 4)
    scratch = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    for _ in range(2):                                                        # the second call reads the first one's leftovers
        got = ops.stereo_hints(left, right, side, c["D"], c["paths"], uniqueness=c["uniqueness"], fill=c["fill"],
                               scratch=scratch, backend=hip)
        assert sc.same((got[0].cpu().numpy(), got[1].cpu().numpy()), sc.reference("lanes2"))
    assert int(scratch[need:].cpu().min()) == 0xA5                            # nothing is written past the formula
    with pytest.raises(ValueError, match="scratch must be"):
        ops.stereo_hints(left, right, side, c["D"], c["paths"], scratch=scratch[:need - 8], backend=hip)


def test_argument_errors_launch_nothing(hip):
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd._lib import ptr
    c = sc.make("low")
    left, right, side = (torch.from_numpy(c[k]).to(DEV) for k in ("left", "right", "side"))
    disp = torch.full((1, 5, 40), 7, dtype=torch.int16, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    scratch = torch.empty(hip.lib.sgm_scratch_bytes(1, 5, 40, 64, 8), dtype=torch.uint8, device=DEV)
    good = [ptr(left), ptr(right), ptr(side), ptr(disp), ptr(count), ptr(scratch), scratch.numel(), 1, 5, 40, 64, 8, 10, 120,
            5, 0]
    for at, value in ((0, None), (5, None), (6, scratch.numel() - 1), (7, 0), (10, 96), (10, 320), (11, 6), (12, 0),
                      (13, 10), (13, _lib.SGM_MAX_P2 + 1), (14, 100), (15, 2)):
        bad = list(good)
        bad[at] = value
        assert hip.lib._dll.bbd_sgm_hints(*bad, None) == _lib.E_BADARG, (at, value)
    bad = list(good)
    bad[7] = 65536
    assert hip.lib._dll.bbd_sgm_hints(*bad, None) == _lib.E_TOOMANY
    torch.cuda.synchronize()
    assert int(disp.cpu().min()) == 7 == int(disp.cpu().max()) and int(count.cpu()[0]) == 7


def _train(weight, graph, monkeypatch, batches, seq):
    """The MD2 trainer of tests/test_gpu_geo.py (deterministic convolution solvers) with `--depth_hints`.  Returns (the
    losses of every step, what the trainer says about its graphs).  The trainer, its captured graph and their memory are
    released HERE, behind a synchronisation."""
    from baseboostdepth_amd.trainer import Trainer
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    opt = types.SimpleNamespace(
        height=H, width=W, batch_size=B, scales=[0, 1, 2, 3], frame_ids=[0, -1, 1], min_depth=0.1, max_depth=100.0,
        disparity_smoothness=1e-3, no_ssim=False, trimin=False, decomp=False, pose_error=5.5, incremental_skip=False,
        partial_skip=False, materialize_warps=False, num_layers=18, weights_init="scratch", learning_rate=1e-4,
        no_cuda=False, cuda=0, load_weights_folder="None", log_dir="/tmp", model_name="t", step_graph=graph,
        depth_hints=weight, hint_disparities=64)
    torch.manual_seed(5)
    tr = Trainer(opt)
    tr.set_train()
    record = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in seq:
            _, losses = tr.train_step(dict(batches[i]))
            record.append({k: v.detach().clone() for k, v in losses.items()})
    torch.cuda.synchronize()
    said = dict(use_graph=tr.use_graph, graphs=len(tr._graphs), step=tr.step, replays=tr.graph_stats["replays"])
    tr._graphs.clear()
    del tr, losses
    pygc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return record, said


def test_a_step_with_hints_replays_as_a_graph_with_the_eager_losses(monkeypatch):
    from baseboostdepth_amd.synthetic import structured_batch
    # a textured plane whose stereo partner is a true shift of fx * 0.1 / depth pixels (tests/test_sgm_port.py)
    batches = [structured_batch([1] * B, H, W, (0, 1, 2, 3), device=DEV, seed=20 + i, trimin=False, decomp=False,
                                incremental=False, partial=False, occluders=1) for i in range(2)]
    eager, _ = _train(0.5, False, monkeypatch, batches, [0, 1])
    replay, said = _train(0.5, True, monkeypatch, batches, [0, 1])
    assert said == dict(use_graph=True, graphs=1, step=2, replays=2)
    assert 0.0 < float(eager[0]["hint_share"]) <= 1.0 and float(eager[0]["loss/hints"]) > 0.0
    assert 0.0 < float(replay[-1]["hint_share"]) <= 1.0
    for k in ("loss", "loss/hints"):
        a, b = float(eager[-1][k]), float(replay[-1][k])
        assert 0.0 < a and abs(a - b) <= 1e-5 * abs(a), (k, a, b)
