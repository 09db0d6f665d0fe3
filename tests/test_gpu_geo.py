"""GPU tier of the geometry-consistency loss (bbd_geo.hip through the C ABI): on every case of
tests/geo_checks.py the device equals the host port byte for byte in every output, forward and backward, and a second
identical call gives the same bytes; one full-size case (192 x 640: 60 work items a sample and the final reductions);
the ABI's refusals; and the trainer with `--geometry_consistency`: eager steps against step-graph replays, and weight 0
against a trainer built without the option.

No tolerance between device and port: the arithmetic has no transcendental function and is one IEEE operation where
written, the scattered sums are integers and every float64 sum has one written order."""
import gc as pygc
import os
import sys
import types
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geo_checks as gc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# The trainer cases run at 64 x 128, the size of the CPU tier's (tests/test_geo_port.py): below it the encoder's last
# map has one row, which the depth decoder's reflection padding does not take.
H, W, B = 64, 128, 2


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.mark.parametrize("name", gc.CASES + ("full",))
def test_device_matches_the_port(hip, name):
    got = gc.run(name, hip, DEV)
    assert gc.differing(got, gc.port_result(name)) == []                       # byte for byte the host port
    assert gc.differing(got, gc.run(name, hip, DEV)) == []                     # identical calls, identical bytes
    if name == "full":
        assert got["pair_count"].min() > 0.7 * 192 * 640 and abs(got["grad_T"]).max() > 0


def test_argument_errors_launch_nothing(hip):
    lib = hip.lib

    def status(name, *args):
        return getattr(lib._dll, name)(*args, None)

    gc.bad_argument_sweep(status, DEV)


def _train(weight, graph, monkeypatch, batches, seq):
    """The MD2 trainer of tests/test_gpu_trainer.py with deterministic convolution solvers (MIOpen's split-K weight
    gradients add with atomics), so that the bar is rounding and not solver noise.  Returns (parameters, the losses of every
    step, what the trainer says about its graphs).  The trainer, its captured graph and their memory are released HERE,
    behind a synchronisation, and not whenever the cyclic collector next runs: a step graph that dies in the middle of
    a later test's capture or replay is no state to leave behind."""
    from baseboostdepth_amd.trainer import Trainer
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    opt = types.SimpleNamespace(
        height=H, width=W, batch_size=B, scales=[0, 1, 2, 3], frame_ids=[0, -1, 1], min_depth=0.1, max_depth=100.0,
        disparity_smoothness=1e-3, no_ssim=False, trimin=False, decomp=False, pose_error=5.5, incremental_skip=False,
        partial_skip=False, materialize_warps=False, num_layers=18, weights_init="scratch", learning_rate=1e-4,
        no_cuda=False, cuda=0, load_weights_folder="None", log_dir="/tmp", model_name="t", step_graph=graph)
    if weight is not None:
        opt.geometry_consistency = weight
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
    params = torch.cat([p.detach().flatten() for p in tr.parameters_to_train]).clone()
    said = dict(use_graph=tr.use_graph, graphs=len(tr._graphs), step=tr.step, replays=tr.graph_stats["replays"])
    tr._graphs.clear()
    del tr, losses
    pygc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return params, record, said


@pytest.fixture(scope="module")
def batches():
    from baseboostdepth_amd.synthetic import synthetic_batch
    return [synthetic_batch([1] * B, H, W, [0, 1, 2, 3], device=DEV, seed=20 + i) for i in range(3)]


def test_step_graph_replays_match_eager_steps_with_the_term(monkeypatch, batches):
    """Set up like test_step_graph_replay_matches_eager: the same parameters and losses from three eager steps and from
    three replays of the captured step, with the geometry term inside the graph."""
    pe, le, _ = _train(0.5, False, monkeypatch, batches, [0, 1, 2])
    pg, lg, said = _train(0.5, True, monkeypatch, batches, [0, 1, 2])
    assert said == dict(use_graph=True, graphs=1, step=3, replays=3)
    for k in ("loss", "loss/geometry"):
        a, b = float(le[-1][k]), float(lg[-1][k])
        assert 0.0 < a and abs(a - b) <= 1e-5 * abs(a), (k, a, b)
    assert float((pe - pg).abs().max()) <= 1e-5 * float(pe.abs().max())


def test_weight_zero_leaves_the_existing_path_unchanged(monkeypatch, batches):
    _, plain, _ = _train(None, False, monkeypatch, batches, [0])
    _, zero, _ = _train(0.0, False, monkeypatch, batches, [0])
    _, half, _ = _train(0.5, False, monkeypatch, batches, [0])
    assert [list(r) for r in plain] == [list(r) for r in zero] and "loss/geometry" not in zero[0]
    assert all(torch.equal(a[k], b[k]) for a, b in zip(plain, zero) for k in a)
    # the first step's photometric part does not depend on the weight: the term is added to it
    assert torch.equal(half[0]["loss"], plain[0]["loss"] + 0.5 * half[0]["loss/geometry"])
