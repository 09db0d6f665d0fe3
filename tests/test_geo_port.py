"""CPU tier of the geometry-consistency loss (`--geometry_consistency`): the host port of bbd_geo.hip (same
bbd_geo_math.h) through the `backend=` seam of `ops.geometry_consistency` against the float64 reference
(tests/geo_ref.py) on the cases of tests/geo_checks.py; the exact cases; the ValueErrors and the ABI's refusals;
`layers.GeometryConsistency`; the trainer's branch through the port; option parsing; and the port as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer.

Figures of the port against the reference (float32 against float64), printed by the tests:
  19 x 67   4 476 visible of 5 092, 0.54 % near a kink, loss 6.7e-8 relative, gradients 2.2e-6 (q_tgt), 7.8e-6 (q_src),
            3.5e-7 (T) of their maxima
  33 x 130  15 222 of 17 160, 0.75 %, loss 2.4e-7, gradients 6.6e-6, 1.5e-5, 5.7e-7"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geo_checks as gc  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import Trainer, _lib, layers, ops, synthetic  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402

# The trainer cases run at 64 x 128: at 32 x 64 the encoder's last map is 1 x 2 and torch refuses the depth decoder's
# reflection padding of a one-row map, so no trainer of the CPU tier can be built below this size.
H, W, B = 64, 128, 2


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.mark.parametrize("name", gc.STREETS)
def test_host_port_matches_the_reference(name):
    got = gc.port_result(name)
    assert gc.all_finite(got)
    gc.against_reference(name, got)


@pytest.mark.parametrize("name", [n for n in gc.CASES if n not in gc.STREETS])
def test_exact_and_edge_cases(name):
    gc.precondition(name, gc.port_result(name))


def test_identical_calls_give_identical_bytes(port):
    for name in ("street19", "spoilt"):
        assert gc.differing(gc.run(name, port, "cpu"), gc.port_result(name)) == []


def test_argument_errors_write_nothing(port):
    gc.bad_argument_sweep(port.status, "cpu")


def test_the_optional_outputs_are_optional_and_the_loss_is_the_mean(port):
    t = gc.tensors(gc.make("street19"), "cpu")
    res = ops.geometry_consistency(t["q_tgt"], t["q_src"], t["T"].reshape(2, 2, 3, 4), t["K"].reshape(2, 4, 4),
                                   t["inv_K"], backend=port)
    want = gc.port_result("street19")
    assert res.err is None and res.code is None and res._fields == ("loss", "pair_sum", "pair_count", "err", "code")
    assert res.pair_sum.dtype == torch.float64 and res.pair_count.dtype == torch.int64 and res.loss.dim() == 0
    assert gc.same_bytes(res.pair_sum.numpy(), want["pair_sum"]) and gc.same_bytes(res.loss.numpy(), want["loss"])
    assert float(res.loss) == float(want["pair_sum"].sum() / want["pair_count"].sum())
    assert _lib.ABI_VERSION >= 25 and _lib.GEO_MAX_VIEWS == 8 and _lib.GEO_RUN == 2048
    assert ops.geo_scratch_words(2, 33, 130, 2, False) == 2 * 3 * 2 * 2
    assert ops.geo_scratch_words(2, 33, 130, 2, True) == 2 * 2 * 33 * 130 + 2 * 3 * 2 * 12


def test_value_errors(port):
    t = gc.tensors(gc.make("street19"), "cpu")
    q, s, T, K, iK = t["q_tgt"], t["q_src"], t["T"], t["K"], t["inv_K"]
    port.calls.clear()
    for args, said in (
            ((q.double(), s, T, K, iK), "q_tgt must be float32"),
            ((q[0], s, T, K, iK), "q_tgt must be float32"),
            ((q[:0], s[:, :0], T[:, :0], K[:0], iK[:0]), "q_tgt must not be empty"),
            ((q, s.double(), T, K, iK), "q_src must be float32"),
            ((q, s[:, :1], T, K, iK), "q_src must be float32"),
            ((q, s[:0], T[:0], K, iK), "1 <= V <= 8"),
            ((q, s.repeat(5, 1, 1, 1), T.repeat(5, 1, 1), K, iK), "1 <= V <= 8"),
            ((q, s, T.double(), K, iK), "T must be float32"),
            ((q, s, T[:, :, :9], K, iK), "T must be float32"),
            ((q, s, T, K.double(), iK), "K must be float32"),
            ((q, s, T, K[:, :9], iK), "K must be float32"),
            ((q, s, T, K, iK[:1]), "inv_K must be float32"),
            ((q, s, T, K, iK.numpy()), "inv_K must be float32")):
        with pytest.raises(ValueError, match="geometry_consistency: .*" + said):
            ops.geometry_consistency(*args, backend=port)
    assert port.calls == []


def test_layer_scales_the_disparities_and_takes_whole_poses(port):
    case = gc.make("street19")
    t = gc.tensors(case, "cpu")
    lo, hi = 0.1, 100.0
    unscale = lambda q: (q - 1 / hi) / (1 / lo - 1 / hi)                  # noqa: E731
    disp = unscale(t["q_tgt"])[:, None].requires_grad_()
    sources = [unscale(t["q_src"][v])[:, None] for v in range(2)]
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(2, 1, 4)
    poses = [torch.cat([t["T"][v].reshape(2, 3, 4), bottom], 1) for v in range(2)]
    layer = layers.GeometryConsistency(lo, hi)
    res = layer(disp, sources, poses, t["K"].reshape(2, 4, 4), t["inv_K"].reshape(2, 4, 4), backend=port)
    q_tgt = layers.disp_to_depth(disp, lo, hi)[0][:, 0]
    q_src = torch.stack([layers.disp_to_depth(d, lo, hi)[0][:, 0] for d in sources])
    by_hand = ops.geometry_consistency(q_tgt, q_src, t["T"], t["K"], t["inv_K"], backend=port)
    assert gc.same_bytes(res.pair_sum.detach().numpy(), by_hand.pair_sum.detach().numpy()) and float(res.loss.detach()) > 0.01
    assert abs(float(res.loss.detach()) - float(gc.port_result("street19")["loss"])) < 1e-3     # the round trip moves q by ulps
    res.loss.backward()
    assert disp.grad is not None and float(disp.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="one pose per source"):
        layer(disp, sources, poses[:1], t["K"], t["inv_K"], backend=port)


# ---------------------------------------------------------------------------------------------- trainer and options
def _opts(extra=""):
    return MonodepthOptions().parse(("--no_cuda --weights_init scratch --height %d --width %d --batch_size %d %s"
                                     % (H, W, B, extra)).split())


def _step(extra):
    """One `process_batch` + backward through the port: (trainer, inputs, outputs, losses, parameter gradients)."""
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts(extra)
    tr = Trainer(opts, backend=PortBackend())
    tr.set_train()
    inputs = synthetic.synthetic_batch([1] * B, H, W, opts.scales, device="cpu", seed=5)
    outputs, losses = tr.process_batch(inputs)
    losses["loss"].backward()
    grads = {k: [None if p.grad is None else p.grad.clone() for p in m.parameters()] for k, m in tr.models.items()}
    return tr, inputs, outputs, losses, grads


@pytest.fixture(scope="module")
def steps():
    return {w: _step(extra) for w, extra in ((None, ""), (0.0, "--geometry_consistency 0"),
                                            (0.5, "--geometry_consistency 0.5"))}


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def test_weight_zero_is_the_step_without_the_option(steps):
    _, _, out0, los0, grads0 = steps[None]
    _, _, out1, los1, grads1 = steps[0.0]
    assert list(los0) == list(los1) and "loss/geometry" not in los1 and list(out0) == list(out1)
    assert all(gc.same_bytes(los0[k].detach().numpy(), los1[k].detach().numpy()) for k in los0)
    assert all(torch.equal(out0[k], out1[k]) for k in out0 if torch.is_tensor(out0[k]))
    assert all(_same(a, b) for k in grads0 for a, b in zip(grads0[k], grads1[k]))


def test_weighted_term_is_added_and_reaches_the_networks(steps, port):
    _, _, _, los0, grads0 = steps[0.0]
    tr, inputs, outputs, los, grads = steps[0.5]
    assert los["loss/geometry"].dtype == los["loss"].dtype and 0.0 < float(los["loss/geometry"]) < 1.0
    assert gc.same_bytes(los["loss"].detach().numpy(), (los0["loss"] + 0.5 * los["loss/geometry"]).detach().numpy())
    assert any(not _same(a, b) for a, b in zip(grads0["depth"], grads["depth"]))
    assert any(not _same(a, b) for a, b in zip(grads0["encoder"], grads["encoder"]))
    assert any(not _same(a, b) for a, b in zip(grads0["pose"], grads["pose"]))
    # the op by hand on the step's own tensors
    lo, hi = tr.opt.min_depth, tr.opt.max_depth
    scaled = lambda d: layers.disp_to_depth(d.detach(), lo, hi)[0][:, 0]      # noqa: E731
    q_src = torch.stack([scaled(outputs[("disp_source", f)]) for f in (-1, 1)])
    T = torch.stack([outputs[("cam_T_cam", 0, f)].detach()[:, :3] for f in (-1, 1)])
    by_hand = ops.geometry_consistency(scaled(outputs[("disp", 0)]), q_src, T, inputs[("K", 0)], inputs[("inv_K", 0)],
                                       backend=port)
    assert int(by_hand.pair_count.sum()) > H * W and torch.equal(by_hand.loss.to(los["loss"].dtype), los["loss/geometry"])


def test_the_scalar_reaches_the_training_log(port, tmp_path, capsys):
    import json
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts("--synthetic --log_dir %s --model_name t --num_epochs 1 --train_log text --log_frequency 1 "
                 "--geometry_consistency 0.5" % tmp_path)
    tr = Trainer(opts, backend=port)
    tr.num_total_steps = 2
    tr.run_epoch(synthetic.synthetic_loader(B, 2, H, W, opts.scales, device="cpu", seed=5, epoch=0))
    capsys.readouterr()
    rows = [json.loads(line) for line in open(os.path.join(tr.log_path, "train", "scalars.jsonl"))]
    assert len(rows) >= 1 and all(0.0 < r["loss/geometry"] < 1.0 and np.isfinite(r["loss"]) for r in rows)


def test_option_parsing_refuses_what_the_term_cannot_do(capsys):
    assert _opts().geometry_consistency == 0.0 and _opts("--geometry_consistency 0.25").geometry_consistency == 0.25
    assert _opts("--rand --geometry_consistency 0").rand
    for extra, said in (("--geometry_consistency 0.5 --rand", "--rand or --trimin"),
                        ("--geometry_consistency 0.5 --trimin", "--rand or --trimin"),
                        ("--geometry_consistency -0.1", "must not be negative"),
                        ("--geometry_consistency nan", "must not be negative")):
        with pytest.raises(SystemExit):
            _opts(extra)
        assert said in capsys.readouterr().err
    opts = _opts()
    opts.geometry_consistency, opts.trimin = 0.5, True                     # options set by hand are refused as loudly
    with pytest.raises(ValueError, match="--rand or --trimin"):
        Trainer(opts, backend=PortBackend())


# ---------------------------------------------------------------------------------------------- sanitizers
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "geo_port_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "geo_port_main.cpp"),
           os.path.join(ROOT, "tests", "host_port", "geo.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("name", ["street19", "spoilt"])
def test_port_runs_clean_under_the_sanitizers(program, tmp_path, name):
    """A stand-alone program with its own `main`; nothing sanitized is loaded into Python.  The -O1 sanitized build
    gives the bytes of the -O2 port."""
    case = gc.make(name)
    V, Bn, h, w = case["q_src"].shape
    with open(tmp_path / "case.bin", "wb") as f:
        f.write(np.array([Bn, h, w, V], "<i4").tobytes())
        for k in ("q_tgt", "q_src", "T", "K", "inv_K", "weights"):
            f.write(np.ascontiguousarray(case[k]).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], env=env, capture_output=True,
                          text=True, timeout=60)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    want = gc.port_result(name)
    blob = b"".join(np.ascontiguousarray(want[k]).tobytes() for k in gc.OUTPUTS if k != "loss")
    assert open(tmp_path / "out.bin", "rb").read() == blob
