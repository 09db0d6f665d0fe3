"""CPU tier of the semi-global stereo matcher and of `--depth_hints`: the host port of bbd_sgm.hip (same
bbd_sgm_math.h) through the `backend=` seam of `ops.stereo_hints` against the numpy reference (tests/sgm_ref.py) on the
cases of tests/sgm_checks.py, byte for byte; the planted-shift property of the reference; the mirror property; the
ValueErrors and the ABI's refusals; `ops.hint_depth`; `layers.DepthHints` against a plain-torch composition; the
trainer's branch through the port; option parsing; and the port as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer.  There are no real KITTI data here: every image is synthetic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sgm_checks as sc  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import Trainer, _lib, layers, ops, synthetic  # noqa: E402
from baseboostdepth_amd.options import MonodepthOptions  # noqa: E402
from oracle import hotpath_ref as O  # noqa: E402

# The trainer cases run at 64 x 128, the smallest size at which the depth decoder can be built (tests/test_geo_port.py).
H, W, B = 64, 128, 2


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def test_the_reference_recovers_a_planted_shift():
    """Random byte texture, the partner shifted by d0 = 11: on the interior (PLANTED_MARGIN = 8 pixels from the borders
    and from the zone x < d0) the numpy reference is valid everywhere and within 8/16 pixel of d0 - the parabola moves a
    true minimum by at most half a pixel.  Everything else is then held to byte equality with this reference."""
    disp, count = sc.reference("planted")
    inner = sc.planted_interior(disp)
    assert inner.size == 8 * 133
    assert (inner != -16).all()
    assert np.abs(inner.astype(np.int64) - 16 * sc.PLANTED_SHIFT).max() <= 8
    assert int(count[0]) == int((disp != -16).sum())


@pytest.mark.parametrize("name", list(sc.CASES))
def test_host_port_matches_the_reference(name):
    assert sc.same(sc.port_result(name), sc.reference(name))


def test_the_cases_reach_what_they_are_there_for():
    none, _ = sc.reference("none")
    assert (none == -16).all(2).any()                                   # a row with no valid pixel, fill on: stays invalid
    two, count = sc.reference("two")
    assert (two != -16).all() and 0 < int(count.min()) and int(count.max()) < two[0].size   # the fill filled, the count is pre-fill
    const, count = sc.reference("constant")
    assert (const == 0).all() and int(count[0]) == const.size          # all ties: the lowest d wins, unique, consistent
    for name in ("low", "lanes2", "mixed", "wide", "lanes3"):
        disp, count = sc.reference(name)
        filled = sc.CASES[name][6]
        assert 0 < int(count.min()) < disp[0].size and (disp == -16).any() != filled and (disp > 16).any(), name
    wide, _ = sc.reference("wide")
    assert wide.max() > 16 * 2 and (wide % 16 != 0).any()              # sub-pixel values occur


def test_mirrored_inputs_give_the_mirror_image(port):
    c = sc.make("two")
    flipped = dict(left=c["left"][..., ::-1].copy(), right=c["right"][..., ::-1].copy(), side=np.ones(2, np.int32))
    disp, count = sc.port_result("two")
    mirrored, mcount = sc.run("two", port, "cpu", **flipped)
    assert np.array_equal(mirrored, disp[..., ::-1]) and np.array_equal(count, mcount)
    # the mixed case holds the flags 0, 1, 1: images 0 and 2 were drawn apart, so only its own mirror is checked
    m = sc.make("mixed")
    back = dict(left=m["left"].copy(), right=m["right"].copy(), side=np.zeros(3, np.int32))
    back["left"][1:], back["right"][1:] = m["left"][1:, ..., ::-1], m["right"][1:, ..., ::-1]
    plain, _ = sc.run("mixed", port, "cpu", **back)
    mixed, _ = sc.port_result("mixed")
    assert np.array_equal(mixed[0], plain[0]) and np.array_equal(mixed[1:], plain[1:, ..., ::-1])


def test_identical_calls_give_identical_bytes_and_paths_and_fill_matter(port):
    assert sc.same(sc.run("lanes2", port, "cpu"), sc.port_result("lanes2"))
    assert not sc.same(sc.run("lanes2", port, "cpu", paths=8), sc.port_result("lanes2"))
    assert not sc.same(sc.run("lanes2", port, "cpu", fill=True), sc.port_result("lanes2"))
    assert not sc.same(sc.run("lanes2", port, "cpu", uniqueness=0), sc.port_result("lanes2"))


def test_scratch_formula_and_constants():
    from baseboostdepth_amd.csrc.build import build
    lib = _lib.HipLibrary(build())                                       # loading needs no GPU
    for shape in ((1, 5, 40, 64, 8), (3, 16, 33, 64, 4), (12, 192, 640, 128, 8), (1, 7, 301, 256, 8)):
        want = ops.sgm_scratch_bytes(*shape)
        assert want == lib.sgm_scratch_bytes(*shape) and want % 8 == 0
    assert ops.sgm_scratch_bytes(1, 1, 1, 64, 8) == 8 + 16 + 3 * 64 + 8
    assert lib.sgm_scratch_bytes(1, 5, 40, 96, 8) == 0 == lib.sgm_scratch_bytes(1, 5, 40, 64, 6)
    assert _lib.ABI_VERSION >= 27 and lib.abi_version == _lib.ABI_VERSION and "bbd_sgm_hints" in _lib.PROTOTYPES
    assert (_lib.SGM_P1, _lib.SGM_P2, _lib.SGM_UNIQUENESS, _lib.SGM_INVALID) == (10, 120, 5, -16)
    assert 8 * (62 + _lib.SGM_MAX_P2) <= 65535 < 8 * (62 + _lib.SGM_MAX_P2 + 1)     # the overflow bound is tight


def test_the_largest_penalty_cannot_wrap_the_sums(port):
    """P2 at its bound on a pair without any agreement: the reference adds in int64 and asserts S <= 65535."""
    got = sc.run("none", port, "cpu", uniqueness=0)
    c = sc.make("none")
    import sgm_ref
    for p1, p2 in ((_lib.SGM_MAX_P2 - 1, _lib.SGM_MAX_P2), (1, _lib.SGM_MAX_P2)):
        want = sgm_ref.stereo_hints(c["left"], c["right"], c["side"], 64, 8, p1, p2, 0, True)
        left, right, side = (torch.from_numpy(c[k]) for k in ("left", "right", "side"))
        disp, count = ops.stereo_hints(left, right, side, 64, 8, p1, p2, 0, True, backend=port)
        assert sc.same((disp.numpy(), count.numpy()), want)
    assert got[0].shape == (1, 6, 40)


def test_value_errors_and_refusals(port):
    c = sc.make("low")
    left, right, side = (torch.from_numpy(c[k]) for k in ("left", "right", "side"))
    port.calls.clear()
    for args, kw, said in (
            ((left.double(), right, side), {}, "left must be"),
            ((left[:, :2], right, side), {}, "left must be"),
            ((left[:0], right[:0], side[:0]), {}, "left must be"),
            ((left, right[..., :-1], side), {}, "right must be"),
            ((left, right.numpy(), side), {}, "right must be"),
            ((left, right, side.long()), {}, "side must be int32"),
            ((left, right, side.repeat(2)), {}, "side must be int32"),
            ((left, right, side, 96), {}, "disparities must be"),
            ((left, right, side, 320), {}, "disparities must be"),
            ((left, right, side, 64, 6), {}, "disparities must be"),
            ((left, right, side), dict(p1=0), "penalties"),
            ((left, right, side), dict(p1=120, p2=120), "penalties"),
            ((left, right, side), dict(p2=_lib.SGM_MAX_P2 + 1), "penalties"),
            ((left, right, side), dict(uniqueness=100), "uniqueness"),
            ((left, right, side), dict(uniqueness=-1), "uniqueness"),
            ((left, right, side, 64), dict(scratch=torch.empty(64, dtype=torch.uint8)), "scratch must be"),
            ((left, right, side, 64), dict(scratch=torch.empty(1 << 20, dtype=torch.float32)), "scratch must be")):
        with pytest.raises(ValueError, match="stereo_hints: .*" + said):
            ops.stereo_hints(*args, backend=port, **kw)
    assert port.calls == []
    from baseboostdepth_amd._lib import ptr
    disp = torch.full((1, 5, 40), 7, dtype=torch.int16)
    count = torch.full((1,), 7, dtype=torch.int64)
    scratch = torch.empty(ops.sgm_scratch_bytes(1, 5, 40, 64, 8), dtype=torch.uint8)
    good = [ptr(left), ptr(right), ptr(side), ptr(disp), ptr(count), ptr(scratch), scratch.numel(), 1, 5, 40, 64, 8, 10, 120,
            5, 0]
    for at, value in ((0, None), (3, None), (5, None), (6, scratch.numel() - 1), (7, 0), (8, 0), (10, 96), (10, 320), (11, 6),
                      (12, 0), (13, 10), (13, _lib.SGM_MAX_P2 + 1), (14, 100), (15, 2)):
        bad = list(good)
        bad[at] = value
        assert port.status("bbd_sgm_hints", *bad) == _lib.E_BADARG, (at, value)
    bad = list(good)
    bad[7] = 65536
    assert port.status("bbd_sgm_hints", *bad) == _lib.E_TOOMANY
    assert int(disp.min()) == 7 == int(disp.max()) and int(count[0]) == 7
    assert port.status("bbd_sgm_hints", *good) == 0 and int(count[0]) == int(sc.reference("low")[1][0])


def test_hint_depth_is_in_the_units_of_disp_to_depth():
    """A point at depth z of the network's units (baseline 0.1) has disparity fx * 0.1 / z pixels."""
    K = torch.tensor([[0.58 * 640, 0, 320, 0], [0, 1.92 * 192, 96, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(2, 1, 1)
    sT = torch.eye(4)[None].repeat(2, 1, 1)
    sT[0, 0, 3], sT[1, 0, 3] = -0.1, 0.1
    disp16 = torch.tensor([[[16, 40, -16, 0]], [[371, 16 * 255, 1, -16]]], dtype=torch.int16)
    depth, valid = ops.hint_depth(disp16, K, sT)
    assert depth.dtype == torch.float32 and valid.tolist() == [[[True, True, False, False]], [[True, True, True, False]]]
    fx = 0.58 * 640
    want = [[fx * 0.1 / 1.0, fx * 0.1 / 2.5, 0.0, 0.0], [fx * 0.1 * 16 / 371, fx * 0.1 / 255, fx * 0.1 * 16, 0.0]]
    assert torch.allclose(depth[:, 0], torch.tensor(want), rtol=1e-6, atol=0)
    assert torch.equal(ops.hint_depth(disp16, K.reshape(2, 16), sT)[0], depth)
    with pytest.raises(ValueError, match="int16"):
        ops.hint_depth(disp16.int(), K, sT)


# ---------------------------------------------------------------------------------------------- the layer
def _scene(seed=3):
    """A structured batch (a textured plane; the stereo partner a true shift of fx * 0.1 / depth pixels) on the host."""
    return synthetic.structured_batch([1] * B, H, W, (0, 1, 2, 3), device="cpu", seed=seed, trimin=False, decomp=False,
                                      incremental=False, partial=False, occluders=1)


def test_depth_hints_layer_against_a_plain_torch_composition(port):
    inputs = _scene()
    left, right = inputs[("color", 0, 0)], inputs[("color", "s", 0)]
    K, iK, sT = inputs[("K", 0)], inputs[("inv_K", 0)], inputs["stereo_T"]
    layer = layers.DepthHints(0.1, 100.0, 64)
    hint, valid, l_h = layer.hints(left, right, K, iK, sT, backend=port)
    # the matcher by hand: stereo_T[0,3] = +0.1, so the roles are mirrored (side 1)
    disp16, count = ops.stereo_hints(left, right, torch.ones(B, dtype=torch.int32), 64, backend=port)
    by_hand, by_hand_valid = ops.hint_depth(disp16, K, sT)
    assert torch.equal(hint, by_hand) and torch.equal(valid, by_hand_valid) and int(count.min()) > 0.5 * H * W
    px = round(float(K[0, 0, 0]) * 0.1 / synthetic._structured_depth())
    assert float((disp16[valid].float() / 16 - px).abs().median()) <= 0.5    # the plane's true disparity
    warped = O.warp(right, torch.where(valid, hint, torch.ones_like(hint))[:, None], K, iK, sT)
    want_lh = O.photometric_loss(warped, left)[:, 0]
    assert float((l_h - want_lh).abs().max()) < 1e-5
    # the term from the layer's own hint and l_h, written out
    gen = torch.Generator().manual_seed(1)
    disps = [torch.rand(B, 1, H >> s, W >> s, generator=gen).requires_grad_() for s in range(4)]
    best = [(l_h + 0.05 * torch.randn(B, H, W, generator=gen)).requires_grad_() for _ in range(4)]
    term, share = layer(left, right, K, iK, sT, disps, best, backend=port)
    want_term = want_share = 0.0
    for d, t in zip(disps, best):
        full = torch.nn.functional.interpolate(d.detach(), [H, W], mode="bilinear", align_corners=False)
        depth = 1 / (0.01 + (10 - 0.01) * full[:, 0])
        mask = (valid & (l_h < t.detach())).float()
        want_term += float((mask * torch.log(1 + (depth - hint).abs())).mean()) / 4
        want_share += float(mask.mean()) / 4
    assert 0.2 < want_share < 0.8 and abs(float(share) - want_share) < 1e-6
    assert abs(float(term.detach()) - want_term) <= 1e-5 * want_term
    term.backward()
    assert all(d.grad is not None and float(d.grad.abs().max()) > 0 for d in disps)
    assert all(t.grad is None for t in best) and not hint.requires_grad and not l_h.requires_grad and not share.requires_grad
    with pytest.raises(ValueError, match="one minimum-loss map per"):
        layer(left, right, K, iK, sT, disps, best[:2], backend=port)
    with pytest.raises(ValueError, match="stereo partner of every sample"):
        layer(left, right[:1], K, iK, sT, disps, best, backend=port)
    kept = layer._scratch
    layer(left, right, K, iK, sT, disps, best, backend=port)
    assert layer._scratch is kept                                        # allocated once


# ---------------------------------------------------------------------------------------------- trainer and options
def _opts(extra=""):
    return MonodepthOptions().parse(("--no_cuda --weights_init scratch --height %d --width %d --batch_size %d %s"
                                     % (H, W, B, extra)).split())


def _step(extra):
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts(extra)
    tr = Trainer(opts, backend=PortBackend())
    tr.set_train()
    outputs, losses = tr.process_batch(_scene(5))
    losses["loss"].backward()
    grads = {k: [None if p.grad is None else p.grad.clone() for p in m.parameters()] for k, m in tr.models.items()}
    return tr, outputs, losses, grads


@pytest.fixture(scope="module")
def steps():
    return {w: _step(extra) for w, extra in ((None, ""), (0.0, "--depth_hints 0"),
                                            (0.5, "--depth_hints 0.5 --hint_disparities 64"))}


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def test_weight_zero_is_the_step_without_the_option(steps):
    _, out0, los0, grads0 = steps[None]
    _, out1, los1, grads1 = steps[0.0]
    assert list(los0) == list(los1) and "loss/hints" not in los1 and "hint_share" not in los1 and list(out0) == list(out1)
    assert all(los0[k].detach().numpy().tobytes() == los1[k].detach().numpy().tobytes() for k in los0)
    assert all(torch.equal(out0[k], out1[k]) for k in out0 if torch.is_tensor(out0[k]))
    assert all(_same(a, b) for k in grads0 for a, b in zip(grads0[k], grads1[k]))


def test_weighted_term_is_added_and_reaches_the_depth_network_only(steps):
    _, _, los0, grads0 = steps[0.0]
    _, _, los, grads = steps[0.5]
    assert los["loss/hints"].dtype == los["loss"].dtype and float(los["loss/hints"]) > 0.0
    assert 0.0 < float(los["hint_share"]) <= 1.0 and not los["hint_share"].requires_grad
    assert torch.equal(los["loss"].detach(), (los0["loss"] + 0.5 * los["loss/hints"]).detach())
    assert float(los["loss"]) != float(los0["loss"])
    assert any(not _same(a, b) for a, b in zip(grads0["depth"], grads["depth"]))
    assert any(not _same(a, b) for a, b in zip(grads0["encoder"], grads["encoder"]))
    assert all(_same(a, b) for a, b in zip(grads0["pose"], grads["pose"]))            # the hint knows no pose


def test_hint_share_reaches_the_training_log(port, tmp_path, capsys):
    torch.manual_seed(0)
    torch.set_num_threads(4)
    opts = _opts("--synthetic --log_dir %s --model_name t --num_epochs 1 --train_log text --log_frequency 1 "
                 "--depth_hints 0.5 --hint_disparities 64" % tmp_path)
    tr = Trainer(opts, backend=port)
    tr.set_train()
    outputs, losses = tr.process_batch(_scene(5))
    tr.step, tr.epoch = 0, 0
    row = tr.log("train", _scene(5), outputs, losses)
    capsys.readouterr()
    rows = [json.loads(line) for line in open(os.path.join(tr.log_path, "train", "scalars.jsonl"))]
    assert row is not None and len(rows) == 1
    assert 0.0 < rows[0]["hint_share"] <= 1.0 and rows[0]["loss/hints"] > 0.0 and np.isfinite(rows[0]["loss"])


def test_option_parsing_refuses_what_the_term_cannot_do(capsys):
    assert _opts().depth_hints == 0.0 and _opts().hint_disparities == 128
    assert _opts("--depth_hints 0.25 --hint_disparities 256").depth_hints == 0.25
    assert _opts("--rand --depth_hints 0").rand
    for extra, said in (("--depth_hints 0.5 --rand", "--rand or --trimin"),
                        ("--depth_hints 0.5 --trimin", "--rand or --trimin"),
                        ("--depth_hints 0.5 --ViT", "--ViT"),
                        ("--depth_hints -0.1", "must not be negative"),
                        ("--depth_hints nan", "must not be negative"),
                        ("--depth_hints 0.5 --hint_disparities 100", "64, 128, 192 or 256")):
        with pytest.raises(SystemExit):
            _opts(extra)
        assert said in capsys.readouterr().err
    opts = _opts()
    opts.depth_hints, opts.trimin = 0.5, True                              # options set by hand are refused as loudly
    with pytest.raises(ValueError, match="--rand or --trimin"):
        Trainer(opts, backend=PortBackend())


# ---------------------------------------------------------------------------------------------- sanitizers
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "sgm_port_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "sgm_port_main.cpp"),
           os.path.join(ROOT, "tests", "host_port", "sgm.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("name", ["low", "two", "mixed", "lanes3", "none"])
def test_port_runs_clean_under_the_sanitizers(program, tmp_path, name):
    """A stand-alone program with its own `main`; nothing sanitized is loaded into Python.  The -O1 sanitized build
    gives the bytes of the -O2 port."""
    c = sc.make(name)
    Bn, _, h, w = c["left"].shape
    with open(tmp_path / "case.bin", "wb") as f:
        f.write(np.array([Bn, h, w, c["D"], c["paths"], 10, 120, c["uniqueness"], int(c["fill"])], "<i4").tobytes())
        for k in ("left", "right", "side"):
            f.write(np.ascontiguousarray(c[k]).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], env=env, capture_output=True,
                          text=True, timeout=60)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    want = sc.port_result(name)
    assert open(tmp_path / "out.bin", "rb").read() == want[0].tobytes() + want[1].tobytes()
