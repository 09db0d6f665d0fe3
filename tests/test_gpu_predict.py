"""GPU tier of single-image prediction: bbd_disp_viz through `ops.disp_viz`, `DepthPredictor`, and the root
test_simple.py as a child process.  Acceptance rules: tests/viz_checks.py (s bit-equal to the fixture and within
rtol 3e-5 / atol 2e-6 of torch on this host's CPU; exact order statistics; vmax within 2 ulps of np.percentile; colours
equal to the LUT formula on the kernel's own numbers and within the capped one-step rule of the reference)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viz_checks  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# network size -> original size: KITTI, a full-HD photograph, and the high-resolution model on the other KITTI size
GEOMETRIES = [((192, 640), (375, 1242)), ((192, 640), (1080, 1920)), ((320, 1024), (370, 1226))]


def _close(got, want, rtol=3e-5):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=rtol, atol=2e-6)


def _synthetic_disp(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 1, h // 16 + 1, w // 16 + 1, generator=g)
    disp = torch.nn.functional.interpolate(low, (h, w), mode="bicubic", align_corners=True)
    return (disp + 0.02 * torch.rand(1, 1, h, w, generator=g)).clamp(0.0, 1.0).float().contiguous()


def _synthetic_image(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) % 256)], -1)
    return np.clip(base + rng.integers(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("name", viz_checks.CASES)
def test_fixture_cases_on_the_device(name):
    from baseboostdepth_amd import ops
    viz_checks.run_fixture_case(name, ops.default_backend(), DEV)


def test_live_reference_ragged_batch_and_single_calls():
    """Three geometries; the two that share a network size go through ONE ragged call, and every image alone gives
    the bits of the batched call."""
    from baseboostdepth_amd import ops
    lut = ops.magma_lut("cpu").numpy()
    by_net = {}
    for k, (net, orig) in enumerate(GEOMETRIES):
        by_net.setdefault(net, []).append((k, orig))
    assert max(len(v) for v in by_net.values()) >= 2
    for (h, w), members in by_net.items():
        disps = [_synthetic_disp(10 + k, h, w) for k, _ in members]
        sizes = [orig for _, orig in members]
        batch = torch.cat(disps).to(DEV)
        colour, floats, stats = ops.disp_viz(batch, sizes, want_float=True)
        colour_nf, none, stats_nf = ops.disp_viz(batch, sizes, want_float=False)
        assert none is None and torch.equal(stats, stats_nf)
        for i, (H0, W0) in enumerate(sizes):
            assert torch.equal(colour[i], colour_nf[i])                       # want_float changes no colour
            one_c, one_f, one_s = ops.disp_viz(batch[i:i + 1], [sizes[i]], want_float=True)
            assert torch.equal(one_c[0], colour[i]) and torch.equal(one_f[0], floats[i])
            assert torch.equal(one_s[0], stats[i])
            s, st, col = floats[i].cpu().numpy(), stats[i].cpu().numpy(), colour[i].cpu().numpy()
            ref_s, ref_vmin, ref_vmax, ref_col = viz_checks.live_reference(disps[i], H0, W0, lut)
            print("geometry %dx%d -> %dx%d: max |s - ref| %.3g" % (h, w, H0, W0, float(np.abs(s - ref_s).max())))
            _close(s, ref_s)
            viz_checks.check_stats(s, st)                                     # exact, on the kernel's own s
            _close([st[0], st[1]], [ref_vmin, ref_vmax])
            viz_checks.check_colours(col, s, st, lut, ref_col)


def test_three_geometries_in_one_call_when_the_network_size_is_shared():
    """All three original sizes ragged in ONE call (one network size), bit-identical to one call each."""
    from baseboostdepth_amd import ops
    sizes = [orig for _, orig in GEOMETRIES]
    batch = torch.cat([_synthetic_disp(20 + k, 192, 640) for k in range(3)]).to(DEV)
    colour, floats, stats = ops.disp_viz(batch, sizes, want_float=True)
    for i in range(3):
        one_c, one_f, one_s = ops.disp_viz(batch[i:i + 1], [sizes[i]], want_float=True)
        assert torch.equal(one_c[0], colour[i]) and torch.equal(one_f[0], floats[i]) and torch.equal(one_s[0], stats[i])
        viz_checks.check_stats(floats[i].cpu().numpy(), stats[i].cpu().numpy())


TINY_SIZES = [(1, 1), (3, 5), (5, 7), (12, 40)]


def test_tiny_ragged_batch_equals_the_host_port():
    """One call, an 8 x 8 network output for four images: one pixel; 15 and 35 pixels (fewer than a workgroup has
    threads, a last quad of three: byte stores); 480 pixels (two workgroups per histogram sweep, whole quads: packed
    stores).  Colours, floats and stats equal the host port's bit for bit."""
    from ports import PortBackend
    from baseboostdepth_amd import ops
    disp = torch.rand(4, 1, 8, 8, generator=torch.Generator().manual_seed(31))
    colour, floats, stats = ops.disp_viz(disp.to(DEV), TINY_SIZES, want_float=True)
    want_c, want_f, want_s = ops.disp_viz(disp, TINY_SIZES, want_float=True, backend=PortBackend())
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), want_s.numpy().view(np.uint32))
    for i, size in enumerate(TINY_SIZES):
        assert tuple(colour[i].shape) == size + (3,)
        assert np.array_equal(floats[i].cpu().numpy().view(np.uint32), want_f[i].numpy().view(np.uint32)), size
        assert np.array_equal(colour[i].cpu().numpy(), want_c[i].numpy()), size


def _random_predictor(H=64, W=128, **kw):
    from baseboostdepth_amd import networks
    from baseboostdepth_amd.inference import DepthPredictor
    torch.manual_seed(3)
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    return DepthPredictor(enc, dec, H, W, DEV, **kw)


def test_predictor_input_is_pillow_exact_and_colours_are_disp_viz():
    from PIL import Image
    from baseboostdepth_amd import ops
    pred = _random_predictor(64, 128, batch_size=1)                 # batch_size 1: two network batches
    images = [_synthetic_image(1, 75, 230), _synthetic_image(2, 120, 161)]
    x = pred.prepare(images)
    for i, im in enumerate(images):
        want = np.asarray(Image.fromarray(im).resize((128, 64), Image.LANCZOS), np.float32).transpose(2, 0, 1) / np.float32(255)
        assert np.array_equal(x[i].cpu().numpy(), want)
    results = pred.predict(images, want_float=True)
    disp = pred.last_disp                                           # the disparity those results were made from
    assert tuple(disp.shape) == (2, 1, 64, 128)
    colour, floats, stats = ops.disp_viz(disp, [(75, 230), (120, 161)], want_float=True)
    plain = pred.predict(images)
    plain_colour, _, _ = ops.disp_viz(pred.last_disp, [(75, 230), (120, 161)])
    for i, r in enumerate(results):
        assert r.color.shape == images[i].shape and r.color.dtype == np.uint8
        assert np.array_equal(r.color, colour[i].cpu().numpy())
        assert np.array_equal(plain[i].color, plain_colour[i].cpu().numpy())
        assert np.array_equal(r.scaled_disp, floats[i].cpu().numpy())
        assert np.array_equal(r.depth, np.float32(1) / r.scaled_disp)
        assert (r.vmin, r.vmax) == (float(stats[i, 0]), float(stats[i, 1]))
        assert plain[i].scaled_disp is None and plain[i].depth is None


def _saved_weights(tmp_path, H, W):
    from test_gpu_trainer import make_opt
    from baseboostdepth_amd.trainer import Trainer
    opt = make_opt(H, W, 2, [0, 1, 2, 3], False)
    opt.log_dir, opt.model_name = str(tmp_path), "m"
    tr = Trainer(opt)
    return tr, tr.save_model("w")


def test_from_weights_reads_the_stored_feed_size(tmp_path):
    from baseboostdepth_amd.inference import DepthPredictor
    tr, folder = _saved_weights(tmp_path, 96, 320)                   # not the default 192 x 640
    pred = DepthPredictor.from_weights(folder, device=DEV)
    assert (pred.feed_height, pred.feed_width) == (96, 320)
    for mine, theirs in ((pred.encoder, tr.models["encoder"]), (pred.decoder, tr.models["depth"])):
        saved = theirs.state_dict()
        own = mine.state_dict()
        assert own and all(torch.equal(v, saved[k]) for k, v in own.items())
    r = pred.predict([_synthetic_image(5, 100, 300)])[0]
    assert r.color.shape == (100, 300, 3) and r.vmin <= r.vmax


def test_command_line_as_a_child_process(tmp_path):
    from PIL import Image
    from baseboostdepth_amd.inference import DepthPredictor
    _, folder = _saved_weights(tmp_path, 64, 128)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    images = {"a": _synthetic_image(7, 90, 200), "b": _synthetic_image(8, 75, 230)}
    for name, im in images.items():
        Image.fromarray(im).save(src / (name + ".png"))
    single = tmp_path / "one.png"
    Image.fromarray(images["a"]).save(single)
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "test_simple.py"), "--weights", folder]
    r = subprocess.run(base + ["--image_path", str(src), "--save_path", str(dst), "--ext", "png", "--save_npy"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r1 = subprocess.run(base + ["--image_path", str(single), "--save_path", str(tmp_path / "unused")],
                        capture_output=True, text=True)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert sorted(os.listdir(dst)) == ["a_Base.jpg", "a_disp.npy", "b_Base.jpg", "b_disp.npy"]
    assert (tmp_path / "one_Base.jpg").is_file() and not (tmp_path / "unused").exists()
    pred = DepthPredictor.from_weights(folder, device=DEV)
    results = dict(zip(images, pred.predict(list(images.values()), want_float=True)))
    for name, im in images.items():
        got = np.asarray(Image.open(dst / (name + "_Base.jpg")))
        assert got.shape == im.shape
        again = tmp_path / (name + "_host.jpg")                      # JPEG is lossy: same array through Pillow here
        Image.fromarray(results[name].color).save(again)
        assert np.array_equal(got, np.asarray(Image.open(again)))
        mad = float(np.abs(got.astype(np.int32) - results[name].color.astype(np.int32)).mean())
        print("%s: mean |jpeg - colours| = %.3f" % (name, mad))
        # "small": Pillow's default JPEG (quality 75, 4:2:0 chroma) quantises luminance in steps of 5..60 and halves
        # the chroma resolution; on a textured colour image that is a few levels per channel.  3 % of the range
        # (8 of 255) separates that from a wrong picture (two unrelated magma images differ by ~80).
        assert mad < 8.0
        assert np.array_equal(np.load(dst / (name + "_disp.npy")), results[name].scaled_disp)
    alone = tmp_path / "alone_host.jpg"
    Image.fromarray(pred.predict([images["a"]])[0].color).save(alone)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "one_Base.jpg")), np.asarray(Image.open(alone)))
