"""GPU tier of the checkpoint comparison sheets: bbd_compare.hip against the goldens and, byte for byte, against its host
port; `compare.compare_batch` end to end with two random-weight ResNet-18 checkpoints; validation.py as a child process.
Acceptance rules: tests/compare_checks.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compare_checks as C  # noqa: E402
from baseboostdepth_amd import compare, evaluation, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEED = (96, 160)                     # the smallest feed size the decoder accepts


@pytest.fixture(scope="module")
def backend():
    return ops.default_backend()


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.fixture(scope="module")
def vectors():
    return np.load(C.GOLDEN)


@pytest.fixture(scope="module")
def pred():
    return C.synth_pred(3, 6, 20)


@pytest.mark.parametrize("name", C.DISP_CASES)
def test_raw_disparity_picture_matches_fixture(backend, vectors, name):
    C.check_disp_golden(name, backend, DEV, vectors)


def test_ground_truth_pictures_match_fixture(backend, vectors):
    C.check_gt_golden(backend, DEV, vectors)


@pytest.mark.parametrize("name", C.FRAME_CASES)
def test_per_frame_abs_rel_matches_fixture(backend, vectors, name):
    C.check_frame_golden(name, backend, DEV, vectors)


def test_gt_viz_equals_the_host_port_on_ragged_batches(backend, port):
    maps = C.ragged_maps() + C.aligned_map()
    dev_set, host_set = evaluation.GroundTruthSet(maps, DEV), evaluation.GroundTruthSet(maps, "cpu")
    for idx in ([0, 1, 2, 3], [3], [1, 2]):
        got, got_stats = ops.gt_viz(dev_set, idx, backend=backend)
        want, want_stats = ops.gt_viz(host_set, idx, backend=port)
        assert np.array_equal(C.np_(got_stats).view(np.uint32), C.np_(want_stats).view(np.uint32))
        for g, w in zip(got, want):
            assert np.array_equal(C.np_(g), C.np_(w))


@pytest.mark.parametrize("which", ["ragged", "aligned", "rules"])
@pytest.mark.parametrize("radius", [0, 2, 4])
def test_error_map_equals_the_host_port(backend, port, pred, which, radius):
    maps = {"ragged": C.ragged_maps, "aligned": C.aligned_map, "rules": lambda: [C.rules_map()]}[which]()
    images = C.pictures_for(maps)
    crop = which == "rules"
    for ims, scaling in ((images, True), (None, False)):
        kw = dict(crop=crop, images=ims, radius=radius, median_scaling=scaling)
        rows_d, pics_d, planes_d = C.run_error_maps(backend, DEV, maps, pred[:len(maps)], **kw)
        rows_h, pics_h, planes_h = C.run_error_maps(port, "cpu", maps, pred[:len(maps)], **kw)
        assert np.array_equal(rows_d[:, 7:11].view(np.uint32), rows_h[:, 7:11].view(np.uint32))      # ratio, medians, count
        for i in range(len(maps)):
            assert np.array_equal(planes_d[i].view(np.uint32), planes_h[i].view(np.uint32)), i
            assert np.array_equal(pics_d[i], pics_h[i]), i


def test_error_map_all_invalid_map_is_background(backend, pred):
    gt = np.zeros((12, 40), np.float32)
    images = C.pictures_for([gt])
    rows, pictures, planes = C.check_error_maps_against_ref(backend, DEV, [gt], pred[:1], images=images)
    assert rows[0, 10] == 0 and np.isnan(planes[0]).all()


def _checkpoint(folder, seed):
    """A random-weight ResNet-18 checkpoint as the trainer saves it: encoder.pth carries the feed size."""
    from baseboostdepth_amd import networks
    torch.manual_seed(seed)
    encoder = networks.ResnetEncoder(18, False)
    decoder = networks.DepthDecoder(encoder.num_ch_enc)
    os.makedirs(folder)
    state = encoder.state_dict()
    state["height"], state["width"] = FEED
    torch.save(state, os.path.join(folder, "encoder.pth"))
    torch.save(decoder.state_dict(), os.path.join(folder, "depth.pth"))
    return folder


@pytest.fixture(scope="module")
def models_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("models")
    for k, name in enumerate(("first", "second", "third")):
        _checkpoint(str(root / name), 40 + k)
    return str(root)


@pytest.fixture(scope="module")
def predictors(models_dir):
    from baseboostdepth_amd.inference import DepthPredictor
    return [DepthPredictor.from_weights(os.path.join(models_dir, n), device=DEV) for n in ("first", "second", "third")]


@pytest.mark.parametrize("n_models,error_maps", [(2, False), (3, False), (2, True)])
def test_compare_batch_end_to_end(backend, predictors, n_models, error_maps):
    assert (predictors[0].feed_height, predictors[0].feed_width) == FEED
    C.check_compare_batch(predictors[:n_models], backend, DEV, error_maps)


def test_validation_py_as_a_child_process(tmp_path, models_dir, predictors):
    from PIL import Image
    images, maps = C.synth_frames()
    kt, split = C.write_tree(str(tmp_path), images, maps)
    out = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "validation.py"), "--model_name", "first", "second", "--models_dir",
           models_dir, "--kt_path", kt, "--split_dir", split, "--output", out, "--ext", "png", "--format", "png",
           "--cell_size", "64", "24", "--no_labels", "--error_maps"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    gts = evaluation.GroundTruthSet(maps, DEV)
    res = compare.compare_batch(images, gts, [0, 1, 2], predictors[:2], cell=(24, 64), error_maps=True).host()

    def png(*parts):
        return np.asarray(Image.open(os.path.join(out, *parts)))

    for i in range(3):
        name = "%010d.png" % i
        assert np.array_equal(png("sheets", name), res.sheets[i])
        assert np.array_equal(png("depth", name), res.gt[i])
        for m, model in enumerate(("first", "second")):
            assert np.array_equal(png(model, name), res.disps[m][i])
            assert np.array_equal(png("errors", model, name), res.errors[m][i])
    header, body, mean = C.read_csv(os.path.join(out, "abs_rel.csv"))
    assert header == ["index", "frame", "first", "second"] and len(body) == 3
    values = np.array([[float(v) for v in row[2:]] for row in body])
    assert [row[2:] for row in body] == [["%.6f" % v for v in res.rows[:, i, 0]] for i in range(3)]
    # every printed value is rounded to 6 decimals (5e-7 each): the mean of the rows and the printed mean differ by 1e-6 at most
    assert mean[0] == "mean" and np.allclose([float(v) for v in mean[2:]], values.mean(0), rtol=0, atol=1.01e-6)
    assert "scaling ratio" in r.stdout
