"""CPU tier of the checkpoint comparison sheets: the host port of bbd_compare.hip (same bbd_compare_math.h) driven
through `ops.gt_viz`, `ops.error_map`, `ops.disp_viz(raw=True)` and `compare.compare_batch`, against vectors captured
from the reference's own lines (tools/make_golden_compare.py) and a numpy restatement (tests/compare_ref.py).
Acceptance rules: tests/compare_checks.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compare_checks as C  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, evaluation, inference, ops  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.fixture(scope="module")
def vectors():
    return np.load(C.GOLDEN)


@pytest.fixture(scope="module")
def pred():
    return C.synth_pred(3, 6, 20)


def test_fixture_covers_the_required_regimes(vectors):
    sizes = {c: tuple(int(k) for k in vectors["disp/%s/size" % c]) for c in C.DISP_CASES}
    shapes = {c: vectors["disp/%s/disp" % c].shape[2:] for c in C.DISP_CASES}
    assert sum(sizes["up_small"]) <= 128 < sum(sizes["up_big"])
    assert sizes["same"] == tuple(shapes["same"]) and sizes["down"][0] < shapes["down"][0]
    assert vectors["disp/constant/vmin"] == vectors["disp/constant/vmax"]
    assert not vectors["gt/zero_32/gt"].any() and (vectors["gt/dense_31/gt"] != 0).all()
    assert vectors["gt/dense_31/vmin"] > 0
    assert (vectors["gt/cut/gt"][vectors["gt/cut/gt"] > 0] < 1 / 80).any() and vectors["gt/cut/vmax"] == 64.0
    assert {vectors["gt/%s/gt" % c].shape[1] for c in C.GT_CASES} >= {31, 32}
    share = np.mean(vectors["gt/sparse_31/gt"] != 0)
    assert 0.05 < share < 0.2
    for key in vectors.files:
        assert vectors[key].dtype != object and not (vectors[key].dtype.kind == "f" and np.isnan(vectors[key]).any())


@pytest.mark.parametrize("name", C.DISP_CASES)
def test_raw_disparity_picture_matches_fixture(port, vectors, name):
    C.check_disp_golden(name, port, "cpu", vectors)


def test_default_disp_viz_call_is_unchanged(port, vectors):
    disp = torch.from_numpy(vectors["disp/up_big/disp"])
    a = ops.disp_viz(disp, [(80, 250)], backend=port)
    b = ops.disp_viz(disp, [(80, 250)], 0.1, 80.0, 95.0, False, port, raw=False)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[2], b[2])
    raw = ops.disp_viz(disp, [(80, 250)], backend=port, raw=True)
    assert not torch.equal(raw[2], a[2])


def test_ground_truth_pictures_match_fixture(port, vectors):
    gts, pictures = C.check_gt_golden(port, "cpu", vectors)
    lut = ops.magma_lut("cpu").numpy()
    assert (C.np_(pictures[1]) == lut[0]).all() and tuple(lut[0]) == (0, 0, 3)          # the all-zero map
    one, stats = ops.gt_viz(gts, [4], backend=port)                                     # a batch that starts mid-buffer
    assert np.array_equal(C.np_(one[0]), vectors["gt/sparse_32/colour"])
    assert ops.viz_buffer(one).numel() == 3 * 16 * 32


def test_gt_viz_skips_nans_and_takes_entry_zero_for_them(port):
    gt = np.array([[2.0, np.nan, 4.0, 0.0, 8.0]], np.float32)
    gts = evaluation.GroundTruthSet([gt], "cpu")
    pictures, stats = ops.gt_viz(gts, [0], backend=port)
    assert stats[0, 0] == 0.0 and stats[0, 1] == 0.5
    lut = ops.magma_lut("cpu").numpy()
    assert tuple(C.np_(pictures[0])[0, 1]) == tuple(lut[0]) and tuple(C.np_(pictures[0])[0, 0]) == tuple(lut[255])


@pytest.mark.parametrize("name", C.FRAME_CASES)
def test_per_frame_abs_rel_matches_fixture(port, vectors, name):
    C.check_frame_golden(name, port, "cpu", vectors)


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("crop", [True, False])
def test_error_map_rules(port, pred, radius, crop):
    gt = C.rules_map()
    images = C.pictures_for([gt])
    rows, pictures, planes = C.check_error_maps_against_ref(port, "cpu", [gt], pred[:1], crop=crop, images=images,
                                                            radius=radius)
    plane, picture = planes[0], pictures[0]
    lut = ops.magma_lut("cpu").numpy()
    grey = (images[0].astype(np.int64).sum(-1) // 6).astype(np.uint8)
    assert np.isnan(plane[8, 20]) and np.isnan(plane[5, 25]) and np.isnan(plane[3, 3])
    assert np.isnan(plane[8, 0]) == crop and np.isnan(plane[0, 0]) == crop and np.isnan(plane[11, 39]) == crop
    if crop:                                     # (8, 0) is outside the window: it and its surroundings stay background
        assert (picture[7:10, 0:3] == grey[7:10, 0:3, None]).all()
    else:                                        # clipped neighbourhood of the map corner
        r = radius                               # (rows 0-1 only: (4, 1) reaches row 2 at radius 2)
        assert (picture[0:min(r, 1) + 1, 0:r + 1] == lut[compare_index(plane[0, 0])]).all()
        assert (picture[0, r + 1] == grey[0, r + 1]).all()
    assert plane[9, 30] >= 0.5 and tuple(picture[9, 30]) == tuple(lut[255])
    lo, hi = sorted((plane[7, 10], plane[7, 11]))
    assert lo != hi
    if radius >= 1:                              # both pixels see both errors: the maximum wins
        assert tuple(picture[7, 10]) == tuple(picture[7, 11]) == tuple(lut[compare_index(hi)])
    else:
        assert tuple(picture[7, 10]) == tuple(lut[compare_index(plane[7, 10])])
    assert int(rows[0, 10]) == int((~np.isnan(plane)).sum())


def compare_index(e, err_max=0.5):
    from compare_ref import lut_index_ref
    return int(lut_index_ref(np.float32(e), 0.0, err_max))


def test_error_map_without_picture_is_black_elsewhere(port, pred):
    gt = C.rules_map()
    rows, pictures, planes = C.check_error_maps_against_ref(port, "cpu", [gt], pred[:1], radius=0)
    assert (pictures[0][np.isnan(planes[0])] == 0).all()
    # count invariant: with radius 0 the coloured pixels are the scored ones (magma has no black entry)
    assert int((pictures[0].max(-1) > 0).sum()) == int((~np.isnan(planes[0])).sum()) == int(rows[0, 10])


def test_error_map_all_invalid_map_is_background(port, pred):
    gt = np.zeros((12, 40), np.float32)
    gt[0:3] = 90.0
    images = C.pictures_for([gt])
    rows, pictures, planes = C.check_error_maps_against_ref(port, "cpu", [gt], pred[:1], images=images)
    assert rows[0, 10] == 0 and np.isnan(planes[0]).all()
    assert np.array_equal(pictures[0][..., 0], (images[0].astype(np.int64).sum(-1) // 6).astype(np.uint8))


def test_error_map_without_median_scaling(port, pred):
    gt = C.rules_map()
    a = C.check_error_maps_against_ref(port, "cpu", [gt], pred[:1], median_scaling=False)
    b = C.check_error_maps_against_ref(port, "cpu", [gt], pred[:1], median_scaling=True)
    assert a[0][0, 7] == 1.0 and not np.array_equal(a[2][0], b[2][0], equal_nan=True)


@pytest.mark.parametrize("which", ["ragged", "aligned"])
def test_error_map_ragged_batch_invariants(port, pred, which):
    """Three maps at offsets 0, 15, 495 (byte stores) and one 8 x 32 map at offset 0 (packed stores), against the numpy
    restatement; the plane's count and mean are the metrics row's."""
    maps = C.ragged_maps() if which == "ragged" else C.aligned_map()
    images = C.pictures_for(maps)
    for radius in (0, 2):
        rows, pictures, planes = C.check_error_maps_against_ref(port, "cpu", maps, pred[:len(maps)], crop=False,
                                                                images=images, radius=radius)
    for i, plane in enumerate(planes):
        valid = plane[~np.isnan(plane)]
        assert valid.size == int(rows[i, 10]) > 0
        mean = np.float32(valid.astype(np.float64).sum() / valid.size)
        assert abs(mean - rows[i, 0]) <= np.spacing(np.float32(rows[i, 0])), (mean, rows[i, 0])


def test_gt_viz_ragged_batch_against_numpy(port):
    maps = C.ragged_maps() + C.aligned_map()
    gts = evaluation.GroundTruthSet(maps, "cpu")
    for idx in ([0, 1, 2, 3], [3], [1, 2]):
        pictures, stats = ops.gt_viz(gts, idx, backend=port)
        lut = ops.magma_lut("cpu").numpy()
        for k, i in enumerate(idx):
            with np.errstate(divide="ignore"):
                v = np.float32(1) / maps[i]
            v[v > 80] = 0
            from compare_ref import lut_index_ref
            assert stats[k, 0] == v.min() and stats[k, 1] == v.max()
            assert np.array_equal(C.np_(pictures[k]), lut[lut_index_ref(v, v.min(), v.max())])


def test_argument_errors(port):
    gt = C.rules_map()
    gts = evaluation.GroundTruthSet([gt], "cpu")
    pred = C.synth_pred(1, 6, 20)
    rows = evaluation.depth_metrics(pred, gts, [0], min_depth=0.1, pred_is_disp=True, median="numpy", backend=port)
    with pytest.raises(ValueError, match="radius"):
        ops.error_map(pred, gts, [0], rows, radius=5, backend=port)
    out = torch.zeros(3 * gt.size, dtype=torch.uint8)
    args = [_lib.ptr(pred), _lib.ptr(gts.buffer), _lib.ptr(gts.desc), _lib.ptr(rows), _lib.ptr(None),
            _lib.ptr(ops.magma_lut("cpu")), _lib.ptr(out), _lib.ptr(None)]
    assert port.status("bbd_error_map", *args, 1, 6, 20, 0.1, 80.0, 1.0, 0.5, 5, 0) == -1
    assert port.status("bbd_error_map", *args, 1, 6, 20, 0.1, 80.0, 1.0, 0.5, 2, 1) == -1      # PRED_IS_DISP is implied
    assert port.status("bbd_error_map", *args, 0, 6, 20, 0.1, 80.0, 1.0, 0.5, 2, 0) == -1
    assert port.status("bbd_error_map", *args, 1, 6, 20, 0.1, 80.0, 1.0, 0.5, 2, 0) == 0


# ---------------------------------------------------------------------------- compare_batch on the host
@pytest.mark.parametrize("error_maps", [False, True])
def test_compare_batch_on_the_host(port, error_maps):
    """Three models, two feed sizes (one `prepare` shared by the first and third), an odd count: one black cell."""
    predictors = C.tiny_predictors(port, [(32, 64), (24, 48), (32, 64)])
    C.check_compare_batch(predictors, port, "cpu", error_maps)


def test_error_background_follows_pictures_of_another_size(port):
    """Pictures that do not have their maps' sizes are brought there by the LANCZOS kernel before they are greyed."""
    from baseboostdepth_amd import compare, imageops
    images, maps = C.synth_frames()
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, (30, 100 + i, 3), dtype=np.uint8) for i in range(3)]
    gts = evaluation.GroundTruthSet(maps, "cpu")
    predictors = C.tiny_predictors(port, [(32, 64)])
    res = compare.compare_batch(images, gts, [0, 1, 2], predictors, cell=(24, 64), error_maps=True)
    pipe = imageops.ImagePipeline("cpu", port)
    for i, (gh, gw) in enumerate(C.FRAME_SIZES):
        assert tuple(res.disps[0][i].shape) == images[i].shape and tuple(res.errors[0][i].shape) == (gh, gw, 3)
        at_gt = pipe.resize(torch.from_numpy(images[i]).view(-1), [(0, 30, 100 + i, False)], gh, gw)
        pipe.flush()
        grey = (at_gt[0].numpy().astype(np.int64).sum(-1) // 6).astype(np.uint8)
        _, plane = ops.error_map(compare.disp_to_depth(predictors[0].disparity(predictors[0].prepare(images)), 0.1, 80.0)[0],
                                 gts, [0, 1, 2], res.rows[0], want_float=True, radius=2, backend=port)
        far = np.ones((gh, gw), bool)                       # pixels with no valid pixel within the radius
        ys, xs = np.nonzero(~np.isnan(plane[i].numpy()))
        for y, x in zip(ys, xs):
            far[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = False
        assert far.any() and (res.errors[0][i].numpy()[far] == grey[far][:, None]).all()
