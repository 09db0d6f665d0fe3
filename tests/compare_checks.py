"""Acceptance rules of the comparison-sheet code, shared by the CPU tier (host port, tests/test_compare_port.py) and the
GPU tier (tests/test_gpu_compare.py): every function takes the backend and the device it runs on.

Exact equality is the bar against the goldens (tests/golden/compare_cases.npz, tools/make_golden_compare.py) and against
the numpy restatement (tests/compare_ref.py): the arithmetic is float32 with one rounding per operation on both sides.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compare_ref  # noqa: E402
from baseboostdepth_amd import compare, evaluation, imageops, inference, ops  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "compare_cases.npz")
DISP_CASES = ["up_small", "up_big", "same", "down", "constant"]
GT_CASES = ["sparse_31", "zero_32", "cut", "dense_31", "sparse_32"]
FRAME_CASES = ["frame_a", "frame_b"]
MIN_DEPTH, MAX_DEPTH = 0.1, 80.0


def np_(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------- goldens
def check_disp_golden(name, backend, device, vectors):
    disp = torch.from_numpy(vectors["disp/%s/disp" % name]).to(device)
    H0, W0 = (int(k) for k in vectors["disp/%s/size" % name])
    colour, _, stats = ops.disp_viz(disp, [(H0, W0)], raw=True, backend=backend)
    st = np_(stats)
    assert st[0, 0] == vectors["disp/%s/vmin" % name] and st[0, 1] == vectors["disp/%s/vmax" % name]
    assert np.array_equal(np_(colour[0]), vectors["disp/%s/colour" % name])


def check_gt_golden(backend, device, vectors, cases=GT_CASES):
    """All maps in ONE ragged batch: offsets 0, 620, 876, 1356 take the packed stores, 1635 the byte stores."""
    maps = [vectors["gt/%s/gt" % c] for c in cases]
    gts = evaluation.GroundTruthSet(maps, device)
    pictures, stats = ops.gt_viz(gts, list(range(len(cases))), backend=backend)
    st = np_(stats)
    for i, c in enumerate(cases):
        assert st[i, 0] == vectors["gt/%s/vmin" % c] and st[i, 1] == vectors["gt/%s/vmax" % c], c
        assert np.array_equal(np_(pictures[i]), vectors["gt/%s/colour" % c]), c
    return gts, pictures


def check_frame_golden(name, backend, device, vectors):
    """validation.py:232-269 for one frame.  count and ratio are exact (the same float32 operations); abs_rel is the
    reference's float32 pairwise mean of ~800 float32 values against a float64 sum rounded once: (log2(800) + 1) *
    2^-24 + 2^-24 < 1e-6 relative."""
    pred = torch.from_numpy(vectors["frame/%s/pred_disp" % name])[None].to(device)
    gts = evaluation.GroundTruthSet([vectors["frame/%s/gt" % name]], device)
    rows = np_(evaluation.depth_metrics(pred, gts, [0], min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_is_disp=True,
                                        median="numpy", backend=backend))
    want = float(vectors["frame/%s/abs_rel" % name])
    print(name, "abs_rel", rows[0, 0], want, "ratio", rows[0, 7], float(vectors["frame/%s/ratio" % name]))
    assert int(rows[0, 10]) == int(vectors["frame/%s/count" % name])
    assert rows[0, 7] == np.float32(vectors["frame/%s/ratio" % name])
    assert abs(float(rows[0, 0]) - want) <= 1e-6 * want


# ---------------------------------------------------------------------------- error map
def synth_pred(n, h, w, seed=5):
    """Scaled disparities [n,h,w] as disp_to_depth(sigmoid output, 0.1, 80) gives them."""
    gen = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 1, 3, 5, generator=gen)
    d = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=True)[:, 0]
    d = (0.05 + 0.5 * d + 0.02 * torch.rand(n, h, w, generator=gen)).clamp(0.001, 0.999)
    return (1.0 / MAX_DEPTH + (1.0 / MIN_DEPTH - 1.0 / MAX_DEPTH) * d).float().contiguous()


def rules_map():
    """12 x 40, Garg window rows 4-10, columns 1-37: one pixel per rule of include/bbd_hip.h."""
    gt = np.zeros((12, 40), np.float32)
    gt[8, 0] = 7.0                      # valid depth one column outside the crop window: must not colour
    gt[0, 0] = 9.0                      # map corners: the neighbourhood is clipped (scored only without the crop)
    gt[11, 39] = 11.0
    gt[4, 1] = 5.0                      # corner of the crop window
    gt[7, 10], gt[7, 11] = 6.0, 14.0    # two valid pixels in one neighbourhood: the larger error wins
    gt[9, 30] = 0.3                     # far off the prediction: error >= err_max, entry 255
    gt[8, 20] = 90.0                    # above max_depth: invalid
    gt[5, 25] = 0.05                    # below min_depth: invalid
    gt[10, 37] = 8.0                    # last row and column of the window
    gt[6, 18], gt[6, 33], gt[9, 5] = 12.0, 20.0, 4.0
    return gt


def run_error_maps(backend, device, maps, pred, crop=True, images=None, **kw):
    """(rows, pictures, planes) of `ops.error_map` over all maps as one batch, as numpy arrays."""
    gts = evaluation.GroundTruthSet(maps, device, crop=crop)
    idx = list(range(len(maps)))
    pred_d = pred.to(device)
    ms = kw.get("median_scaling", True)
    rows = evaluation.depth_metrics(pred_d, gts, idx, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_is_disp=True,
                                    median="numpy", median_scaling=ms, backend=backend)
    ims = None if images is None else [torch.from_numpy(im).to(device) for im in images]
    pictures, planes = ops.error_map(pred_d, gts, idx, rows, images=ims, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                                     want_float=True, backend=backend, **kw)
    return np_(rows), [np_(p) for p in pictures], [np_(p) for p in planes]


def check_error_maps_against_ref(backend, device, maps, pred, crop=True, images=None, radius=2, err_max=0.5,
                                 median_scaling=True):
    rows, pictures, planes = run_error_maps(backend, device, maps, pred, crop=crop, images=images, radius=radius,
                                            err_max=err_max, median_scaling=median_scaling)
    lut = ops.magma_lut("cpu").numpy()
    for i, gt in enumerate(maps):
        want_pic, want_plane = compare_ref.error_map_ref(
            pred[i].numpy(), gt, rows[i, 7], int(rows[i, 10]), lut, image=None if images is None else images[i],
            err_max=err_max, radius=radius, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, median_scaling=median_scaling,
            crop=crop)
        assert np.array_equal(planes[i].view(np.uint32), want_plane.view(np.uint32)), "float plane of map %d" % i
        assert np.array_equal(pictures[i], want_pic), "picture of map %d" % i
    return rows, pictures, planes


def ragged_maps(seed=11):
    """3 x 5 (fewer pixels than a workgroup has threads), 12 x 40 and 5 x 7: offsets 0, 15 and 495, so the second and
    third picture start off a 4-byte boundary (byte stores); dense enough that every map is scored."""
    rng = np.random.default_rng(seed)
    maps = []
    for gh, gw in ((3, 5), (12, 40), (5, 7)):
        gt = (2.0 + 60.0 * rng.random((gh, gw))).astype(np.float32)
        gt[rng.random((gh, gw)) < 0.6] = 0.0
        gt[gh // 2, gw // 2] = 10.0
        maps.append(gt)
    return maps


def aligned_map(seed=12):
    """One 8 x 32 map at offset 0: every quad is whole and aligned (packed stores only)."""
    rng = np.random.default_rng(seed)
    gt = (2.0 + 60.0 * rng.random((8, 32))).astype(np.float32)
    gt[rng.random((8, 32)) < 0.7] = 0.0
    return [gt]


def pictures_for(maps, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, m.shape + (3,), dtype=np.uint8) for m in maps]


# ---------------------------------------------------------------------------- compare_batch
FRAME_SIZES = [(47, 150), (48, 152), (47, 151)]


def synth_frames(seed=21):
    """Three frames of the sizes above and sparse ground truth at those sizes."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in FRAME_SIZES]
    maps = []
    for h, w in FRAME_SIZES:
        gt = (3.0 + 50.0 * rng.random((h, w))).astype(np.float32)
        gt[rng.random((h, w)) < 0.8] = 0.0
        maps.append(gt)
    return images, maps


def _resized(pipe, picture, ch, cw):
    """`ImagePipeline.resize` of one full-size picture (a device tensor [H,W,3]) to the cell size."""
    flat = picture.contiguous().view(-1)
    out = pipe.resize(flat, [(0, picture.shape[0], picture.shape[1], False)], ch, cw)
    pipe.flush()
    return out[0]


def check_compare_batch(predictors, backend, device, error_maps, cell=(24, 64)):
    images, maps = synth_frames()
    gts = evaluation.GroundTruthSet(maps, device)
    idx = [0, 1, 2]
    res = compare.compare_batch(images, gts, idx, predictors, cell=cell, error_maps=error_maps, backend=backend)
    M, n = len(predictors), len(images)
    ch, cw = cell
    R = compare.sheet_rows(M, error_maps)
    assert tuple(res.sheets.shape) == (n, R * ch, 2 * cw, 3) and res.sheets.dtype == torch.uint8
    assert tuple(res.rows.shape) == (M, n, 12)
    pipe = imageops.ImagePipeline(device, backend)
    named = compare.sheet_cells(M, error_maps)
    for i in range(n):
        full = {("image", None): torch.from_numpy(images[i]).to(device), ("gt", None): res.gt[i]}
        for m in range(M):
            full[("disp", m)] = res.disps[m][i]
            assert tuple(res.disps[m][i].shape) == FRAME_SIZES[i] + (3,)
            if error_maps:
                full[("error", m)] = res.errors[m][i]
        for row in range(R):
            for col in range(2):
                y0, y1, x0, x1 = compare.cell_rect(row, col, cell)
                got = res.sheets[i, y0:y1, x0:x1]
                if (row, col) in named:
                    assert torch.equal(got, _resized(pipe, full[named[(row, col)]], ch, cw)), (i, row, col)
                else:
                    assert int(got.max()) == 0, "an unused cell is black"
    if not error_maps and M % 2:
        assert (R - 1, 1) not in named
    for m, p in enumerate(predictors):                   # the metrics rows are a direct depth_metrics call's
        with torch.no_grad():
            disp = p.disparity(p.prepare(images))
        pred_disp, _ = compare.disp_to_depth(disp, MIN_DEPTH, MAX_DEPTH)
        rows = evaluation.depth_metrics(pred_disp, gts, idx, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_is_disp=True,
                                        median="numpy", backend=backend)
        assert torch.equal(res.rows[m], rows)
        assert float(rows[:, 10].min()) > 0
    host = res.host()
    assert np.array_equal(host.sheets, np_(res.sheets)) and np.array_equal(host.rows, np_(res.rows))
    for i in range(n):
        assert np.array_equal(host.gt[i], np_(res.gt[i]))
        for m in range(M):
            assert np.array_equal(host.disps[m][i], np_(res.disps[m][i]))
            if error_maps:
                assert np.array_equal(host.errors[m][i], np_(res.errors[m][i]))
    return res


# ---------------------------------------------------------------------------- tiny networks for the host tier
class TinyEncoder(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, 4, 3, padding=1)

    def forward(self, x):
        return [torch.tanh(self.conv(x))]


class TinyDecoder(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed + 100)
        self.conv = torch.nn.Conv2d(4, 1, 3, padding=1)

    def forward(self, feats):
        return {("disp", 0): torch.sigmoid(2.0 * self.conv(feats[0]))}


def tiny_predictors(port, feeds):
    return [inference.DepthPredictor(TinyEncoder(k), TinyDecoder(k), h, w, "cpu", backend=port)
            for k, (h, w) in enumerate(feeds)]


# ---------------------------------------------------------------------------- a KITTI-shaped tree
def write_tree(root, images, maps, ext="png"):
    """kt_path and split_dir of a synthetic tree holding `images` as frames 0 .. n-1 of one drive, with gt_depths.npz."""
    from PIL import Image
    kt, split = os.path.join(root, "kitti"), os.path.join(root, "split")
    folder = "2011_09_26/2011_09_26_drive_0001_sync"
    os.makedirs(os.path.join(kt, folder, "image_02", "data"))
    os.makedirs(split)
    lines = []
    for i, im in enumerate(images):
        Image.fromarray(im).save(os.path.join(kt, folder, "image_02", "data", "%010d.%s" % (i, ext)))
        lines.append("%s %d l" % (folder, i))
    with open(os.path.join(split, "val_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    data = np.empty(len(maps), dtype=object)
    for i, m in enumerate(maps):
        data[i] = m
    np.savez_compressed(os.path.join(split, "gt_depths.npz"), data=data)
    return kt, split


def read_csv(path):
    with open(path) as f:
        lines = [line.rstrip("\n").split(",") for line in f]
    return lines[0], lines[1:-1], lines[-1]
