"""Shared pieces of the Velodyne depth-map tests (CPU tier through the host port, GPU tier through the HIP backend).

Fixture: tests/golden/velo_cases.npz, recorded from the reference's kitti_utils.generate_depth_map by
tools/make_golden_velo.py.  Acceptance rules, as the feature's issue sets them:
  vel_depth=True   the depth is the point's float32 x widened and cast back: maps equal the reference BIT FOR BIT
  vel_depth=False  the depth is q2 = P[2] . p in float64, whose last bits depend on the summation order (numpy hands the
                   product to BLAS): the set of non-zero pixels is identical and values are within 1 float32 ulp
The fixture tool asserts that no projected coordinate lies within 1e-6 of a half-integer, so the pixel a point lands on
does not depend on that order."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "velo_cases.npz")
CASES = ["scan_a", "scan_b", "crafted", "degenerate", "empty"]
CAMS = (2, 3)
DRIVES = {"2011_09_26": "2011_09_26/2011_09_26_drive_0001_sync", "2011_09_30": "2011_09_30/2011_09_30_drive_0020_sync"}


def load():
    return np.load(GOLDEN)


def size(v, case):
    return tuple(int(k) for k in v[case + "/size"])


def golden_map(v, case, cam, vel_depth):
    """The reference's float32 map, rebuilt from (gaps between non-zero pixels, values)."""
    h, w = size(v, case)
    flat = np.zeros(h * w, np.float32)
    key = "%s/cam%d/vd%d/" % (case, cam, int(vel_depth))
    flat[np.cumsum(v[key + "gaps"].astype(np.int64))] = v[key + "values"]
    return flat.reshape(h, w)


def scan(v, case):
    """float32 [N,4] as a KITTI .bin file holds it: xyz and a reflectance column the product must ignore."""
    pts = v[case + "/points"]
    return np.concatenate([pts, np.full((len(pts), 1), 0.37, np.float32)], 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_map(got, want, vel_depth, what=""):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    if vel_depth:
        assert np.array_equal(bits(got), bits(want)), "%s: %d pixels differ" % (what, int((bits(got) != bits(want)).sum()))
        return
    assert np.array_equal(got != 0, want != 0), "%s: non-zero sets differ" % what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    worst = float((err / ulp).max()) if err.size else 0.0
    print("%s: max error %.2f ulp, %d of %d non-zero pixels differ" % (what, worst, int((err > 0).sum()), int((want != 0).sum())))
    assert (err <= ulp).all(), what


def run_batch(v, members, vel_depth, backend, device, **kw):
    """`members` = [(case, cam), ...] through ONE `ops.velo_depth` call; returns the maps as numpy arrays."""
    from baseboostdepth_amd import ops
    scans = [scan(v, c) for c, _ in members]
    pts = torch.from_numpy(np.concatenate(scans)).to(device)
    shapes = [size(v, c) for c, _ in members]
    out, offsets = ops.velo_depth(pts, [len(s) for s in scans], np.stack([v["%s/P%d" % m] for m in members]), shapes,
                                  vel_depth=vel_depth, backend=backend, **kw)
    host = out.cpu().numpy()
    return [host[o:o + h * w].reshape(h, w) for o, (h, w) in zip(offsets, shapes)], out


def write_calibration(v, root, name):
    d = os.path.join(root, name)
    os.makedirs(d, exist_ok=True)
    for fname in ("cam_to_cam", "velo_to_cam"):
        with open(os.path.join(d, "calib_%s.txt" % fname), "w") as f:
            f.write(str(v["calib/%s/%s" % (name, fname)]))
    return d


def write_tree(v, root, frames):
    """A KITTI-raw-shaped tree: `frames` = [(date, frame index, float32 [N,4] scan)], calibration files per date and
    <date>/<drive>/velodyne_points/data/<index>.bin.  Returns the split lines ("folder index l")."""
    lines = []
    for date, t, pts in frames:
        write_calibration(v, root, date)
        d = os.path.join(root, DRIVES[date], "velodyne_points", "data")
        os.makedirs(d, exist_ok=True)
        np.ascontiguousarray(pts, np.float32).tofile(os.path.join(d, "%010d.bin" % t))
        lines.append("%s %d l" % (DRIVES[date], t))
    return lines


def write_split(splits_dir, split, lines):
    d = os.path.join(splits_dir, split)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "val_files.txt" if split == "eigen_zhou" else "test_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return d
