#!/usr/bin/env python3
"""Golden vectors for the Velodyne depth maps, recorded from the reference's own `kitti_utils.generate_depth_map`
(imported unmodified from the reference tree; `np.int`, which it still uses, is put back for this process only).
Output: tests/golden/velo_cases.npz - data only: calibration file texts, point clouds (float32 xyz), the projection
matrices and image sizes the reference computes, and its depth maps cast to float32 as its export casts them, for
cameras 2 and 3 with vel_depth on and off.  Maps are stored as (gaps between non-zero pixels, values); tests/velo_checks.py
rebuilds them.

    python tools/make_golden_velo.py

Cases
  scan_a, scan_b  synthetic 64-beam scans (ground plane + obstacles, ranges on a 1/512 m grid like the sensor's 2 mm)
                  on two calibrations with different image sizes (375 x 1242, 370 x 1226): a ragged batch.  Azimuth is
                  restricted to the camera's field of view and points that project more than 40 px outside the image of
                  camera 2 are dropped, to keep the file small.
  crafted         points placed on chosen pixels by inverting P of camera 2: the (r, w-1) / (r+1, 0) key collision with
                  the first point on either side, triple hits, x < 0, x = -0.0, NaN / inf coordinates, points one pixel
                  outside each border
  degenerate      an axis-aligned calibration with exactly representable entries, so that q2 == 0 (inf) and
                  q0 == q2 == 0 (NaN) are hit exactly
  empty           no points

The assertions keep the reference alone inside the conditions the tests state: enough points and duplicate keys, each
collision order present, and every q0/q2, q1/q2 more than 1e-6 away from a half-integer, so that any sane float64
summation order picks the same pixel.
"""
import os
import sys
import tempfile
from collections import Counter

import numpy as np

np.int = int          # removed in numpy 1.24; kitti_utils.py:86 uses it
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

sys.path.insert(0, refshim.REFERENCE_ROOT)
import kitti_utils as ref  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "velo_cases.npz")

CALIB = {
    "2011_09_26": (
        "calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n"
        "S_rect_02: 1.242000e+03 3.750000e+02\n"
        "R_rect_00: 9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01\n"
        "P_rect_02: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03\n"
        "P_rect_03: 7.215377e+02 0.000000e+00 6.095593e+02 -3.395242e+02 0.000000e+00 7.215377e+02 1.728540e+02 2.199936e+00 0.000000e+00 0.000000e+00 1.000000e+00 2.729905e-03\n",
        "calib_time: 15-Mar-2012 11:37:16\n"
        "R: 7.533745e-03 -9.999714e-01 -6.166020e-04 1.480249e-02 7.280733e-04 -9.998902e-01 9.998621e-01 7.523790e-03 1.480755e-02\n"
        "T: -4.069766e-03 -7.631618e-02 -2.717806e-01\n"),
    "2011_09_30": (
        "calib_time: 09-Jan-2012 14:00:15\ncorner_dist: 9.950000e-02\n"
        "S_rect_02: 1.226000e+03 3.700000e+02\n"
        "R_rect_00: 9.999280e-01 8.085985e-03 -8.866797e-03 -8.123205e-03 9.999583e-01 -4.169750e-03 8.832711e-03 4.241477e-03 9.999520e-01\n"
        "P_rect_02: 7.070912e+02 0.000000e+00 6.018873e+02 4.688783e+01 0.000000e+00 7.070912e+02 1.831104e+02 1.178601e-01 0.000000e+00 0.000000e+00 1.000000e+00 6.203223e-03\n"
        "P_rect_03: 7.070912e+02 0.000000e+00 6.018873e+02 -3.334597e+02 0.000000e+00 7.070912e+02 1.831104e+02 1.930130e+00 0.000000e+00 0.000000e+00 1.000000e+00 3.318498e-03\n",
        "calib_time: 25-May-2012 16:47:16\n"
        "R: 7.027555e-03 -9.999753e-01 2.599616e-05 -2.254837e-03 -4.184312e-05 -9.999975e-01 9.999728e-01 7.027479e-03 -2.255075e-03\n"
        "T: -7.137748e-03 -7.482656e-02 -3.336324e-01\n"),
    "axis_aligned": (
        "calib_time: none\n"
        "S_rect_02: 1.242000e+03 3.750000e+02\n"
        "R_rect_00: 1 0 0 0 1 0 0 0 1\n"
        "P_rect_02: 700 0 600 0 0 700 180 0 0 0 1 0\n"
        "P_rect_03: 700 0 600 -350 0 700 180 0 0 0 1 0\n",
        "calib_time: none\n"
        "R: 0 -1 0 0 0 -1 1 0 0\n"
        "T: 0 0 -0.25\n"),
}


def write_calib(root, name):
    d = os.path.join(root, name)
    os.makedirs(d, exist_ok=True)
    for fname, text in zip(("calib_cam_to_cam.txt", "calib_velo_to_cam.txt"), CALIB[name]):
        with open(os.path.join(d, fname), "w") as f:
            f.write(text)
    return d


class DotSpy:
    """Stands in for the reference module's `np` while it runs: numpy itself, with the results of np.dot kept.  The
    second product of generate_depth_map is its projection matrix (kitti_utils.py:62), which it does not return."""

    def __init__(self):
        self.dots = []

    def __getattr__(self, name):
        return getattr(np, name)

    def dot(self, a, b):
        self.dots.append(np.dot(a, b))
        return self.dots[-1]


def run_reference(calib_dir, scan, cam, vel_depth):
    """(float32 depth map, P) of the reference for one frame."""
    spy = DotSpy()
    ref.np = spy
    try:
        with np.errstate(all="ignore"):
            depth = ref.generate_depth_map(calib_dir, scan, cam, vel_depth)
    finally:
        ref.np = np
    assert len(spy.dots) == 3 and spy.dots[1].shape == (3, 4) and spy.dots[1].dtype == np.float64
    return depth.astype(np.float32), spy.dots[1]


def project(P, pts):
    """u, v, valid for points float32 [N,3] in one explicit float64 order (the tool's own check, not a golden)."""
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        q = p[:, 0:1] * P[None, :, 0] + p[:, 1:2] * P[None, :, 1] + p[:, 2:3] * P[None, :, 2] + P[None, :, 3]
        a, b = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    return a, b, q[:, 2]


def landing(P, pts, h, w):
    a, b, _ = project(P, pts)
    with np.errstate(all="ignore"):
        u, v = np.round(a) - 1, np.round(b) - 1
        ok = (pts[:, 0] >= 0) & (u >= 0) & (v >= 0) & (u < w) & (v < h)
    return u, v, ok


def assert_clear_of_half_integers(P, pts, name):
    a, b, _ = project(P, pts)
    keep = (pts[:, 0] >= 0) & np.isfinite(a) & np.isfinite(b) & (np.abs(a) < 1e7) & (np.abs(b) < 1e7)
    for t in (a[keep], b[keep]):
        dist = np.abs(t - np.floor(t) - 0.5)
        assert dist.size == 0 or dist.min() > 1e-6, (name, float(dist.min()))


def synthetic_scan(rng, n, P2, P3, h, w):
    """64 beams between -24.8 and +2 degrees, azimuth inside +-43 degrees; ground plane 1.73 m below the sensor and
    obstacles at random ranges; points far outside camera 2's image are dropped."""
    az = rng.uniform(-np.deg2rad(43), np.deg2rad(43), n)
    el = np.deg2rad(rng.integers(0, 64, n) * (26.8 / 63) - 24.8)
    ground = 1.73 / np.maximum(np.sin(-el), 1e-3)
    r = np.round(np.minimum(ground, rng.uniform(4, 80, n)) * 512) / 512
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1)
    pts = (np.round(pts * 512) / 512).astype(np.float32)
    a, b, _ = project(P2, pts)
    keep = (a > -40) & (a < w + 40) & (b > -40) & (b < h + 40)
    for P in (P2, P3):           # a handful of points sit on a rounding boundary of one camera: not part of the fixture
        for t in project(P, pts)[:2]:
            keep &= np.abs(t - np.floor(t) - 0.5) > 1e-5
    return pts[keep]


def crafted_cloud(P, h, w):
    def at(u, v, zc):                       # the point camera 2 sees at pixel (u, v) with depth zc
        return np.linalg.solve(P[:, :3], zc * np.array([u + 1.0, v + 1.0, 1.0]) - P[:, 3])

    def at_x0(u, v):                        # a point with x == 0 that lands on (u, v): solve for y, z and the depth
        A = np.stack([P[:, 1], P[:, 2], -np.array([u + 1.0, v + 1.0, 1.0])], 1)
        y, z, _ = np.linalg.solve(A, -P[:, 3])
        return np.array([-0.0, y, z])

    pix = [(w - 1, 200, 30.0), (0, 201, 12.0), (0, 201, 9.0), (w - 1, 200, 31.0),      # first on the (r, w-1) side
           (0, 101, 15.0), (w - 1, 100, 7.0), (w - 1, 100, 22.0), (0, 101, 11.0),      # first on the (r+1, 0) side
           (w - 1, 250, 8.0), (0, 251, 20.0),      # one point each: the first keeps its own minimum
           (0, 261, 6.0), (w - 1, 260, 25.0),
           (0, 271, 19.0), (w - 1, 270, 5.0),      # the first takes the OTHER pixel's smaller depth
           (w - 1, 281, 40.0), (0, 282, 3.0),
           (5, 5, 10.0), (5, 5, 7.0), (5, 5, 9.0),                                     # triple hits
           (700, 300, 12.0), (700, 300, 18.0), (700, 300, 15.0),
           (600, 180, -5.0), (610, 180, -0.5),                                         # behind the sensor: x < 0
           (-1, 100, 10.0), (w, 100, 10.0), (300, -1, 10.0), (300, h, 10.0),           # one pixel outside each border
           (0, 0, 10.0), (w - 1, h - 1, 10.0), (0, h - 1, 10.0), (w - 1, 0, 10.0)]     # the four corners
    pts = [at(*p) for p in pix]
    pts.insert(10, at_x0(400, 150))
    pts.append(at_x0(800, 200))
    pts += [np.array(p) for p in ([np.nan, 1.0, 1.0], [5.0, np.nan, 0.0], [5.0, 1.0, np.nan], [np.inf, 0.0, 0.0],
                                  [5.0, np.inf, 0.0], [5.0, 1.0, -np.inf], [3e38, 1.0, 1.0], [0.0, 0.0, 0.0],
                                  [-3.0, 1.0, 0.5])]
    return np.array(pts, np.float32)


def degenerate_cloud():
    # axis_aligned: q0 = -700 y + 600 (x - 0.25), q1 = -700 z + 180 (x - 0.25), q2 = x - 0.25
    return np.array([[0.25, 1.0, 0.0],      # q2 == 0, q0 < 0  -> -inf
                     [0.25, -1.0, -1.0],    # q2 == 0, q0 > 0  -> +inf
                     [0.25, 0.0, 0.0],      # 0 / 0            -> NaN
                     [10.25, 1.0, 0.5], [10.25, 1.0, 0.5], [20.25, -3.25, 1.0], [0.125, 0.025, 0.0125],   # q2 < 0, lands
                     [0.0, 0.1, 0.05], [-0.0, 0.1, 0.05]], np.float32)


def sparse(depth32):
    nz = np.flatnonzero(depth32.view(np.uint32))          # (-0.0 counts: bit patterns are recorded)
    return np.diff(nz, prepend=0).astype(np.int32), depth32.ravel()[nz]


def main():
    out = {}
    rng = np.random.default_rng(2025)
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {name: write_calib(tmp, name) for name in CALIB}
        for name, (c2c, v2c) in CALIB.items():
            out["calib/%s/cam_to_cam" % name] = np.array(c2c)
            out["calib/%s/velo_to_cam" % name] = np.array(v2c)
        nothing = os.path.join(tmp, "nothing.bin")
        np.zeros((0, 4), np.float32).tofile(nothing)
        geo = {}
        for name, d in dirs.items():
            for cam in (2, 3):
                depth, P = run_reference(d, nothing, cam, True)
                geo.setdefault(name, {})[cam] = (P, depth.shape)
        P26, (h26, w26) = geo["2011_09_26"][2]
        P30, (h30, w30) = geo["2011_09_30"][2]
        assert (h26, w26, h30, w30) == (375, 1242, 370, 1226)
        clouds = [("scan_a", "2011_09_26", synthetic_scan(rng, 40000, P26, geo["2011_09_26"][3][0], h26, w26)),
                  ("scan_b", "2011_09_30", synthetic_scan(rng, 40000, P30, geo["2011_09_30"][3][0], h30, w30)),
                  ("crafted", "2011_09_26", crafted_cloud(P26, h26, w26)),
                  ("degenerate", "axis_aligned", degenerate_cloud()),
                  ("empty", "2011_09_30", np.zeros((0, 3), np.float32))]
        for case, calib, pts in clouds:
            out[case + "/calib"] = np.array(calib)
            out[case + "/points"] = pts
            scan = os.path.join(tmp, case + ".bin")
            np.concatenate([pts, np.full((len(pts), 1), 0.5, np.float32)], 1).tofile(scan)
            for cam in (2, 3):
                P, (h, w) = geo[calib][cam]
                out["%s/P%d" % (case, cam)] = P
                out[case + "/size"] = np.array([h, w], np.int32)
                assert_clear_of_half_integers(P, pts, case)
                u, v, ok = landing(P, pts, h, w)
                keys = Counter((v[ok] * (w - 1) + u[ok] - 1).tolist())
                dupes = sum(1 for c in keys.values() if c > 1)
                if case.startswith("scan"):
                    assert ok.sum() >= 20000 and dupes >= 500, (case, cam, int(ok.sum()), dupes)
                if case == "crafted" and cam == 2:
                    ui, vi = u[ok].astype(int), v[ok].astype(int)
                    k = vi * (w - 1) + ui - 1
                    first_right = first_left = 0
                    for key in set(k.tolist()):
                        members = np.flatnonzero(k == key)
                        if len(set(zip(vi[members], ui[members]))) == 2:
                            first_right += ui[members[0]] == w - 1
                            first_left += ui[members[0]] == 0
                    assert first_right >= 1 and first_left >= 1, (first_right, first_left)
                    assert max(Counter(zip(vi, ui)).values()) >= 3
                    assert ((pts[:, 0] == 0) & np.signbit(pts[:, 0]) & ok).sum() >= 2       # x = -0.0 lands
                for vd in (0, 1):
                    depth, P_used = run_reference(dirs[calib], scan, cam, bool(vd))
                    assert depth.shape == (h, w) and np.array_equal(P_used, P)
                    gaps, vals = sparse(depth)
                    out["%s/cam%d/vd%d/gaps" % (case, cam, vd)] = gaps
                    out["%s/cam%d/vd%d/values" % (case, cam, vd)] = vals
                print("%-10s cam %d: %6d points, %6d land, %5d duplicate keys, %6d non-zero pixels"
                      % (case, cam, len(pts), int(ok.sum()), dupes, len(vals)))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size // 1024, "KB")
    assert size < 1 << 20, "a committed file must stay under 1 MiB"


if __name__ == "__main__":
    main()
