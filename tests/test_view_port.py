"""CPU tier of the view rasteriser: the host port (bbd_view_math.h through tests/host_port/bbd_view_port.cpp and the
product's `ops.view_*` / `pointcloud.Canvas`) against the independent numpy reference (tests/view_ref.py) on every case of
tests/view_checks.py, the order-freedom of the canvas, the argument rules and the view matrices."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import view_checks as vc  # noqa: E402
import view_ref as ref  # noqa: E402
from baseboostdepth_amd import ops, pointcloud  # noqa: E402

H, W = vc.H, vc.W


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.fixture(scope="module")
def references():
    return {name: vc.reference(steps) for name, steps in vc.CASES.items()}


def test_the_reference_shows_the_cases_are_what_they_are_for(references):
    r = references
    z1, z3 = r["zfight"], r["zfight3"]
    inside = int(z1.counters[1])
    covered1, covered3 = int((z1.cells != ref.EMPTY).sum()), int((z3.cells != ref.EMPTY).sum())
    # more than two blocks of lanes; depth competition is real (fewer pixels than points); the border clips footprints
    assert z1.counters.tolist() == [700, inside, 700 - inside, 0] and 300 < inside < 400 and 200 < covered1 < inside
    assert int(z3.counters[1]) > inside and covered1 < covered3 < min(9 * covered1, H * W)
    assert (inside, covered1, int(z3.counters[1]), covered3) == (335, 280, 389, 810)      # the reference's own figures
    assert z1.borderline_points == 0 and r["persp"].borderline_points == 0 and not z1.all_excused().any()
    # persp: 8 points with p3 = 0 and 12 with NaN or infinite coordinates are rejected, points behind the camera clipped
    offered, drawn, clipped, rejected = r["persp"].counters.tolist()
    v = vc.persp_points()
    assert (offered, rejected) == (700, 20) and drawn > 50
    assert clipped >= int((v["z"][20:] < -4.0).sum()) > 100 and drawn + clipped + rejected == offered
    # count: none of the late magenta records shows, and they would have
    magenta = lambda canvas: int((canvas.image().reshape(-1, 3) == (255, 0, 255)).all(1).sum())     # noqa: E731
    assert r["count"].counters[0] == 317 and magenta(r["count"]) == 0
    assert magenta(vc.reference([vc.P(vc.count_points(), vc.TOP, size=3)])) > 200
    assert r["count0"].counters.tolist() == [0, 0, 0, 0] and r["count_over"].counters[0] == 100
    # lines: wider lines cover more; the closed one returns to the start; the NaN vertex costs its two segments
    n1, n2, n5 = (int((r[k].cells != ref.EMPTY).sum()) for k in ("lines1", "lines2", "lines5"))
    assert 100 < n1 < n2 < n5 < H * W
    line = vc.polyline()
    far = vc.reference([vc.L(line[7:9], width=2.0)])                      # the segment between the far ends alone
    assert 40 < int((far.cells != ref.EMPTY).sum()) < 120
    assert int((vc.reference([vc.L(line[5:7])]).cells != ref.EMPTY).sum()) == 0          # wholly outside
    assert int((vc.reference([vc.L(line[8:11])]).cells != ref.EMPTY).sum()) == 0         # both segments touch the NaN
    assert 15 < int((vc.reference([vc.L(line[3:5], width=5.0)]).cells != ref.EMPTY).sum()) < 25    # no length: a disc
    # layers: the high bar beats the low one where they cross, both beat every point
    both = r["layers"].image()
    low = vc.reference([vc.BAR_LOW]).cells != ref.EMPTY
    high = vc.reference([vc.BAR_HIGH]).cells != ref.EMPTY
    assert (low & high).sum() > 5
    assert (both.reshape(-1, 3)[high] == (200, 30, 10)).all() and (both.reshape(-1, 3)[low & ~high] == (10, 200, 30)).all()
    assert (r["empty"].image((12, 34, 56)) == (12, 34, 56)).all()


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_port_matches_the_reference(port, references, name):
    bg = vc.BACKGROUNDS.get(name, (255, 255, 255))
    got = vc.run(vc.CASES[name], port, "cpu", bg)
    vc.accept(name, got, references[name], bg)
    assert vc.same(got, vc.run(vc.CASES[name], port, "cpu", bg))


def test_ties_go_to_the_smaller_colour_word(port):
    a, b = vc.tie_points()
    word = lambda v: (v["red"].astype(np.int64) << 16) | (v["green"].astype(np.int64) << 8) | v["blue"]     # noqa: E731
    winner = np.where((word(a) < word(b))[:, None], np.stack([a["red"], a["green"], a["blue"]], 1),
                      np.stack([b["red"], b["green"], b["blue"]], 1))
    results = [vc.run(steps, port, "cpu") for steps in (
        [vc.P(np.concatenate([a, b]), vc.PLAIN)], [vc.P(np.concatenate([b, a]), vc.PLAIN)],
        [vc.P(a, vc.PLAIN), vc.P(b, vc.PLAIN)], [vc.P(b, vc.PLAIN), vc.P(a, vc.PLAIN)],
        [vc.P(np.stack([a, b], 1).reshape(-1), vc.PLAIN)])]
    image = results[0][2]
    for i in range(30):
        assert tuple(image[i % 23, i]) == tuple(winner[i])
    assert all(vc.same(results[0], other) for other in results[1:])
    assert results[0][1].tolist() == [60, 60, 0, 0]


@pytest.mark.parametrize("name", ["layers", "mixed", "zfight3", "persp5"])
def test_the_order_of_submission_does_not_matter(port, name):
    first = vc.run(vc.CASES[name], port, "cpu")
    for steps in vc.orders(vc.CASES[name]):
        assert vc.same(first, vc.run(steps, port, "cpu"))


def test_argument_errors_write_nothing(port):
    vc.bad_argument_sweep(port.status, "cpu")


def test_the_binding_names_what_is_wrong(port):
    state = ops.view_state(H, W, "cpu", port)
    verts = torch.zeros(32, dtype=torch.uint8)
    for bad in (dict(vertices=verts.float()), dict(vertices=verts[:20]), dict(vertices=verts.view(2, 16)), dict(size=2),
                dict(view=np.eye(3)), dict(view=torch.eye(4)), dict(count=torch.zeros(1, dtype=torch.int64)),
                dict(count=torch.zeros(2, dtype=torch.int32))):
        kw = dict(vertices=verts, view=vc.TOP, count=None, size=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="view_points"):
            ops.view_points(state, kw.pop("vertices"), kw.pop("view"), backend=port, **kw)
    for bad in (dict(xyz=np.zeros((0, 3))), dict(xyz=np.zeros((4, 2))), dict(xyz=torch.zeros(4, 3)), dict(width=0.0),
                dict(width=float("nan")), dict(layer=-1), dict(layer=65536), dict(colour=(1, 2)), dict(colour=(1, 2, 256)),
                dict(view=np.eye(3))):
        kw = dict(xyz=np.zeros((2, 3)), view=vc.TOP)
        kw.update(bad)
        with pytest.raises(ValueError, match="view_lines"):
            ops.view_lines(state, kw.pop("xyz"), kw.pop("view"), backend=port, **kw)
    for bad in ((0, 5), (5, 0), (1 << 14, (1 << 14) + 1)):
        with pytest.raises(ValueError, match="view_state"):
            ops.view_state(*bad, "cpu", port)
    with pytest.raises(ValueError, match="view_resolve"):
        ops.view_resolve(state, (1, 2, 300), port)
    assert (state.cells == -1).all() and state.counters.tolist() == [0, 0, 0, 0]


def test_hip_backend_has_no_cpu_path():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    build()
    with pytest.raises(_lib.BbdError, match="no CPU path"):
        pointcloud.Canvas(W, H, "cpu", ops.HipBackend())


# ------------------------------------------------------------------------------------------------------ the views
def _project(V, xyz):
    p = V @ np.append(np.asarray(xyz, np.float64), 1.0)
    return p[0] / p[3], p[1] / p[3], p[2]


def test_ortho_view_fits_and_centres_the_box():
    lo, hi = np.array([-10.0, -2.0, 5.0]), np.array([30.0, 1.0, 25.0])
    V, mpp = pointcloud.ortho_view(lo, hi, 200, 100, plane="top", margin=0.05, near=-4.0)
    assert V.dtype == np.float64 and V.shape == (4, 4) and V[3].tolist() == [0, 0, 0, 1]
    # x spans 40 m over 180 px, z 20 m over 90 px: both 0.2222 m / px; forward (z) is up, depth = y - near
    assert mpp == pytest.approx(40.0 / 180.0)
    u0, v0, d0 = _project(V, (-10.0, -2.0, 5.0))
    u1, v1, d1 = _project(V, (30.0, 1.0, 25.0))
    assert (u0, v0, u1, v1) == pytest.approx((10.0, 95.0, 190.0, 5.0)) and (d0, d1) == pytest.approx((2.0, 5.0))
    # the tighter axis decides the scale, the other is centred
    V, mpp = pointcloud.ortho_view(lo, hi, 100, 200, plane="top", margin=0.0)
    assert mpp == pytest.approx(0.4)
    assert _project(V, (10.0, 0.0, 15.0))[:2] == pytest.approx((50.0, 100.0))
    assert _project(V, (10.0, -2.0, 15.0))[2] == pytest.approx(1000.0)              # near = lo - 1000 by default
    V, mpp = pointcloud.ortho_view(lo, hi, 100, 50, plane="side", margin=0.0, near=-20.0)
    assert mpp == pytest.approx(0.2)                                                # z: 20 m over 100 px; y: 3 m over 50
    u, v, d = _project(V, (-10.0, -2.0, 5.0))
    assert (u, d) == pytest.approx((0.0, 10.0)) and v == pytest.approx(25.0 - 1.5 / 0.2)   # +y is down the picture
    assert pointcloud.ortho_view(lo, lo, 10, 10)[1] == 1.0                         # a box without extent
    for bad in (dict(plane="front"), dict(margin=0.5), dict(hi=lo - 1), dict(lo=[np.nan, 0, 0])):
        with pytest.raises(ValueError, match="ortho_view"):
            pointcloud.ortho_view(**dict(dict(lo=lo, hi=hi, width=10, height=10), **bad))


def test_orbit_view_turns_the_camera_about_the_pivot():
    K = pointcloud.camera_matrix(60, 100, fxfycxcy=(70, 80, 49, 31)).astype(np.float64)
    still = pointcloud.orbit_view(K, 0.0, 0.0, 7.0)
    assert np.allclose(still[:2], K[:2]) and still[2].tolist() == still[3].tolist() == [0, 0, 1, 0]
    V = pointcloud.orbit_view(K[:3, :3], 15.0, -10.0, 7.0)
    assert V.dtype == np.float64 and V.shape == (4, 4) and np.array_equal(V[2], V[3])
    u, v, d = _project(V, (0.0, 0.0, 7.0))
    assert (u, v, d) == pytest.approx((49.0, 31.0, 7.0))                           # the pivot stays where it was
    # the camera's centre: the point with p = 0 in the turned frame; it keeps its distance from the pivot
    E = np.linalg.inv(np.vstack([K[:3, :3] @ np.eye(3, 4), [0, 0, 0, 1]])[:3, :3]) @ V[:3, :3]
    t = np.linalg.inv(K[:3, :3]) @ V[:3, 3]
    centre = -E.T @ t
    assert np.allclose(E @ E.T, np.eye(3)) and np.linalg.norm(centre - (0, 0, 7.0)) == pytest.approx(7.0)
    assert centre[0] < -1.0 and abs(np.degrees(np.arctan2(-centre[0], 7.0 - centre[2]))) == pytest.approx(15.0, abs=1.0)
    for bad in (dict(K=np.eye(2)), dict(pivot=0.0), dict(pivot=float("inf"))):
        with pytest.raises(ValueError, match="orbit_view"):
            pointcloud.orbit_view(**dict(dict(K=K, yaw_deg=1.0, pitch_deg=1.0, pivot=2.0), **bad))


def test_scene_map_render_draws_the_finished_voxels(port):
    """`SceneMap.render` against `finish` + the reference's points on the same vertices; the state stays usable."""
    import map_checks as mc
    case = mc.make("merge")
    scene = mc.new_map(case, port, "cpu")
    mc.add(scene, case, "cpu", slice(0, 3))
    verts, _, stats = scene.finish(2)
    lo = np.array([verts[a].min() for a in "xyz"], np.float64)
    hi = np.array([verts[a].max() for a in "xyz"], np.float64)
    V, _ = pointcloud.ortho_view(lo, hi, W, H, plane="top")
    canvas = pointcloud.Canvas(W, H, "cpu", port)
    port.calls.clear()
    scene.render(canvas, V, min_points=2, size=3)
    assert port.calls == ["bbd_map_finish", "bbd_view_points"]
    want = ref.Canvas(H, W)
    want.points(verts, V, size=3)
    cells = canvas.state.cells.numpy().view(np.uint64).reshape(-1)
    picture, got = canvas.read()
    vc.accept("render", (cells, canvas.state.counters.numpy(), picture), want)
    assert got["offered"] == stats["voxels"] == len(verts) > 20 and got["drawn"] == len(verts)
    again, _, same_stats = scene.finish(2)
    assert again.tobytes() == verts.tobytes() and same_stats == stats
