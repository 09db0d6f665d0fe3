"""Cases and acceptance rules of the view rasteriser (bbd_view_*), shared by the CPU tier
(tests/test_view_port.py: host port against tests/view_ref.py) and the GPU tier (tests/test_gpu_view.py: device against
host port, byte for byte).  The canvas is 37 x 23: no power of two hides an indexing slip.

A case is a list of steps, ("points", kwargs) or ("lines", kwargs), with numpy inputs; `run` sends them through
`pointcloud.Canvas` on a backend, `reference` through `view_ref.Canvas`.

Test infrastructure only."""
import itertools

import numpy as np
import torch

import view_ref as ref

H, W = 23, 37
N_POINTS = 700                     # more than two blocks of 256 lanes

# top view at 1.5 px / m: u = 1.5 x + 18.5, v = -1.5 z + 11.5, depth = y + 5
TOP = np.array([[1.5, 0, 0, 18.5], [0, 0, -1.5, 11.5], [0, 1, 0, 5.0], [0, 0, 0, 1]], np.float64)
# a pinhole camera 4 m behind the origin: p3 = z + 4 (exactly 0 at z = -4), f = 20 px, principal point mid-canvas
PERSP = np.array([[20, 0, 18.5, 74.0], [0, 20, 11.5, 46.0], [0, 0, 1, 4.0], [0, 0, 1, 4.0]], np.float64)
# pixels are metres: u = x, v = z, depth = y.  With dyadic coordinates every tier is exact.
PLAIN = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
EXACT = ("tie",)                   # cases in which the reference must be met without any excuse


def vertices(xyz, rgb):
    v = np.zeros(len(xyz), ref.VERTEX)
    v["x"], v["y"], v["z"] = np.asarray(xyz, np.float32).T
    v["red"], v["green"], v["blue"] = np.asarray(rgb, np.uint8).reshape(-1, 3).T
    v["alpha"] = 255
    return v


def seeded_points(seed=3, n=N_POINTS):
    """Points over a box half again as large as what TOP shows: about half land on the canvas, several per pixel."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-17, 17, n), rng.uniform(-1, 4, n), rng.uniform(-11, 11, n)], 1)
    return vertices(xyz, rng.integers(0, 256, (n, 3)))


def persp_points():
    """The seeded points with the troublemakers in front: p3 exactly 0, NaN and infinite coordinates."""
    v = seeded_points()
    v["z"][:8] = -4.0                                                  # p3 = z + 4 = 0: rejected (u, v not finite)
    v["x"][8:11], v["y"][11:13], v["z"][13:14] = np.nan, np.nan, np.nan
    v["x"][14:16], v["y"][16:17], v["z"][17:18] = np.inf, -np.inf, np.inf
    v["z"][18:20] = -np.inf
    return v


def tie_points():
    """30 pairs at one pixel and one float32 depth each, with different colours."""
    rng = np.random.default_rng(5)
    i = np.arange(30)
    xyz = np.stack([i + 0.5, 2.0 + 0.25 * (i % 4), (i % 23) + 0.5], 1)
    a = rng.integers(0, 256, (30, 3))
    b = (a + rng.integers(1, 255, (30, 3))) % 256                    # differs in every channel
    return vertices(xyz, a), vertices(xyz, b)


def count_points():
    """600 records of which 317 count; the rest would be nearest (depth 0.5) on the canvas, in magenta."""
    v = seeded_points(7, 600)
    rng = np.random.default_rng(9)
    late = 600 - 317
    v[317:] = vertices(np.stack([rng.uniform(-12, 12, late), np.full(late, -4.5), rng.uniform(-7, 7, late)], 1),
                       np.tile([255, 0, 255], (late, 1)))
    return v


def polyline():
    """40 vertices in PLAIN's pixels: horizontal, vertical and diagonal runs, a segment of no length, one that leaves the
    canvas, one wholly outside, one from a million pixels outside to a million pixels outside on the other side that
    crosses the canvas, a NaN vertex, then a seeded zigzag."""
    pts = [(3.3, 4.3), (15.3, 4.3), (15.3, 12.7), (24.3, 20.2), (24.3, 20.2), (45.2, 18.7), (50.1, 30.3),
           (18.2 - 1e6, 11.4 - 5e5), (18.2 + 1e6, 11.4 + 5e5), (np.nan, 3.0), (30.3, 2.7), (33.7, 9.3)]
    rng = np.random.default_rng(11)
    while len(pts) < 40:
        pts.append((float(rng.integers(0, W)) + 0.3, float(rng.integers(0, H)) + 0.7))
    pts = np.asarray(pts, np.float64)
    return np.stack([pts[:, 0], np.ones(len(pts)), pts[:, 1]], 1)


def P(vertices, view, count=None, size=1):
    return ("points", dict(vertices=vertices, view=view, count=count, size=size))


def L(xyz, view=PLAIN, colour=(0, 0, 0), width=2.0, layer=0, closed=False):
    return ("lines", dict(xyz=np.asarray(xyz, np.float64).reshape(-1, 3), view=view, colour=colour, width=width,
                          layer=layer, closed=closed))


BAR_LOW = L([(2.3, 1, 9.3), (34.7, 1, 9.3)], colour=(10, 200, 30), width=5.0, layer=1)
BAR_HIGH = L([(6.3, 1, 3.3), (30.7, 1, 17.7), (30.7, 1, 9.3)], colour=(200, 30, 10), width=3.0, layer=2)


def _cases():
    pts, tie_a, tie_b = seeded_points(), *tie_points()
    line = polyline()
    both = np.concatenate([tie_a, tie_b])
    c = {
        "zfight": [P(pts, TOP)],
        "zfight3": [P(pts, TOP, size=3)],
        "zfight7": [P(pts, TOP, size=7)],
        "persp": [P(persp_points(), PERSP)],
        "persp5": [P(persp_points(), PERSP, size=5)],
        "tie": [P(both, PLAIN)],
        "count": [P(count_points(), TOP, count=317, size=3)],
        "count0": [P(pts, TOP, count=0)],
        "count_over": [P(pts[:100], TOP, count=5000)],
        "lines1": [L(line, width=1.0)],
        "lines2": [L(line, width=2.0, closed=True)],
        "lines5": [L(line, width=5.0, colour=(31, 119, 180))],
        "disc": [L(line[10:11], width=5.0), L([(0.2, 1, 0.2)], width=7.0, colour=(9, 9, 9), layer=4)],
        "layers": [P(pts, TOP, size=3), BAR_LOW, BAR_HIGH],
        "empty": [],
        "mixed": [P(pts, TOP, size=3), L(line, width=2.0, layer=2), P(persp_points(), PERSP), BAR_LOW,
                  P(count_points(), TOP, count=317), L(line[10:11], width=5.0, colour=(1, 2, 3), layer=7)],
    }
    return c


CASES = _cases()
BACKGROUNDS = {"empty": (12, 34, 56), "mixed": (0, 0, 0)}


def reference(steps):
    canvas = ref.Canvas(H, W)
    for kind, kw in steps:
        getattr(canvas, kind)(**kw)
    return canvas


def run(steps, backend, device, background=(255, 255, 255)):
    """The steps through `pointcloud.Canvas` on `backend`: (cells uint64 [H*W], counters int64 [4], image uint8
    [H,W,3]).  `read` - the one read-back of `save` - must agree with the three."""
    from baseboostdepth_amd import pointcloud
    canvas = pointcloud.Canvas(W, H, device, backend)
    for kind, kw in steps:
        if kind == "points":
            verts = torch.from_numpy(kw["vertices"].view(np.uint8).copy()).to(device)
            count = None if kw["count"] is None else torch.tensor([kw["count"]], dtype=torch.int32, device=device)
            canvas.points(verts, count=count, view=kw["view"], size=kw["size"])
        else:
            canvas.lines(**kw)
    image = canvas.image(background)
    assert image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3) and image.device.type == torch.device(device).type
    cells = canvas.state.cells.cpu().numpy().view(np.uint64).reshape(-1).copy()
    counters = canvas.state.counters.cpu().numpy().copy()
    picture, stats = canvas.read(background)
    assert np.array_equal(picture, image.cpu().numpy()) and canvas.stats() == stats
    assert [stats[k] for k in ("offered", "drawn", "clipped", "rejected")] == counters.tolist()
    return cells, counters, picture


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def accept(name, got, want, background=(255, 255, 255)):
    """`got` = (cells, counters, image) of the port or the device against the reference canvas `want`: the counters
    equal, every pixel that no borderline primitive touches equal, at most 1 % of the covered pixels excused; nothing
    excused at all in the EXACT cases."""
    cells, counters, image = got
    assert counters.tolist() == want.counters.tolist(), (name, counters, want.counters)
    excused = np.zeros(want.H * want.W, bool) if name in EXACT else want.all_excused()
    covered = (want.cells != ref.EMPTY) | (cells != ref.EMPTY)
    assert np.array_equal(cells[~excused], want.cells[~excused]), (name, np.nonzero((cells != want.cells) & ~excused)[0])
    assert np.array_equal(image.reshape(-1, 3)[~excused], want.image(background).reshape(-1, 3)[~excused]), name
    assert int((excused & covered).sum()) <= 0.01 * int(covered.sum()), (name, int((excused & covered).sum()))


def orders(steps):
    """Every submission order of the steps (up to 24), and the point steps cut in three calls."""
    for perm in itertools.islice(itertools.permutations(range(len(steps))), 24):
        yield [steps[i] for i in perm]
    cut = []
    for kind, kw in steps:
        if kind == "points" and kw["count"] is None:
            n = len(kw["vertices"])
            cut += [P(kw["vertices"][a:b], kw["view"], size=kw["size"]) for a, b in ((n // 2, n), (0, n // 5), (n // 5, n // 2))]
        else:
            cut.append((kind, kw))
    yield cut


# ------------------------------------------------------------------------------------------------ argument errors
ORDER = {"clear": ("cells", "counters", "H", "W"),
         "points": ("cells", "counters", "H", "W", "vertices", "count", "n_max", "view", "size"),
         "lines": ("cells", "counters", "H", "W", "xyz", "P", "view", "rgb", "width", "layer", "closed"),
         "resolve": ("cells", "H", "W", "background", "out")}
BADARG, TOOMANY = -1, -2
BAD = [("clear", dict(cells=None), BADARG), ("clear", dict(counters=None), BADARG), ("clear", dict(H=0), BADARG),
       ("clear", dict(W=-3), BADARG), ("clear", dict(H=1 << 14, W=(1 << 14) + 1), TOOMANY),
       ("points", dict(cells=None), BADARG), ("points", dict(counters=None), BADARG), ("points", dict(vertices=None), BADARG),
       ("points", dict(view=None), BADARG), ("points", dict(H=0), BADARG), ("points", dict(W=0), BADARG),
       ("points", dict(n_max=-1), BADARG), ("points", dict(misalign=4), BADARG), ("points", dict(H=1 << 15, W=1 << 14), TOOMANY)]
BAD += [("points", dict(size=s), BADARG) for s in (0, 2, 4, 6, 8, 9, -1)]
BAD += [("lines", dict(cells=None), BADARG), ("lines", dict(counters=None), BADARG), ("lines", dict(xyz=None), BADARG),
        ("lines", dict(view=None), BADARG), ("lines", dict(P=0), BADARG), ("lines", dict(H=0), BADARG),
        ("lines", dict(W=1 << 29), TOOMANY), ("lines", dict(rgb=-1), BADARG), ("lines", dict(rgb=1 << 24), BADARG),
        ("lines", dict(layer=-1), BADARG), ("lines", dict(layer=1 << 16), BADARG), ("lines", dict(closed=2), BADARG)]
BAD += [("lines", dict(width=w), BADARG) for w in (0.0, -1.0, float("nan"), float("inf"))]
BAD += [("resolve", dict(cells=None), BADARG), ("resolve", dict(out=None), BADARG), ("resolve", dict(H=0), BADARG),
        ("resolve", dict(W=0), BADARG), ("resolve", dict(background=-1), BADARG), ("resolve", dict(background=1 << 24), BADARG),
        ("resolve", dict(H=1 << 20, W=1 << 9), TOOMANY)]


def bad_argument_sweep(status, device):
    """Every row of BAD through `status(name, *args)` (the port's or the device library's raw call): the status is the
    ABI's, and no buffer changes.  Ends with the valid calls, which do write."""
    from baseboostdepth_amd._lib import ptr
    pts, line = seeded_points(), polyline()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    bufs = dict(cells=torch.full((H * W,), 7, dtype=torch.int64), counters=torch.full((4,), 7, dtype=torch.int64),
                out=torch.full((H * W * 3,), 7, dtype=torch.uint8))
    bufs = {k: v.to(device) for k, v in bufs.items()}
    ins = dict(vertices=dev(pts.view(np.uint8)), xyz=dev(line), view=dev(TOP))
    before = {k: v.clone() for k, v in bufs.items()}
    valid = dict(H=H, W=W, n_max=len(pts), size=3, P=len(line), rgb=0x0000ff, width=2.0, layer=1, closed=0,
                 background=0xffffff)

    def call(entry, change):
        args = dict(valid)
        args.update({k: ptr(v) for k, v in list(bufs.items()) + list(ins.items())})
        args["count"] = ptr(None)
        for k, v in change.items():
            if k == "misalign":
                args["vertices"] = type(args["vertices"])(ins["vertices"].data_ptr() + v)
            else:
                args[k] = ptr(None) if v is None else v
        return status("bbd_view_" + entry, *[args[k] for k in ORDER[entry]])

    for entry, change, want in BAD:
        assert call(entry, change) == want, (entry, change)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    for entry in ("clear", "points", "lines", "resolve"):
        assert call(entry, {}) == 0
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    assert int(bufs["counters"][0]) == len(pts) and int((bufs["cells"] != -1).sum()) > 100
    assert not torch.equal(bufs["out"], before["out"])
