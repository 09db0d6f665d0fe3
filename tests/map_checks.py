"""The scene map's cases and acceptance rules, shared by the CPU tier (tests/test_map_port.py: the host port) and the GPU
tier (tests/test_gpu_map.py: the device).  Test infrastructure only.

Three checks:
  1 fusion     from the per-point (key, q, rgb) the host port produced (`port_points`), the numpy fusion
               (`map_ref.fuse`) must give the vertices, counts and order of the implementation under test, byte for byte.
               The device is held to the port's per-point values: it must equal the port's result byte for byte.
  2 per point  the port's world positions (v + q / 65536) voxel lie within tau + voxel / 65536 of the float64 reference's:
               the second term is the quantisation, tau = 16 2^-24 |scale| max_depth max|ray| (the float32
               back-projection's roundings: three for the ray, one for its product with d, carried through a rotation,
               with room) + 8 2^-52 max|t|.  Computed per case and printed next to the measured worst.
  3 drops      kept and out-of-range counts equal the float64 reference's.  The inputs keep every point further than tau
               from a depth limit and from the +-2^20 range (asserted on the reference).

Shapes are the smallest at which the kernel can go wrong: 3 frames of 12 x 20, strides 1 and 2, a window that cuts two
rows and three columns."""
import ctypes
import functools

import numpy as np
import torch

import map_ref as ref
from baseboostdepth_amd import pointcloud

N, H, W = 3, 12, 20
LO, HI = 0.5, 30.0
WINDOW = (1, 11, 1, 18)                 # cuts rows 0 and 11, columns 0, 18 and 19
INV_K = pointcloud.intrinsics(H, W)
WORST = {}                              # case -> (measured worst, bound) of check 2


def rotation(w):
    th = np.linalg.norm(w)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make_poses(rng, centre, spread, turn=0.05):
    P = np.tile(np.eye(4), (N, 1, 1))
    for i in range(N):
        P[i, :3, :3] = rotation(rng.uniform(-1, 1, 3) * turn + 1e-3)
        P[i, :3, 3] = np.asarray(centre, np.float64) + rng.uniform(-1, 1, 3) * spread
    return P


# name -> keyword changes against the base case
CASES = {
    "merge":      dict(voxel=2.5, T=1024),                       # tens of points per voxel, frames meet in a voxel
    "merge_s2":   dict(voxel=2.5, T=1024, stride=2),
    "merge_win":  dict(voxel=2.5, T=1024, window=WINDOW),
    "merge_min3": dict(voxel=1.0, T=1024, min_points=3),
    "scaled":     dict(voxel=1.0, T=1024, scale=1.7, stride=2, window=WINDOW),
    "fine":       dict(voxel=1e-3, T=2048),                      # nothing merges
    "negative":   dict(voxel=0.5, T=2048, centre=(-50.0, -30.0, -80.0)),
    "far":        dict(voxel=0.2, T=2048, far_frame=1),          # frame 1 lies beyond 2^20 voxels
    "bad_disp":   dict(voxel=0.5, T=2048, holes=True),           # zero and NaN disparities, depths outside the limits
    "nan_scale":  dict(voxel=0.5, T=1024, scale=float("nan")),
    "probe":      dict(voxel=2.5, T=256),                        # 720 candidates, < 128 voxels: long probe chains
    "overflow":   dict(voxel=1e-3, T=64, window=(0, 4, 0, 20)),  # 240 distinct voxels for 64 slots
    "depth_in":   dict(voxel=1.0, T=1024, is_depth=True),
}
RAISES = {"nan_scale": "scale is NaN", "overflow": r"table of 64 slots is full.*--map_capacity"}


@functools.lru_cache(maxsize=None)
def make(name):
    kw = dict(voxel=0.2, T=1024, stride=1, window=None, scale=None, min_points=1, is_depth=False, centre=(0.0, 0.0, 0.0),
              far_frame=None, holes=False)
    kw.update(CASES[name])
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.stack([6.0 + 2.0 * np.sin(0.4 * xx + i) + 1.5 * np.cos(0.6 * yy - i) + rng.uniform(-0.2, 0.2, (H, W))
                      for i in range(N)])                                       # 2.3 .. 9.7
    if kw["holes"]:
        depth[0, 2, 3:9] = 100.0                                                # beyond max_depth
        depth[1, 5, 1:6] = 0.1                                                  # nearer than min_depth
    values = depth if kw["is_depth"] else 1.0 / depth
    disp = values.astype(np.float32)
    if kw["holes"]:
        disp[0, 0, :4] = 0.0
        disp[2, 7, 5:12] = np.nan
        disp[1, 9, 3] = np.inf
        disp[2, 1, 1] = -0.2
    poses = make_poses(rng, kw["centre"], 0.3)
    if kw["far_frame"] is not None:
        poses[kw["far_frame"], :3, 3] += np.array([3.0e5, 0.0, 0.0])           # 1.5e6 voxels of 0.2
    kw.update(disp=disp, rgb=rng.random((N, 3, H, W)).astype(np.float32), poses=poses)
    return kw


def call_kw(case):
    return dict(scale=case["scale"], window=case["window"], stride=case["stride"], min_depth=LO, max_depth=HI,
                voxel=case["voxel"], is_depth=case["is_depth"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference's points of a case (computed once, shared, never changed)."""
    case = make(name)
    p = ref.points(case["disp"], case["rgb"], case["poses"], INV_K, backproject="float64", **call_kw(case))
    for v in p.values():
        v.setflags(write=False)
    return p


def tau(case):
    s = 1.0 if case["scale"] is None or np.isnan(case["scale"]) else abs(case["scale"])
    ys, xs = ref.grid(H, W, None, 1)
    iK = INV_K.astype(np.float64)
    rays = np.stack([iK[j, 0] * xs + iK[j, 1] * ys + iK[j, 2] for j in range(3)], -1)
    return 16 * 2.0 ** -24 * s * HI * np.linalg.norm(rays, axis=-1).max() \
        + 8 * 2.0 ** -52 * np.abs(case["poses"][:, :3, 3]).max()


def new_map(case, backend, device):
    return pointcloud.SceneMap(case["voxel"], case["T"], device, backend)


def add(scene, case, device, frames=slice(None), merge=True):
    scale = None if case["scale"] is None else torch.tensor([0.0, case["scale"]], dtype=torch.float64).to(device)[1:]
    scene.add(torch.from_numpy(case["disp"][frames]).to(device), torch.from_numpy(case["rgb"][frames]).to(device),
              torch.from_numpy(case["poses"][frames]).to(device), INV_K, scale=scale, stride=case["stride"],
              window=case["window"], min_depth=LO, max_depth=HI, is_depth=case["is_depth"], merge=merge)


def counters(scene):
    return scene.state.counters.cpu().numpy().copy()


def run(name, backend, device, split=False, merge=True):
    """(vertices, counts, stats) of a case, or the raised RuntimeError for the cases of RAISES; the counters either way.
    `split`: one call per frame instead of one call of three frames; `merge=False`: BBD_MAP_NO_MERGE."""
    case = make(name)
    scene = new_map(case, backend, device)
    if split:
        for i in range(N):
            add(scene, case, device, slice(i, i + 1), merge)
    else:
        add(scene, case, device, merge=merge)
    try:
        out = scene.finish(case["min_points"])
    except RuntimeError as e:
        out = e
    return out, counters(scene)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def port_points(port, disp, rgb, poses, inv_K, scale, window, stride, min_depth, max_depth, voxel, is_depth):
    """What `bbd_map_point` makes of every candidate of a call (numpy inputs): verdict int32 [G], key int64 [G],
    q uint32 [G,3], rgb uint32 [G,3]; key, q and rgb are meaningful where verdict == 1 (kept)."""
    disp, rgb = np.ascontiguousarray(disp, np.float32), np.ascontiguousarray(rgb, np.float32)
    poses, inv_K = np.ascontiguousarray(poses, np.float64).reshape(-1, 16), np.ascontiguousarray(inv_K, np.float32)
    n, h, w = disp.shape
    G = n * h * w
    verdict, key = np.zeros(G, np.int32), np.zeros(G, np.int64)
    q, col = np.zeros((G, 3), np.uint32), np.zeros((G, 3), np.uint32)
    sc = None if scale is None else np.array([scale], np.float64)
    p = lambda a: ctypes.c_void_p(0 if a is None else a.ctypes.data)   # noqa: E731
    r0, r1, c0, c1 = window or (0, h, 0, w)
    fn = port.dll.hp_map_points
    fn.restype = ctypes.c_int
    got = fn(p(disp), p(rgb), p(poses), p(inv_K), p(sc), *[ctypes.c_int(v) for v in (n, h, w, r0, r1, c0, c1, stride)],
             ctypes.c_double(min_depth), ctypes.c_double(max_depth), ctypes.c_double(voxel),
             ctypes.c_int(1 if is_depth else 0), p(verdict), p(key), p(q), p(col))
    assert 0 <= got <= G, got
    return verdict[:got], key[:got], q[:got], col[:got]


def check(name, out, counts4, port):
    """Checks 1 to 3 of a finished case against the port's per-point values and the float64 reference."""
    case = make(name)
    verdict, key, q, col = port_points(port, case["disp"], case["rgb"], case["poses"], INV_K, **call_kw(case))
    want = reference(name)
    kept = verdict == ref.KEPT
    t = tau(case)
    # 3 drops: the reference's verdicts, and no reference point near a limit
    s = 1.0 if case["scale"] is None else case["scale"]
    ys, xs = ref.grid(H, W, case["window"], case["stride"])
    raw = case["disp"][:, ys, xs]
    with np.errstate(all="ignore"):
        dm = (s * (raw if case["is_depth"] else np.float32(1) / raw).astype(np.float64)).reshape(-1)
    near = np.isfinite(dm) & ((np.abs(dm - LO) <= t) | (np.abs(dm - HI) <= t))
    edge = np.abs(np.abs(np.floor(want["X"] / case["voxel"])) - ref.HALF) * case["voxel"] <= t
    assert not near.any() and not (edge.any(-1) & (want["verdict"] != ref.REJECTED)).any(), name
    assert np.array_equal(verdict, want["verdict"]), name
    assert counts4[0] == verdict.size and counts4[2] == (verdict == ref.OUT_OF_RANGE).sum(), (name, counts4)
    assert counts4[1] + counts4[3] == kept.sum(), (name, counts4)
    # 2 per point
    v = np.stack([((key[kept] >> (21 * (2 - j))) & 0x1fffff) - ref.HALF for j in range(3)], -1)
    mine = (v + q[kept].astype(np.float64) / 65536.0) * case["voxel"]
    worst = float(np.abs(mine - want["X"][kept]).max()) if kept.any() else 0.0
    bound = t + case["voxel"] / 65536.0
    WORST[name] = (worst, bound)
    print("%s: %d candidates, %d kept; per-point worst %.3e, bound %.3e (tau %.3e)" % (name, verdict.size, kept.sum(), worst,
                                                                                     bound, t))
    assert worst <= bound, name
    # 1 fusion
    if isinstance(out, RuntimeError):
        return
    assert counts4[3] == 0
    verts, counts, stats = out
    want_v, want_c, _ = ref.fuse(key[kept], q[kept], col[kept], case["voxel"], case["min_points"])
    assert same_bytes(verts, want_v.astype(pointcloud.VERTEX_DTYPE)) and same_bytes(counts, want_c), name
    assert stats == {"candidates": int(verdict.size), "kept": int(kept.sum()),
                     "dropped_range": int((verdict == ref.OUT_OF_RANGE).sum()), "dropped_full": 0, "voxels": int(want_v.size)}


def same_result(a, b):
    """Two `run` results agree byte for byte (or raised the same error) and have equal counters."""
    (oa, ca), (ob, cb) = a, b
    if isinstance(oa, RuntimeError) or isinstance(ob, RuntimeError):
        return isinstance(oa, RuntimeError) and isinstance(ob, RuntimeError) and str(oa) == str(ob) and np.array_equal(ca, cb)
    return same_bytes(oa[0], ob[0]) and same_bytes(oa[1], ob[1]) and oa[2] == ob[2] and np.array_equal(ca, cb)


# Argument errors of the three entries: (entry, change, status).  `change` edits a dict of valid arguments.
BAD = [
    ("clear", dict(keys=None), -1), ("clear", dict(pos=None), -1), ("clear", dict(col=None), -1),
    ("clear", dict(counters=None), -1), ("clear", dict(T=0), -1), ("clear", dict(T=96), -1), ("clear", dict(T=-4), -1),
    ("accumulate", dict(keys=None), -1), ("accumulate", dict(counters=None), -1), ("accumulate", dict(disp=None), -1),
    ("accumulate", dict(rgb=None), -1), ("accumulate", dict(poses=None), -1), ("accumulate", dict(inv_K=None), -1),
    ("accumulate", dict(T=100), -1), ("accumulate", dict(n=0), -1), ("accumulate", dict(h=0), -1),
    ("accumulate", dict(w=-1), -1), ("accumulate", dict(stride=0), -1), ("accumulate", dict(voxel=0.0), -1),
    ("accumulate", dict(voxel=-1.0), -1), ("accumulate", dict(voxel=float("inf")), -1),
    ("accumulate", dict(voxel=float("nan")), -1), ("accumulate", dict(min_depth=31.0), -1),
    ("accumulate", dict(min_depth=float("nan")), -1), ("accumulate", dict(flags=4), -1), ("accumulate", dict(flags=-1), -1),
    ("accumulate", dict(n=60000, h=300, w=200), -2),
    ("finish", dict(keys=None), -1), ("finish", dict(out_keys=None), -1), ("finish", dict(vertices=None), -1),
    ("finish", dict(out_counts=None), -1), ("finish", dict(m=None), -1), ("finish", dict(scratch=None), -1),
    ("finish", dict(min_points=0), -1), ("finish", dict(voxel=0.0), -1), ("finish", dict(T=48), -1),
    ("finish", dict(scratch_ints=0), -1), ("finish", dict(misalign=8), -1),
]
ORDER = {
    "clear": "keys pos col counters T".split(),
    "accumulate": "keys pos col counters T disp rgb poses inv_K scale n h w r0 r1 c0 c1 stride min_depth max_depth voxel "
                  "flags".split(),
    "finish": "keys pos col T min_points voxel out_keys vertices out_counts m scratch scratch_ints".split(),
}


def bad_argument_sweep(status, device):
    """Every row of BAD through `status(name, *args)` (the port's or the device library's raw call): the status is the
    ABI's, and no buffer changes.  Ends with the valid call, which does write."""
    from baseboostdepth_amd._lib import ptr
    T = 64
    case = make("merge")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    bufs = dict(keys=torch.full((T,), 7, dtype=torch.int64), pos=torch.full((T, 3), 7, dtype=torch.int64),
                col=torch.full((T, 4), 7, dtype=torch.int32), counters=torch.full((4,), 7, dtype=torch.int64),
                out_keys=torch.full((T,), 7, dtype=torch.int64), vertices=torch.full((T * 16 + 16,), 7, dtype=torch.uint8),
                out_counts=torch.full((T,), 7, dtype=torch.int32), m=torch.full((1,), 7, dtype=torch.int32),
                scratch=torch.full((4,), 7, dtype=torch.int32))
    bufs = {k: v.to(device) for k, v in bufs.items()}
    ins = dict(disp=dev(case["disp"]), rgb=dev(case["rgb"]), poses=dev(case["poses"]), inv_K=dev(INV_K))
    before = {k: v.clone() for k, v in bufs.items()}
    valid = dict(T=T, scale=None, n=N, h=H, w=W, r0=0, r1=H, c0=0, c1=W, stride=1, min_depth=LO, max_depth=HI, voxel=0.5,
                 flags=0, min_points=1, scratch_ints=4)

    def call(entry, change):
        args = dict(valid)
        args.update({k: ptr(v) for k, v in list(bufs.items()) + list(ins.items())})
        args["scale"] = ptr(None)
        for k, v in change.items():
            if k == "misalign":
                args["vertices"] = type(args["vertices"])(bufs["vertices"].data_ptr() + v)
            else:
                args[k] = ptr(None) if v is None else v
        return status("bbd_map_" + entry, *[args[k] for k in ORDER[entry]])

    for entry, change, want in BAD:
        assert call(entry, change) == want, (entry, change)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    for entry in ("clear", "accumulate", "finish"):
        assert call(entry, {}) == 0
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    assert int(bufs["counters"][0]) == N * H * W and 0 < int(bufs["m"][0]) <= T


# ---------------------------------------------------------------------------- a synthetic sequence for evaluate_pose
SEQ_H, SEQ_W, SEQ_FRAMES = 12, 20, 12


class PassEncoder(torch.nn.Module):
    num_ch_enc = np.array([6])

    def forward(self, x):
        return [x]


class SpotPoseDecoder(torch.nn.Module):
    """Stands in for PoseDecoder: a few pixels of the two frames times constants ([n, 2, 1, 3] twice)."""
    SPOTS = ((0, 1, 2), (1, 3, 5), (2, 6, 11), (1, 2, 9), (2, 7, 3), (0, 4, 14))

    def forward(self, input_features):
        x = input_features[0][-1]
        first = torch.stack([x[:, c, r, col] for c, r, col in self.SPOTS], 1)
        second = torch.stack([x[:, 3 + c, r, col] for c, r, col in self.SPOTS], 1)
        diff = second - first
        axisangle = (diff[:, :3] * 0.05).view(-1, 1, 1, 3)
        translation = (diff[:, 3:] * 0.2 + torch.tensor([0.0, 0.0, -0.45], device=x.device)).view(-1, 1, 1, 3)
        return torch.cat([axisangle, axisangle * 0.5], 1), torch.cat([translation, translation * 0.5], 1)


class RampDepthDecoder(torch.nn.Module):
    """Stands in for DepthDecoder: a sigmoid disparity from the image and the pixel's place, [n,1,H,W]."""

    def forward(self, features):
        x = features[-1]
        yy, xx = torch.meshgrid(torch.arange(SEQ_H, dtype=torch.float32, device=x.device),
                                torch.arange(SEQ_W, dtype=torch.float32, device=x.device), indexing="ij")
        return {("disp", 0): 0.02 + 0.05 * torch.sigmoid(x.mean(1, keepdim=True) + 0.2 * yy - 0.1 * xx)}


def models():
    return PassEncoder(), SpotPoseDecoder(), PassEncoder(), RampDepthDecoder()


def setup_sequence(tmp_path, **flags):
    """A 12-frame odometry sequence on disk (empty frame files, a split), its options, pool, ground truth and loader."""
    import os
    import types
    import traj_checks as tc
    rng = np.random.default_rng(8)
    pool = torch.from_numpy(rng.random((SEQ_FRAMES, 3, SEQ_H, SEQ_W)).astype(np.float32))
    d = tmp_path / "odom" / "sequences" / "09" / "image_2" / "data"
    os.makedirs(d, exist_ok=True)
    for t in range(SEQ_FRAMES):                               # `windows` only asks whether the frames exist
        open(d / ("%06d.jpg" % t), "wb").close()
    os.makedirs(tmp_path / "splits" / "odom", exist_ok=True)
    with open(tmp_path / "splits" / "odom" / "test_files_09.txt", "w") as f:
        f.write("".join("9 %d l\n" % t for t in range(SEQ_FRAMES - 1)))
    gt = tc.make("noisy63")["gt"][:SEQ_FRAMES]
    opt = types.SimpleNamespace(eval_split="odom_9", splits_dir=str(tmp_path / "splits"), kt_path=str(tmp_path / "kitti"),
                                odom_path=None, height=SEQ_H, width=SEQ_W, skip_frame=2, track_length=1, cuda=0, num_layers=18,
                                load_weights_folder="None", num_workers=0, **flags)
    loader = [{("color", 0, 0): pool[:7]}, {("color", 0, 0): pool[7:]}]
    return opt, pool, gt, loader
