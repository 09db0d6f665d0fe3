"""numpy reference of the scene map (bbd_map_*), written from the definitions in include/bbd_hip.h.

Test infrastructure only.  `points` evaluates every candidate of a call: with `backproject="float64"` everything after
the float32 depth d runs in float64 - the independent reference the per-point tolerance is measured against - and with
`backproject="float32"` the ray and its product with d are float32 operations, one rounding each, as the definition
writes them, so that keys and offsets are the definition's own.  `fuse` is the fusion: `np.unique` on the keys and
`np.add.at` on integer arrays."""
import numpy as np

HALF = 1 << 20
REJECTED, KEPT, OUT_OF_RANGE = 0, 1, 2
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def grid(h, w, window, stride):
    """Rows and columns of the candidates, raster order."""
    r0, r1, c0, c1 = window or (0, h, 0, w)
    r0, r1, c0, c1 = max(r0, 0), min(r1, h), max(c0, 0), min(c1, w)
    ys, xs = np.meshgrid(np.arange(r0, r1, stride), np.arange(c0, c1, stride), indexing="ij")
    return ys.reshape(-1), xs.reshape(-1)


def points(disp, rgb, poses, inv_K, scale=None, window=None, stride=1, min_depth=0.5, max_depth=30.0, voxel=0.2,
           is_depth=False, backproject="float64"):
    """Every candidate, frame-major: dict of verdict [G], X float64 [G,3] (world position), key int64 [G], q int64 [G,3],
    rgb int64 [G,3]; key, q, rgb are meaningful where verdict == KEPT."""
    disp = np.asarray(disp, np.float32)
    n, h, w = disp.shape
    ys, xs = grid(h, w, window, stride)
    s = 1.0 if scale is None else float(scale)
    poses = np.asarray(poses, np.float64).reshape(n, 4, 4)
    iK = np.asarray(inv_K, np.float32)
    with np.errstate(all="ignore"):
        raw = disp[:, ys, xs]                                                    # [n, cap]
        d = raw if is_depth else np.float32(1.0) / raw                           # float32
        if backproject == "float32":
            u, v = xs.astype(np.float32), ys.astype(np.float32)
            x = np.stack([((iK[j, 0] * u + iK[j, 1] * v) + iK[j, 2])[None, :] * d for j in range(3)], -1).astype(np.float64)
        else:
            ray = np.stack([(np.float64(iK[j, 0]) * xs + np.float64(iK[j, 1]) * ys) + np.float64(iK[j, 2]) for j in range(3)], -1)
            x = ray[None] * d.astype(np.float64)[..., None]
        dm = s * d.astype(np.float64)
        passed = np.isfinite(dm) & (dm >= min_depth) & (dm <= max_depth)
        sx = s * x                                                               # [n, cap, 3]
        R, t = poses[:, :3, :3], poses[:, :3, 3]
        X = ((R[:, None, :, 0] * sx[..., 0:1] + R[:, None, :, 1] * sx[..., 1:2]) + R[:, None, :, 2] * sx[..., 2:3]) \
            + t[:, None, :]
        uu = X / voxel
        vv = np.floor(uu)
        inside = np.isfinite(X).all(-1) & (np.abs(vv) < HALF).all(-1)
        ok = passed & inside
        vi = np.where(ok[..., None], vv, 0).astype(np.int64)
        q = np.where(ok[..., None], (uu - vv) * 65536.0, 0).astype(np.int64)
        key = ((vi[..., 0] + HALF) << 42) | ((vi[..., 1] + HALF) << 21) | (vi[..., 2] + HALF)
        c = np.asarray(rgb, np.float32)[:, :, ys, xs].transpose(0, 2, 1)         # [n, cap, 3]
        tt = c * np.float32(255.0) + np.float32(0.5)
        byte = np.where(tt > 0, np.minimum(tt, np.float32(255.0)), np.float32(0.0)).astype(np.int64)
    verdict = np.where(passed, np.where(inside, KEPT, OUT_OF_RANGE), REJECTED).astype(np.int32)
    G = n * ys.size
    return {"verdict": verdict.reshape(G), "X": X.reshape(G, 3), "key": key.reshape(G), "q": q.reshape(G, 3),
            "rgb": byte.reshape(G, 3)}


def fuse(key, q, rgb, voxel, min_points=1):
    """Kept points -> (vertices as VERTEX records, counts int32, keys), voxels in ascending key order."""
    key, q, rgb = np.asarray(key, np.int64), np.asarray(q, np.int64), np.asarray(rgb, np.int64)
    keys, inverse = np.unique(key, return_inverse=True)
    M = keys.size
    sum_q, sum_c, count = np.zeros((M, 3), np.int64), np.zeros((M, 3), np.int64), np.zeros(M, np.int64)
    np.add.at(sum_q, inverse, q)
    np.add.at(sum_c, inverse, rgb)
    np.add.at(count, inverse, 1)
    keep = count >= min_points
    keys, sum_q, sum_c, count = keys[keep], sum_q[keep], sum_c[keep], count[keep]
    out = np.zeros(keys.size, VERTEX)
    for j, name in enumerate("xyz"):
        v = ((keys >> (21 * (2 - j))) & 0x1fffff) - HALF
        off = (sum_q[:, j].astype(np.float64) / count.astype(np.float64) + 0.5) / 65536.0
        out[name] = ((v.astype(np.float64) + off) * voxel).astype(np.float32)
    for j, name in enumerate(("red", "green", "blue")):
        out[name] = (sum_c[:, j] + count // 2) // count
    out["alpha"] = 255
    return out, count.astype(np.int32), keys


def scene(disp, rgb, poses, inv_K, min_points=1, **kw):
    """The whole definition: `points` with the float32 ray, then `fuse`.  Returns (vertices, counts, stats)."""
    kw.setdefault("backproject", "float32")
    p = points(disp, rgb, poses, inv_K, **kw)
    kept = p["verdict"] == KEPT
    verts, counts, _ = fuse(p["key"][kept], p["q"][kept], p["rgb"][kept], kw.get("voxel", 0.2), min_points)
    stats = {"candidates": int(p["verdict"].size), "kept": int(kept.sum()),
             "dropped_range": int((p["verdict"] == OUT_OF_RANGE).sum()), "dropped_full": 0, "voxels": int(verts.size)}
    return verts, counts, stats
