"""numpy reference of `bbd_depth_consistency` and a scene renderer for its tests.  Test infrastructure only.

`consistency` restates csrc/bbd_consist_math.h independently, on whole arrays: the same types and the same order of
operations - numpy rounds every array operation on its own - so its outputs are compared with the port's and the device's
BY BYTES.  The 4x4 inverse and product are plain Python floats (IEEE doubles) in the order of bbd_odom_inv4 / _mul4d.

`render` gives the analytic depth of a small street scene - a road plane, a far wall and, optionally, a post standing on
the road - seen by a pinhole camera at a given pose, by intersecting every pixel's ray with the three shapes."""
import numpy as np

NAN_BITS = 0x7fc00000
ERR_ONE = 16777216.0
COUNTERS = 5


def inv4(a):
    """Gauss-Jordan with partial pivoting on [a | I], the first of equal pivots (bbd_odom_inv4)."""
    m = [[float(a[i][j]) for j in range(4)] + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for col in range(4):
        p, best = col, abs(m[col][col])
        for row in range(col + 1, 4):
            if abs(m[row][col]) > best:
                p, best = row, abs(m[row][col])
        m[col], m[p] = m[p], m[col]
        pivot = m[col][col]
        m[col] = [np.float64(x) / np.float64(pivot) for x in m[col]]          # numpy scalars: x / 0 is inf, not an exception
        for row in range(4):
            if row != col:
                f = m[row][col]
                m[row] = [m[row][j] - f * m[col][j] for j in range(8)]
    return [[float(m[i][4 + j]) for j in range(4)] for i in range(4)]


def mul4(a, b):
    return [[((a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]) + a[i][3] * b[3][j] for j in range(4)]
            for i in range(4)]


def clean_sources(sources, n):
    s = np.asarray(sources, np.int64).copy()
    s[(s < 0) | (s >= n)] = -1
    return s


def transforms(poses, sources):
    """float64 [n,V,12]: rows 0..2 of inv(P_src) . P_ref, zeros where there is no source."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    n = poses.shape[0]
    src = clean_sources(sources, n)
    out = np.zeros((n, src.shape[1], 12), np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            for v in range(src.shape[1]):
                if src[i, v] >= 0:
                    prod = mul4(inv4(poses[src[i, v]].tolist()), poses[i].tolist())
                    out[i, v] = np.array(prod, np.float64).reshape(16)[:12]
    return out


def _depth(raw, is_depth):
    d = raw if is_depth else np.float32(1.0) / raw
    return d, (d > 0) & np.isfinite(d)


def consistency(disp, poses, K, inv_K, sources, scale=None, threshold=0.05, min_views=1, is_depth=False):
    """dict(transforms, seen, agree, err, filtered, counters, errs, visible): the outputs of the entry, plus per source
    `errs` float32 [n,V,h,w] (NaN where not visible) and `visible` bool [n,V,h,w]."""
    disp = np.ascontiguousarray(disp, np.float32)
    n, h, w = disp.shape
    K64, iK = np.asarray(K, np.float32).astype(np.float64), np.asarray(inv_K, np.float32)
    src = clean_sources(sources, n)
    V = src.shape[1]
    s = np.float64(1.0 if scale is None else scale)
    M = transforms(poses, sources)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xf, yf = xs.astype(np.float32), ys.astype(np.float32)
    seen, agree = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w), np.uint8)
    best = np.full((n, h, w), 2.0, np.float32)
    errs = np.full((n, V, h, w), np.nan, np.float32)
    counters = np.zeros((n, COUNTERS), np.int64)
    with np.errstate(all="ignore"):
        d, valid = _depth(disp, is_depth)
        inverse = ((np.float32(1.0) / disp) if is_depth else disp).astype(np.float64)
        for i in range(n):
            p = [((iK[j, 0] * xf + iK[j, 1] * yf) + iK[j, 2]) * d[i] for j in range(3)]               # float32
            q = [s * pj.astype(np.float64) for pj in p]
            for v in range(V):
                j = int(src[i, v])
                if j < 0:
                    continue
                m = M[i, v]
                X = [((m[4 * r] * q[0] + m[4 * r + 1] * q[1]) + m[4 * r + 2] * q[2]) + m[4 * r + 3] for r in range(3)]
                z = X[2]
                c = [((K64[r, 0] * X[0] + K64[r, 1] * X[1]) + K64[r, 2] * X[2]) for r in range(3)]
                u, t = c[0] / c[2], c[1] / c[2]
                vis = valid[i] & (z > 0) & np.isfinite(z) & (u >= 0) & (u <= w - 1) & (t >= 0) & (t <= h - 1)
                if h < 2 or w < 2:
                    vis &= False
                x0 = np.minimum(np.floor(np.where(vis, u, 0.0)).astype(np.int64), max(w - 2, 0))
                y0 = np.minimum(np.floor(np.where(vis, t, 0.0)).astype(np.int64), max(h - 2, 0))
                x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
                vis &= valid[j][y0, x0] & valid[j][y0, x1] & valid[j][y1, x0] & valid[j][y1, x1]
                s00, s01, s10, s11 = inverse[j][y0, x0], inverse[j][y0, x1], inverse[j][y1, x0], inverse[j][y1, x1]
                fx, fy = u - x0.astype(np.float64), t - y0.astype(np.float64)
                top, bot = s00 + fx * (s01 - s00), s10 + fx * (s11 - s10)
                sb = top + fy * (bot - top)
                d_b = s / sb
                vis &= (d_b > 0) & np.isfinite(d_b)
                e = (np.abs(z - d_b) / (z + d_b)).astype(np.float32)
                errs[i, v] = np.where(vis, e, np.float32(np.nan))
                seen[i] += vis
                agree[i] += vis & (e.astype(np.float64) < threshold)
                counters[i, 3] += (e[vis].astype(np.float64) * ERR_ONE + 0.5).astype(np.int64).sum()
                best[i] = np.where(vis & (e < best[i]), e, best[i])
        kept = valid & (agree >= min_views)
        filtered = np.where(kept, disp, np.float32(0.0))
    err = np.where(seen > 0, best, np.array(NAN_BITS, np.uint32).view(np.float32)).astype(np.float32)
    counters[:, 0] = valid.reshape(n, -1).sum(1)
    counters[:, 1] = seen.reshape(n, -1).astype(np.int64).sum(1)
    counters[:, 2] = agree.reshape(n, -1).astype(np.int64).sum(1)
    counters[:, 4] = kept.reshape(n, -1).sum(1)
    return dict(transforms=M, seen=seen, agree=agree, err=err, filtered=filtered, counters=counters, errs=errs,
                visible=~np.isnan(errs), valid=valid)


# ---------------------------------------------------------------------------- the scene
ROAD_Y = 1.65                       # the road lies this far below the first camera (y points down)
WALL_Z = 8.0                        # the wall across the road: near enough for a wrong translation to show
POST = (0.6, 1.0, 4.0, 4.4)         # x0, x1, z0, z1 of the post: a box standing on the road, open at the top


def pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    """float64 [4,4] camera to world: the camera at (tx, ty, tz), turned by `yaw` about the vertical (y) axis."""
    P = np.eye(4)
    P[:3, :3] = [[np.cos(yaw), 0.0, np.sin(yaw)], [0.0, 1.0, 0.0], [-np.sin(yaw), 0.0, np.cos(yaw)]]
    P[:3, 3] = (tx, ty, tz)
    return P


def render(P, inv_K, h, w, post=True):
    """float64 [h,w]: the depth (z in the camera's frame) of the nearest of road, wall and post along every pixel's ray;
    0 where the ray meets none of them."""
    P, iK = np.asarray(P, np.float64), np.asarray(inv_K, np.float64)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([iK[j, 0] * xs + iK[j, 1] * ys + iK[j, 2] for j in range(3)], -1)      # z component 1: t is the depth
    ray = ray / ray[..., 2:3]
    dirs = ray @ P[:3, :3].T
    o = P[:3, 3]
    hits = []
    with np.errstate(all="ignore"):
        hits.append(np.where(dirs[..., 1] > 0, (ROAD_Y - o[1]) / dirs[..., 1], np.inf))
        hits.append(np.where(dirs[..., 2] > 0, (WALL_Z - o[2]) / dirs[..., 2], np.inf))
        if post:
            x0, x1, z0, z1 = POST
            ta, tb = (x0 - o[0]) / dirs[..., 0], (x1 - o[0]) / dirs[..., 0]
            tc, td = (z0 - o[2]) / dirs[..., 2], (z1 - o[2]) / dirs[..., 2]
            near = np.maximum(np.minimum(ta, tb), np.minimum(tc, td))
            far = np.minimum(np.maximum(ta, tb), np.maximum(tc, td))
            hits.append(np.where((near <= far) & (near > 0), near, np.inf))
    depth = np.min(np.stack(hits), 0)
    depth = np.where(depth > 0, depth, np.inf)
    return np.where(np.isfinite(depth), depth, 0.0)
