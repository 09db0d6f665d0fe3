"""Numpy reference of the semi-global stereo matcher (`ops.stereo_hints`, bbd_sgm_hints), written from the rules of
DESIGN.md 6p and not from csrc/bbd_sgm_math.h: whole-image array operations where the kernels walk lines, a mirrored
image as flipped copies where the kernels reflect indices, Python's floor division where the header shifts the numerator.
All integers, so device, port and this file must agree byte for byte."""
import numpy as np

INVALID = -16
COST_OOB = 31
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))


def grey(img):
    """float32 [3,H,W] in [0,1] -> uint8 luma [H,W]."""
    v = np.floor(img.astype(np.float32) * np.float32(255.0) + np.float32(0.5))
    v = np.where(v >= 255, 255, np.where(v >= 0, v, 0)).astype(np.int64)         # NaN fails both comparisons -> 0
    return ((77 * v[0] + 150 * v[1] + 29 * v[2] + 128) >> 8).astype(np.uint8)


def census(g):
    """uint8 [H,W] -> uint64 [H,W]: 9 x 7 window, bit k for the k-th offset in row-major order without the centre."""
    H, W = g.shape
    pad = np.pad(g, ((3, 3), (4, 4)), mode="edge")
    word = np.zeros((H, W), np.uint64)
    k = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            nb = pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
            word |= (nb < g).astype(np.uint64) << np.uint64(k)
            k += 1
    assert k == 62
    return word


def popcount(v):
    return np.unpackbits(v.view(np.uint8).reshape(v.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


def cost_volume(cl, cr, D):
    H, W = cl.shape
    C = np.full((H, W, D), COST_OOB, np.int64)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount(cl[:, d:] ^ cr[:, :W - d])
    return C


def aggregate(C, dx, dy, p1, p2):
    """L_r of one direction for the whole image [H,W,D]."""
    H, W, D = C.shape
    L = np.zeros_like(C)
    big = 1 << 40

    def step(c, q):                                  # c, q: [n, D]
        m = q.min(1, keepdims=True)
        below = np.concatenate([np.full((q.shape[0], 1), big), q[:, :-1]], 1) + p1
        above = np.concatenate([q[:, 1:], np.full((q.shape[0], 1), big)], 1) + p1
        return c + np.minimum(np.minimum(q, m + p2), np.minimum(below, above)) - m

    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else step(C[:, x], L[:, x - dx])
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]
            continue
        L[y] = C[y]                                                  # path starts where x - dx is outside
        lo, hi = max(0, dx), W + min(0, dx)                          # the columns that have a predecessor
        if hi > lo:
            L[y, lo:hi] = step(C[y, lo:hi], L[y - dy, lo - dx:hi - dx])
    return L


def match(left, right, D=128, paths=8, p1=10, p2=120, uniqueness=5, fill=False):
    """One image with the partner on the right (matches at x - d): float32 [3,H,W] each -> (disp16 int16 [H,W], count)."""
    gl, gr = grey(left), grey(right)
    H, W = gl.shape
    C = cost_volume(census(gl), census(gr), D)
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate(C, dx, dy, p1, p2)
    assert S.max() <= 65535
    ds = np.arange(D)
    dl = (S * 256 + ds).argmin(2)                                    # lowest S, then lowest d
    best = np.take_along_axis(S, dl[..., None], 2)[..., 0]
    unique = np.ones((H, W), bool)
    if uniqueness > 0:
        apart = np.abs(ds[None, None] - dl[..., None]) > 1
        unique = ~(apart & (S * (100 - uniqueness) < best[..., None] * 100)).any(2)
    # the right image's disparity from the same sums
    dr = np.zeros((H, W), np.int64)
    for x in range(W):
        n = min(D, W - x)
        diag = S[:, x + np.arange(n), np.arange(n)]                  # [H, n]
        dr[:, x] = (diag * 256 + np.arange(n)).argmin(1)
    xs = np.arange(W)[None] - dl
    inside = xs >= 0
    back = np.take_along_axis(dr, np.clip(xs, 0, W - 1), 1)
    valid = unique & inside & (np.abs(back - dl) <= 1)
    a = np.take_along_axis(S, np.clip(dl - 1, 0, D - 1)[..., None], 2)[..., 0]
    c = np.take_along_axis(S, np.clip(dl + 1, 0, D - 1)[..., None], 2)[..., 0]
    den = np.maximum(a + c - 2 * best, 1)
    off = ((a - c) * 16 + den) // (2 * den)                          # floor division
    off = np.where((dl == 0) | (dl == D - 1), 0, off)
    disp = np.where(valid, 16 * dl + off, INVALID).astype(np.int16)
    count = int(valid.sum())
    if fill:
        for y in range(H):
            row = disp[y]
            good = np.flatnonzero(row != INVALID)
            if good.size == 0:
                continue
            for x in np.flatnonzero(row == INVALID):
                left_of = good[good < x]
                row[x] = row[left_of[-1]] if left_of.size else row[good[0]]      # good holds the pre-fill positions
    return disp, count


def stereo_hints(left, right, side, D=128, paths=8, p1=10, p2=120, uniqueness=5, fill=False):
    """[B,3,H,W] each, side [B] -> (disp16 int16 [B,H,W], valid_count int64 [B]).  A mirrored image is matched as flipped
    copies and the result is flipped back."""
    out, counts = [], []
    for b in range(left.shape[0]):
        l, r = left[b], right[b]
        if side[b]:
            l, r = l[:, :, ::-1], r[:, :, ::-1]
        d, n = match(np.ascontiguousarray(l), np.ascontiguousarray(r), D, paths, p1, p2, uniqueness, fill)
        out.append(d[:, ::-1] if side[b] else d)
        counts.append(n)
    return np.ascontiguousarray(np.stack(out)), np.array(counts, np.int64)
