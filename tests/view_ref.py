"""An independent numpy float64 reference of the view rasteriser (bbd_view_*), written from the contract in
include/bbd_hip.h and not from the kernels: points through `np.minimum.at` on uint64 keys, lines by a test of EVERY
pixel of the canvas against every segment with the textbook point-to-segment distance (no bounding boxes).

Besides the canvas it reports which pixels a BORDERLINE primitive touches - where a second float64 program may
legitimately differ (tests/view_checks.py `accept`):
  * a point whose u or v lies within EDGE of a pixel edge (every pixel its footprint could reach either way),
  * a pixel in which the two smallest different keys offered by points have ranks that differ by at most one
    (depths that round to float32 within one ulp of each other),
  * a pixel centre whose distance from a segment lies within EDGE of width / 2.

Test infrastructure only."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
EDGE = 1e-9
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


class Canvas:
    def __init__(self, H, W):
        self.H, self.W = H, W
        self.clear()

    def clear(self):
        self.cells = np.full(self.H * self.W, EMPTY, np.uint64)
        self.counters = np.zeros(4, np.int64)                        # offered, drawn, clipped, rejected
        self.excused = np.zeros(self.H * self.W, bool)
        self.borderline_points = 0
        self._offers = []                                            # (cells, keys) of every point drawn

    # ------------------------------------------------------------------------------------------------------ points
    def points(self, vertices, view, count=None, size=1):
        H, W = self.H, self.W
        v = np.asarray(vertices).view(VERTEX).reshape(-1)
        n = len(v) if count is None else min(max(int(count), 0), len(v))
        v = v[:n]
        xyz1 = np.stack([v["x"].astype(np.float64), v["y"].astype(np.float64), v["z"].astype(np.float64), np.ones(n)], 1)
        with np.errstate(all="ignore"):
            p = np.stack([(xyz1 * np.asarray(view, np.float64).reshape(4, 4)[r]).sum(1) for r in range(4)], 1)
            u, w, d, p3 = p[:, 0] / p[:, 3], p[:, 1] / p[:, 3], p[:, 2], p[:, 3]
            finite = np.isfinite(u) & np.isfinite(w) & np.isfinite(d) & np.isfinite(p3)
            behind = finite & ((p3 <= 0) | (d <= 0))
            front = finite & ~behind
            fu, fv = np.floor(u), np.floor(w)
            half = size // 2
            on = front & (fu + half >= 0) & (fu - half <= W - 1) & (fv + half >= 0) & (fv - half <= H - 1)
            rank = np.uint64(0x80000000) | (d.astype(np.float32).view(np.uint32) >> np.uint32(1)).astype(np.uint64)
        colour = (v["red"].astype(np.uint64) << np.uint64(24)) | (v["green"].astype(np.uint64) << np.uint64(16)) | \
                 (v["blue"].astype(np.uint64) << np.uint64(8)) | np.uint64(0xFF)
        key = (rank << np.uint64(32)) | colour
        self.counters += [n, int(on.sum()), int((behind | (front & ~on)).sum()), int((~finite).sum())]
        # borderline: u or v next to a pixel edge - everything a footprint shifted by one pixel could cover is excused
        with np.errstate(all="ignore"):
            near_edge = front & ((np.abs(u - np.round(u)) < EDGE) | (np.abs(w - np.round(w)) < EDGE))
        self.borderline_points += int(near_edge.sum())
        for i in np.nonzero(near_edge)[0]:
            if abs(fu[i]) < 1e9 and abs(fv[i]) < 1e9:
                x0, x1 = int(fu[i]) - half - 1, int(fu[i]) + half + 1
                y0, y1 = int(fv[i]) - half - 1, int(fv[i]) + half + 1
                m = self.excused.reshape(H, W)
                m[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = True
        idx = np.nonzero(on)[0]
        px, py = fu[idx].astype(np.int64), fv[idx].astype(np.int64)
        for dy in range(-half, half + 1):
            for dx in range(-half, half + 1):
                x, y = px + dx, py + dy
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                cell, k = (y * W + x)[ok], key[idx][ok]
                self._offer_points(cell, k)

    def _offer_points(self, cell, k):
        np.minimum.at(self.cells, cell, k)
        self._offers.append((cell, k))

    def depth_excused(self):
        """Pixels in which the two smallest different keys that points offered have ranks within one of each other."""
        out = np.zeros(self.H * self.W, bool)
        if not self._offers:
            return out
        cell = np.concatenate([c for c, _ in self._offers])
        key = np.concatenate([k for _, k in self._offers])
        if not len(cell):
            return out
        pairs = np.unique(np.stack([cell.astype(np.uint64), key], 1), axis=0)          # sorted by cell, then key
        same = pairs[1:, 0] == pairs[:-1, 0]
        first_of_cell = np.concatenate([[True], ~same])
        second = np.concatenate([[False], first_of_cell[:-1]]) & ~first_of_cell        # the row after a cell's first
        gap = (pairs[second, 1] >> np.uint64(32)).astype(np.int64) - (pairs[np.nonzero(second)[0] - 1, 1]
                                                                       >> np.uint64(32)).astype(np.int64)
        out[pairs[second, 0][gap <= 1].astype(np.int64)] = True
        return out

    # ------------------------------------------------------------------------------------------------------- lines
    def lines(self, xyz, view, colour=(0, 0, 0), width=2.0, layer=0, closed=False):
        H, W = self.H, self.W
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        P = len(xyz)
        V = np.asarray(view, np.float64).reshape(4, 4)
        with np.errstate(all="ignore"):
            p = np.concatenate([xyz, np.ones((P, 1))], 1) @ V.T
            u, w, d, p3 = p[:, 0] / p[:, 3], p[:, 1] / p[:, 3], p[:, 2], p[:, 3]
            good = np.isfinite(u) & np.isfinite(w) & np.isfinite(d) & np.isfinite(p3) & (p3 > 0) & (d > 0)
        r, g, b = (int(c) for c in colour)
        key = np.uint64(((0x7FFFFFFF - int(layer)) << 32) | (r << 24) | (g << 16) | (b << 8) | 0xFF)
        pairs = [(0, 0)] if P == 1 else [(s, s + 1) for s in range(P - 1)] + ([(P - 1, 0)] if closed and P > 2 else [])
        radius = width / 2.0
        for s, t in pairs:
            if not (good[s] and good[t]):
                continue
            ax, ay, ex, ey = u[s], w[s], u[t] - u[s], w[t] - w[s]
            cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)              # every pixel centre of the canvas
            ll = ex * ex + ey * ey
            tt = np.clip(((cx - ax) * ex + (cy - ay) * ey) / ll, 0.0, 1.0) if ll > 0 else np.zeros_like(cx)
            dist = np.hypot(cx - (ax + tt * ex), cy - (ay + tt * ey)).reshape(-1)
            self.excused |= np.abs(dist - radius) < EDGE
            hit = dist <= radius
            self.cells[hit] = np.minimum(self.cells[hit], key)

    # ----------------------------------------------------------------------------------------------------- resolve
    def image(self, background=(255, 255, 255)):
        c = self.cells
        rgb = np.stack([(c >> np.uint64(24)) & np.uint64(0xFF), (c >> np.uint64(16)) & np.uint64(0xFF),
                        (c >> np.uint64(8)) & np.uint64(0xFF)], 1).astype(np.uint8)
        rgb[c == EMPTY] = np.asarray(background, np.uint8)
        return rgb.reshape(self.H, self.W, 3)

    def all_excused(self):
        return self.excused | self.depth_excused()


def scale_bar(metres):
    """The largest of 1, 2, 5 x 10^k that does not exceed `metres`, by trying them in ascending order."""
    best, k = None, -12
    while 10.0 ** k <= metres:
        for m in (1, 2, 5):
            if m * 10.0 ** k <= metres:
                best = m * 10.0 ** k
        k += 1
    return best
