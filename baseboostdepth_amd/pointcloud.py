"""Point clouds on the host side: camera intrinsics, the one read-back of a batch of clouds, and binary PLY files.

`ops.point_cloud` leaves a batch of clouds in device memory as 16-byte vertices - x, y, z float32 little-endian, then
red, green, blue, alpha - which is exactly the vertex record the PLY header below declares.  `cloud_arrays` copies the
whole buffer to pinned host memory once and hands out numpy views of it; `write_ply` writes the header and then those
bytes as they came from the device.  Nothing here touches a point.

`SceneMap` fuses the clouds of many posed frames on a voxel grid (`ops.map_*`) and reads the finished
voxels back once, as one array of the same vertex record.
`neighbour_sources` makes the table of frames that `ops.depth_consistency` checks every frame against.

`Canvas` draws such vertices, and polylines such as trajectories, into a picture on the device (`ops.view_*`, DESIGN.md
6k); `ortho_view` and `orbit_view` make the view matrices it takes.
"""
import numpy as np
import torch

from ._lib import CLOUD_VERTEX

VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                         ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
assert VERTEX_DTYPE.itemsize == CLOUD_VERTEX

PLY_HEADER = ("ply\n"
              "format binary_little_endian 1.0\n"
              "comment baseboostdepth_amd point cloud\n"
              "element vertex {:d}\n"
              "property float x\n"
              "property float y\n"
              "property float z\n"
              "property uchar red\n"
              "property uchar green\n"
              "property uchar blue\n"
              "property uchar alpha\n"
              "end_header\n")

KITTI_K = ((0.58, 0, 0.5, 0), (0, 1.92, 0.5, 0), (0, 0, 1, 0), (0, 0, 0, 1))       # datasets.KITTIDataset, normalised


def camera_matrix(H, W, K=None, fov=None, fxfycxcy=None):
    """The float32 4x4 camera matrix of an H x W image.  At most one of: `K` (3x3 or 4x4, taken as it is), `fov` (the
    horizontal field of view in degrees: fx = fy = (W/2) / tan(fov/2), cx = W/2, cy = H/2), `fxfycxcy`.  None of them:
    the KITTI matrix of the datasets (0.58, 1.92, 0.5, 0.5 of the image size), scaled to W and H."""
    if sum(v is not None for v in (K, fov, fxfycxcy)) > 1:
        raise ValueError("intrinsics: K, fov and fxfycxcy exclude one another")
    out = np.eye(4, dtype=np.float32)
    if K is not None:
        K = np.asarray(K, dtype=np.float32)
        if K.shape not in ((3, 3), (4, 4)):
            raise ValueError("intrinsics: K must be 3x3 or 4x4, got %s" % (K.shape,))
        out[:K.shape[0], :K.shape[1]] = K
    elif fov is not None:
        if not 0.0 < float(fov) < 180.0:
            raise ValueError("intrinsics: the field of view must lie in (0, 180) degrees, got %r" % (fov,))
        f = (W / 2.0) / np.tan(np.deg2rad(float(fov)) / 2.0)
        out[0, 0], out[1, 1], out[0, 2], out[1, 2] = f, f, W / 2.0, H / 2.0
    elif fxfycxcy is not None:
        fx, fy, cx, cy = (float(v) for v in fxfycxcy)
        if fx == 0.0 or fy == 0.0:
            raise ValueError("intrinsics: focal lengths must not be zero")
        out[0, 0], out[1, 1], out[0, 2], out[1, 2] = fx, fy, cx, cy
    else:
        out = np.array(KITTI_K, dtype=np.float32)
        out[0, :] *= W
        out[1, :] *= H
    return out


def intrinsics(H, W, K=None, fov=None, fxfycxcy=None):
    """float32 [3,3] inverse intrinsics of `camera_matrix(...)`: the pseudo-inverse of the float32 4x4, as the
    reference's loaders take it."""
    return np.ascontiguousarray(np.linalg.pinv(camera_matrix(H, W, K, fov, fxfycxcy))[:3, :3].astype(np.float32))


def intrinsics_at(inv_K, size, map_size):
    """float32 [3,3] inverse intrinsics for pixels of an h x w map (`map_size`) of the same view, from those of the
    H0 x W0 image (`size`; `inv_K` [3,3] or [4,4]): inv_K . A with A = [[sx, 0, 0.5 sx - 0.5], [0, sy, 0.5 sy - 0.5],
    [0, 0, 1]], sx = W0 / w, sy = H0 / h - map pixel (x, y) lies at image position ((x + 0.5) sx - 0.5, (y + 0.5) sy -
    0.5), the pixel-centre rule of the resamplers.  The product is formed in float64 and rounded once."""
    inv_K = np.asarray(inv_K, dtype=np.float64)
    if inv_K.shape not in ((3, 3), (4, 4)):
        raise ValueError("intrinsics_at: inv_K must be 3x3 or 4x4, got %s" % (inv_K.shape,))
    (H0, W0), (h, w) = (int(v) for v in size), (int(v) for v in map_size)
    if min(H0, W0, h, w) < 1:
        raise ValueError("intrinsics_at: sizes must be at least 1, got %r and %r" % (size, map_size))
    sx, sy = W0 / w, H0 / h
    A = np.array([[sx, 0.0, 0.5 * sx - 0.5], [0.0, sy, 0.5 * sy - 0.5], [0.0, 0.0, 1.0]], dtype=np.float64)
    return np.ascontiguousarray((inv_K[:3, :3] @ A).astype(np.float32))


def neighbour_sources(n, offsets=(-1, 1)):
    """The int32 [n, len(offsets)] source table of `ops.depth_consistency` for a run of n frames: frame i is checked
    against frames i + o for every o of `offsets`, -1 (none) past the ends of the run."""
    n, offsets = int(n), [int(o) for o in offsets]
    if n < 1 or not offsets:
        raise ValueError("neighbour_sources: at least one frame and one offset are needed, got %d and %r" % (n, offsets))
    table = np.arange(n, dtype=np.int64)[:, None] + np.asarray(offsets, dtype=np.int64)[None, :]
    table[(table < 0) | (table >= n)] = -1
    return np.ascontiguousarray(table.astype(np.int32))


def cloud_arrays(vertices, counts, offsets):
    """What `ops.point_cloud` returned -> one structured array (`VERTEX_DTYPE`) per image.  ONE pinned read-back of the
    vertex buffer and one of the counts for the whole batch; the arrays are views into that host copy."""
    assert vertices.dtype == torch.uint8 and vertices.dim() == 1 and vertices.numel() % CLOUD_VERTEX == 0
    if vertices.is_cuda:
        host = torch.empty(vertices.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(vertices, non_blocking=True)
        host_counts = torch.empty(counts.shape, dtype=counts.dtype, pin_memory=True)
        host_counts.copy_(counts, non_blocking=True)
        torch.cuda.current_stream(vertices.device).synchronize()
    else:
        host, host_counts = vertices, counts
    all_vertices = host.numpy().view(VERTEX_DTYPE)
    return [all_vertices[int(o):int(o) + int(c)] for o, c in zip(offsets, host_counts.tolist())]


def write_ply(path, array):
    """The header, then the array's bytes as they are."""
    array = np.asarray(array)
    if array.dtype != VERTEX_DTYPE or array.ndim != 1:
        raise ValueError("write_ply: a one-dimensional array of dtype %s is needed, got %s %s"
                         % (VERTEX_DTYPE, array.dtype, array.shape))
    with open(path, "wb") as f:
        f.write(PLY_HEADER.format(array.shape[0]).encode("ascii"))
        f.write(np.ascontiguousarray(array).view(np.uint8).data)
    return path


def read_ply(path):
    """A file `write_ply` wrote -> its structured array.  Any other layout (ASCII, big-endian, other properties, other
    elements) is refused."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("read_ply: %s is not a PLY file" % path)
    header = data[:end + len(b"end_header\n")].decode("ascii", "replace")
    lines = header.split("\n")
    count = None
    if len(lines) > 3 and lines[3].startswith("element vertex "):
        try:
            count = int(lines[3][len("element vertex "):])
        except ValueError:
            pass
    if count is None or count < 0 or header != PLY_HEADER.format(count):
        fmt = lines[1] if len(lines) > 1 else ""
        raise ValueError("read_ply: %s does not have the layout write_ply writes (binary_little_endian 1.0, one vertex "
                         "element of float x y z and uchar red green blue alpha); its format line is %r" % (path, fmt))
    body = data[len(header):]
    if len(body) != count * CLOUD_VERTEX:
        raise ValueError("read_ply: %s declares %d vertices but holds %d bytes of them" % (path, count, len(body)))
    return np.frombuffer(body, dtype=VERTEX_DTYPE).copy()


def ortho_view(lo, hi, width, height, plane="top", margin=0.05, near=None):
    """An orthographic view of the world box [lo, hi] (three coordinates each) for a `width` x `height` canvas:
    (float64 [4,4], metres per pixel).  The box's two plotted axes are fitted into the canvas less `margin` of it on
    every side, with one scale for both, and centred.  `plane="top"`: u along +x, v along -z (forward is up), depth =
    y - near - KITTI's y points down, so the viewer is above; `plane="side"`: u along +z, v along +y, depth = x - near.
    Whatever lies before `near` on the depth axis is clipped; None puts it a kilometre before the box."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if plane not in ("top", "side"):
        raise ValueError("ortho_view: the plane is 'top' or 'side', got %r" % (plane,))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError("ortho_view: the box must be finite with lo <= hi, got %s, %s" % (lo, hi))
    if not 0.0 <= float(margin) < 0.5:
        raise ValueError("ortho_view: the margin must lie in [0, 0.5), got %r" % (margin,))
    a, b, c = (0, 2, 1) if plane == "top" else (2, 1, 0)             # the axes along u, along v, and of the depth
    inner = 1.0 - 2.0 * float(margin)
    extent = max((hi[a] - lo[a]) / (inner * width), (hi[b] - lo[b]) / (inner * height))
    mpp = float(extent) if extent > 0.0 else 1.0                     # a box without extent: a metre per pixel
    s = 1.0 / mpp
    ca, cb = 0.5 * (lo[a] + hi[a]), 0.5 * (lo[b] + hi[b])
    near = float(lo[c] - 1000.0 if near is None else near)
    flip = -1.0 if plane == "top" else 1.0
    V = np.zeros((4, 4), np.float64)
    V[0, a], V[0, 3] = s, 0.5 * width - s * ca
    V[1, b], V[1, 3] = flip * s, 0.5 * height - flip * s * cb
    V[2, c], V[2, 3] = 1.0, -near
    V[3, 3] = 1.0
    return V, mpp


def orbit_view(K, yaw_deg, pitch_deg, pivot):
    """The perspective view (float64 [4,4]) of the camera `K` (3x3 or 4x4, in pixels) after it has been turned about
    the point at depth `pivot` on its optical axis - `yaw_deg` about the y axis, then `pitch_deg` about the x axis -
    keeping its distance from that point.  Positions are in the frame of the camera before the turn, as the vertices
    of `ops.point_cloud` are.  Rows 2 and 3 are both the depth in the turned camera."""
    K = np.asarray(K, np.float64)
    if K.shape not in ((3, 3), (4, 4)):
        raise ValueError("orbit_view: K must be 3x3 or 4x4, got %s" % (K.shape,))
    pivot = float(pivot)
    if not (pivot > 0.0 and np.isfinite(pivot)):
        raise ValueError("orbit_view: the pivot's depth must be positive and finite, got %r" % (pivot,))
    y, p = np.deg2rad(float(yaw_deg)), np.deg2rad(float(pitch_deg))
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    R = Ry @ Rx                                                      # the turned camera's axes in the old frame
    centre = np.array([0.0, 0.0, pivot])
    E = np.eye(4)
    E[:3, :3] = R.T
    E[:3, 3] = centre - R.T @ centre                                 # X' = R^T (X - pivot) + pivot along the axis
    P = np.zeros((4, 4))
    P[0, :3], P[1, :3] = K[0, :3], K[1, :3]
    P[2, 2] = P[3, 2] = 1.0
    return np.ascontiguousarray(P @ E)


class Canvas:
    """A picture drawn on the device (`bbd_view_*`): `width` x `height` cells of one 64-bit key each.
    `points` and `lines` launch one kernel per call and read nothing back; what the canvas shows does not depend on
    the order of the calls."""

    STATS = ("offered", "drawn", "clipped", "rejected")

    def __init__(self, width, height, device="cuda:0", backend=None):
        from . import ops
        self.backend = backend or ops.default_backend()
        self.device = torch.device(device)
        self.width, self.height = int(width), int(height)
        self.state = ops.view_state(self.height, self.width, self.device, self.backend)

    def clear(self):
        from . import ops
        ops.view_clear(self.state, self.backend)

    def points(self, vertices, count=None, view=None, size=1):
        """16-byte vertex records (uint8 [16 n] on the device); `count`: a device int32 that limits them, or None."""
        from . import ops
        ops.view_points(self.state, vertices, view, count=count, size=size, backend=self.backend)

    def lines(self, xyz, view=None, colour=(0, 0, 0), width=2.0, layer=0, closed=False):
        """A polyline through float64 [P,3] world positions, above every point; a higher layer covers a lower one."""
        from . import ops
        ops.view_lines(self.state, xyz, view, colour=colour, width=width, layer=layer, closed=closed,
                       backend=self.backend)

    def image(self, background=(255, 255, 255)):
        """uint8 [H,W,3] on the device."""
        from . import ops
        return ops.view_resolve(self.state, background, self.backend)

    def read(self, background=(255, 255, 255)):
        """(image as numpy uint8 [H,W,3], stats) in ONE pinned read-back of the picture and the counters."""
        packed = torch.cat([self.image(background).reshape(-1), self.state.counters.view(torch.uint8)])
        if packed.is_cuda:
            host = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            torch.cuda.current_stream(packed.device).synchronize()
        else:
            host = packed
        flat = host.numpy()
        n = 3 * self.height * self.width
        counters = flat[n:].copy().view(np.int64)
        return flat[:n].reshape(self.height, self.width, 3).copy(), dict(zip(self.STATS, (int(c) for c in counters)))

    def save(self, path, background=(255, 255, 255)):
        """Writes the picture (PNG by the name's ending, through Pillow); returns the stats of `read`."""
        import PIL.Image as pil
        image, stats = self.read(background)
        pil.fromarray(image).save(path)
        return stats

    def stats(self):
        """The counters of `points` - offered, drawn, clipped, rejected - as a dict (a read-back of 32 bytes)."""
        return dict(zip(self.STATS, (int(c) for c in self.state.counters.cpu().tolist())))


class SceneMap:
    """A scene map: the points of posed frames fused on a grid of `voxel`-sized cells, one coloured vertex per occupied
    cell (`bbd_map_*`).  The state - an open-addressing hash table of `capacity` slots, rounded up to a
    power of two, 48 bytes each - lives on `device`; `add` launches one kernel per batch and reads nothing back."""

    DEFAULT_CAPACITY = 1 << 24
    CAPACITY_FLAG = "--map_capacity"

    def __init__(self, voxel=0.2, capacity=None, device="cuda:0", backend=None):
        from . import ops
        self.voxel = float(voxel)
        if not (self.voxel > 0.0 and np.isfinite(self.voxel)):
            raise ValueError("SceneMap: the voxel size must be positive and finite, got %r" % (voxel,))
        self.backend = backend or ops.default_backend()
        self.device = torch.device(device)
        self.state = ops.map_state(self.DEFAULT_CAPACITY if capacity is None else capacity, self.device, self.backend)
        self.capacity = self.state.T
        self.scale, self.offered = None, 0

    def clear(self):
        from . import ops
        ops.map_clear(self.state, self.backend)
        self.scale, self.offered = None, 0

    def add(self, disp, rgb, poses, inv_K, scale=None, stride=1, window=None, min_depth=0.5, max_depth=30.0,
            is_depth=False, merge=True):
        """One `ops.map_accumulate` call: see there.  `scale` is a float64 device tensor of one element, or None."""
        from . import ops
        ops.map_accumulate(self.state, disp, rgb, poses, inv_K, scale=scale, stride=stride, window=window,
                           min_depth=min_depth, max_depth=max_depth, voxel=self.voxel, is_depth=is_depth,
                           merge=merge, backend=self.backend)
        self.scale = scale if scale is not None else self.scale          # the last one given: read back by finish
        self.offered += int(disp.shape[0]) * int(disp.shape[-2]) * int(disp.shape[-1])    # no more voxels than pixels

    def finish(self, min_points=1):
        """The voxels with at least `min_points` points, in ascending key order (keys are unique: the order does not
        depend on how the table filled).  ONE pinned read-back.  Returns (vertices as `VERTEX_DTYPE`, counts int32 [M],
        stats = dict(candidates, kept, dropped_range, dropped_full, voxels)).  Raises when the table overflowed, and when
        nothing was kept because the `scale` is NaN."""
        from . import ops
        out_keys, vertices, out_counts, m = ops.map_finish(self.state, self.voxel, min_points, self.backend)
        T = self.capacity
        R = max(1, min(T, self.offered))                   # records that can have been written: all that is read back
        # plumbing: order by key.  Records past m take the largest key, so they sort behind the written ones.
        valid = torch.arange(T, device=out_keys.device) < m.to(torch.int64)
        order = torch.sort(torch.where(valid, out_keys, torch.full_like(out_keys, torch.iinfo(torch.int64).max))).indices[:R]
        words = vertices.view(torch.int32).view(T, 4)[order]
        packed = torch.cat([words.reshape(-1), out_counts[order], m, self.state.counters.view(torch.int32)]
                           + ([] if self.scale is None else [self.scale.reshape(1).view(torch.int32)])).contiguous()
        if packed.is_cuda:
            host = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            torch.cuda.current_stream(packed.device).synchronize()
        else:
            host = packed
        flat = host.numpy()
        M = int(flat[5 * R])
        counters = flat[5 * R + 1:5 * R + 9].copy().view(np.int64)
        scale = 1.0 if self.scale is None else float(flat[5 * R + 9:].copy().view(np.float64)[0])
        stats = {"candidates": int(counters[0]), "kept": int(counters[1]), "dropped_range": int(counters[2]),
                 "dropped_full": int(counters[3]), "voxels": M}
        if stats["dropped_full"] > 0:
            raise RuntimeError("SceneMap: the voxel table of %d slots is full, %d points found no slot; raise the "
                               "capacity (%s)" % (T, stats["dropped_full"], self.CAPACITY_FLAG))
        if np.isnan(scale) and stats["kept"] == 0:
            raise RuntimeError("SceneMap: the scale is NaN, so none of the %d candidate points was kept; a prediction "
                               "that never moves has no sim3 scale (--trajectory_align se3 needs none)"
                               % stats["candidates"])
        assert M <= R
        verts = flat[:4 * M].copy().view(np.uint8).view(VERTEX_DTYPE)
        return verts, flat[4 * R:4 * R + M].copy(), stats

    def render(self, canvas, view, min_points=1, size=1):
        """The voxels with at least `min_points` points into `canvas`: `ops.map_finish`, then `canvas.points` on its
        vertices and their device-side count, in slot order - a canvas does not care.  Nothing is read back; the state
        is left as `finish` leaves it."""
        from . import ops
        _, vertices, _, m = ops.map_finish(self.state, self.voxel, min_points, self.backend)
        canvas.points(vertices, count=m, view=view, size=size)
