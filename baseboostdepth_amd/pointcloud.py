"""Point clouds on the host side: camera intrinsics, the one read-back of a batch of clouds, and binary PLY files.

`ops.point_cloud` leaves a batch of clouds in device memory as 16-byte vertices - x, y, z float32 little-endian, then
red, green, blue, alpha - which is exactly the vertex record the PLY header below declares.  `cloud_arrays` copies the
whole buffer to pinned host memory once and hands out numpy views of it; `write_ply` writes the header and then those
bytes as they came from the device.  Nothing here touches a point.

`SceneMap` fuses the clouds of many posed frames on a voxel grid (`ops.map_*`) and reads the finished
voxels back once, as one array of the same vertex record.
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
