"""Build + bind the host port of the scene map (tests/host_port/bbd_map_port.cpp).

Test infrastructure only, in the manner of tests/cloud_port.py: `MapPortBackend` plugs into the `backend=` seam of
`ops.map_*` / `pointcloud.SceneMap`, so the CPU tier runs the product's Python plumbing (state allocation, checks, the
ordering by key, the read-back) with the exact per-candidate arithmetic of bbd_map.hip (bbd_map_math.h).  Every other
call goes to the library of tests/traj_port.py (the trajectory and odometry ports and its stand-ins for
`bbd_gather_pairs` / `bbd_pose_matrix_fwd`), so that `evaluation.evaluate_pose(..., save_map=...)` runs whole on the
host.  A non-zero status raises `BbdError`, as the HIP backend does."""
import ctypes

import numpy as np

from port_build import build_port, call_port
import traj_port

MAP_CALLS = ("bbd_map_clear", "bbd_map_accumulate", "bbd_map_finish")


def build():
    return build_port("libbbd_map_port.so", ["bbd_map_port.cpp"])


class _Sizes:
    def __init__(self, dll):
        self._dll = dll
        dll.hp_map_state_bytes.restype = ctypes.c_long

    def map_state_bytes(self, T):
        return self._dll.hp_map_state_bytes(ctypes.c_int(T))

    def map_finish_scratch_ints(self, T):
        return self._dll.hp_map_finish_scratch_ints(ctypes.c_int(T))


class MapPortBackend:
    name = "map-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())
        self.traj_dll = ctypes.CDLL(traj_port.build())
        self.lib = _Sizes(self.dll)
        self.calls = []

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
        return call_port(self.dll if name in MAP_CALLS else self.traj_dll, name, args)

    def run(self, name, anchor, *args):
        from baseboostdepth_amd._lib import BbdError
        self.calls.append(name)
        rc = self.status(name, *args)
        if rc != 0:
            raise BbdError("%s failed with status %d" % (name, rc))

    def points(self, disp, rgb, poses, inv_K, scale, window, stride, min_depth, max_depth, voxel, is_depth):
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
        fn = self.dll.hp_map_points
        fn.restype = ctypes.c_int
        got = fn(p(disp), p(rgb), p(poses), p(inv_K), p(sc), *[ctypes.c_int(v) for v in (n, h, w, r0, r1, c0, c1, stride)],
                 ctypes.c_double(min_depth), ctypes.c_double(max_depth), ctypes.c_double(voxel),
                 ctypes.c_int(1 if is_depth else 0), p(verdict), p(key), p(q), p(col))
        assert 0 <= got <= G, got
        return verdict[:got], key[:got], q[:got], col[:got]
