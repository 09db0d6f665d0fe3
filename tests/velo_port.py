"""Build + bind the host port of the Velodyne depth maps (tests/host_port/bbd_velo_port.cpp).

Test infrastructure only, in the manner of tests/viz_port.py: `VeloPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.velo_depth` (and of `kitti_utils.generate_depth_maps` above it), so the CPU tier runs the
product's Python plumbing (calibration, descriptor and projection tables, batching, the ragged buffer) with the exact
per-point arithmetic of bbd_velo.hip (bbd_velo_math.h)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_velo_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_velo_port.so")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bbd_math.h"), os.path.join(CSRC, "bbd_viz_math.h"), os.path.join(CSRC, "bbd_velo_math.h"),
        os.path.join(HERE, "..", "include", "bbd_hip.h")]


def build():
    if os.path.isfile(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", LIB, SRC]
    subprocess.run(cmd, check=True)
    return LIB


class _Sizes:
    def __init__(self, dll):
        self._dll = dll

    def velo_depth_scratch_ints(self, total_pixels, n_frames):
        return self._dll.hp_velo_depth_scratch_ints(total_pixels, n_frames)


class VeloPortBackend:
    name = "velo-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())
        self.lib = _Sizes(self.dll)

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def run(self, name, anchor, *args):
        fn = getattr(self.dll, name.replace("bbd_", "hp_"))
        fn.restype = ctypes.c_int
        conv = []
        for a in args:
            if isinstance(a, float):
                conv.append(ctypes.c_double(a))
            elif isinstance(a, int):
                conv.append(ctypes.c_int(a))
            else:
                conv.append(a)
        rc = fn(*conv)
        assert rc == 0, (name, rc)
