"""Build + bind the host port of the colour-mapped disparity (tests/host_port/bbd_viz_port.cpp).

Test infrastructure only, in the manner of tests/host_port.py: `VizPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.disp_viz`, so the CPU tier runs the product's Python plumbing (descriptor table, ragged views,
LUT) with the exact per-pixel arithmetic of bbd_viz.hip (bbd_viz_math.h)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_viz_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_viz_port.so")
DEPS = [SRC, os.path.join(HERE, "..", "baseboostdepth_amd", "csrc", "bbd_math.h"),
        os.path.join(HERE, "..", "baseboostdepth_amd", "csrc", "bbd_viz_math.h"),
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

    def disp_viz_scratch_ints(self, n):
        return self._dll.hp_disp_viz_scratch_ints(n)


class VizPortBackend:
    name = "viz-host-port"

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
