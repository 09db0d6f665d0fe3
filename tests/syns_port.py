"""Build + bind the host port of the SYNS-Patches metrics (tests/host_port/bbd_syns_port.cpp).

Test infrastructure only, in the manner of tests/velo_port.py: `SynsPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.evaluation.pred_edges / distance_transform / edge_metrics / pointcloud_metrics` and of
`ops.chamfer_nn`, so the CPU tier runs the product's Python plumbing (descriptor tables, strides, scratch sizing, flags)
with the exact per-pixel arithmetic of bbd_syns.hip (bbd_syns_math.h, bbd_eval_math.h)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_syns_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_syns_port.so")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bbd_math.h"), os.path.join(CSRC, "bbd_eval_math.h"), os.path.join(CSRC, "bbd_syns_math.h"),
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

    def syns_scratch_ints(self, n, px_stride):
        return self._dll.hp_syns_scratch_ints(n, px_stride)


class SynsPortBackend:
    name = "syns-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())
        self.lib = _Sizes(self.dll)

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
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
        return fn(*conv)

    def run(self, name, anchor, *args):
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
