"""Build + bind the host port of the flip post-processing (tests/host_port/bbd_postproc_port.cpp).

Test infrastructure only, in the manner of tests/syns_port.py: `PostprocPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.post_process_disp`, so the CPU tier runs the product's Python plumbing (shape checks, the
half split) with the exact per-pixel arithmetic of bbd_postproc.hip (bbd_postproc_math.h)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_postproc_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_postproc_port.so")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bbd_math.h"), os.path.join(CSRC, "bbd_postproc_math.h"),
        os.path.join(HERE, "..", "include", "bbd_hip.h")]


def build():
    if os.path.isfile(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", LIB, SRC]
    subprocess.run(cmd, check=True)
    return LIB


class PostprocPortBackend:
    name = "postproc-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
        fn = getattr(self.dll, name.replace("bbd_", "hp_"))
        fn.restype = ctypes.c_int
        return fn(*[ctypes.c_int(a) if isinstance(a, int) else a for a in args])

    def run(self, name, anchor, *args):
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
