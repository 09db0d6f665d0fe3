"""Build + bind the host port of the odometry evaluation (tests/host_port/bbd_odom_port.cpp).

Test infrastructure only, in the manner of tests/velo_port.py: `OdomPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.evaluation.pose_ate`, so the CPU tier runs the product's Python plumbing (shape checks, ground-truth
upload, output allocation) with the exact arithmetic of bbd_odom.hip (bbd_odom_math.h).  A non-zero status raises
`BbdError`, as the HIP backend does."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_odom_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_odom_port.so")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bbd_math.h"), os.path.join(CSRC, "bbd_odom_math.h"),
        os.path.join(HERE, "..", "include", "bbd_hip.h")]


def build():
    if os.path.isfile(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", LIB, SRC]
    subprocess.run(cmd, check=True)
    return LIB


class OdomPortBackend:
    name = "odom-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def run(self, name, anchor, *args):
        from baseboostdepth_amd._lib import BbdError
        fn = getattr(self.dll, name.replace("bbd_", "hp_"))
        fn.restype = ctypes.c_int
        rc = fn(*[ctypes.c_int(a) if isinstance(a, int) else a for a in args])
        if rc != 0:
            raise BbdError("%s failed with status %d" % (name, rc))
