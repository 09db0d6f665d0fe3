"""Build + bind the host port of the odometry evaluation (tests/host_port/bbd_odom_port.cpp).

Test infrastructure only, in the manner of tests/velo_port.py: `OdomPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.evaluation.pose_ate`, so the CPU tier runs the product's Python plumbing (shape checks, ground-truth
upload, output allocation) with the exact arithmetic of bbd_odom.hip (bbd_odom_math.h).  A non-zero status raises
`BbdError`, as the HIP backend does."""
import ctypes

from port_build import build_port, call_port


def build():
    return build_port("libbbd_odom_port.so", ["bbd_odom_port.cpp"])


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
        rc = call_port(self.dll, name, args)
        if rc != 0:
            raise BbdError("%s failed with status %d" % (name, rc))
