"""Build + bind the host port of the flip post-processing (tests/host_port/bbd_postproc_port.cpp).

Test infrastructure only, in the manner of tests/syns_port.py: `PostprocPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.post_process_disp`, so the CPU tier runs the product's Python plumbing (shape checks, the
half split) with the exact per-pixel arithmetic of bbd_postproc.hip (bbd_postproc_math.h)."""
import ctypes

from port_build import build_port, call_port


def build():
    return build_port("libbbd_postproc_port.so", ["bbd_postproc_port.cpp"])


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
        return call_port(self.dll, name, args)

    def run(self, name, anchor, *args):
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
