"""Build + bind the host port of the kernels' arithmetic (tests/host_port/bbd_host_port.cpp).

Test infrastructure only.  `HostPortBackend` plugs into the `backend=` seam of
baseboostdepth_amd.ops so the CPU tier exercises the product's Python plumbing (plan tables,
projection table, autograd wrappers) together with the exact per-pixel math of the HIP kernels.
"""
import ctypes

from port_build import build_port, call_port


def build():
    return build_port("libbbd_host_port.so", ["bbd_host_port.cpp", "bbd_image_port.cpp"])


class HostPortBackend:
    name = "host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())

    def num_tiles(self, H, W):
        return 1

    def num_tiles_fwd(self, H, W):
        return 1

    def num_tiles_bwd(self, H, W):
        return 1

    def smooth_chunks(self):
        return 1

    def fused_work_items(self, plan, S, H, W, backward, device):
        return None       # the work-item table is a launch-order choice of the GPU kernels

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def run(self, name, anchor, *args):
        rc = call_port(self.dll, name, args)
        assert rc == 0, (name, rc)

    def check_div(self, start, count, stride):
        self.dll.hp_check_div.restype = ctypes.c_int
        return self.dll.hp_check_div(ctypes.c_uint32(start), ctypes.c_uint32(count), ctypes.c_uint32(stride))
