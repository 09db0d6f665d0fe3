"""Build + bind the host port of the SYNS-Patches metrics (tests/host_port/bbd_syns_port.cpp).

Test infrastructure only, in the manner of tests/velo_port.py: `SynsPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.evaluation.pred_edges / distance_transform / edge_metrics / pointcloud_metrics` and of
`ops.chamfer_nn`, so the CPU tier runs the product's Python plumbing (descriptor tables, strides, scratch sizing, flags)
with the exact per-pixel arithmetic of bbd_syns.hip (bbd_syns_math.h, bbd_eval_math.h)."""
import ctypes

from port_build import build_port, call_port


def build():
    return build_port("libbbd_syns_port.so", ["bbd_syns_port.cpp"])


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
        return call_port(self.dll, name, args)

    def run(self, name, anchor, *args):
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
