"""Build + bind the host port of the point-cloud export (tests/host_port/bbd_cloud_port.cpp).

Test infrastructure only, in the manner of tests/syns_port.py: `CloudPortBackend` plugs into the `backend=` seam of
`ops.point_cloud`, so the CPU tier runs the product's Python plumbing (descriptor rows, capacities, region offsets,
scratch sizing, flags) with the exact per-candidate arithmetic of bbd_cloud.hip (bbd_cloud_math.h).  The SYNS calls
(`bbd_chamfer_nn`, `bbd_syns_*`) go to the port of bbd_syns.hip, `bbd_depth_metrics` to the one that comes with the port
of bbd_compare.hip and `bbd_post_process_disp` to the port of bbd_postproc.hip, so that the metric the clouds are
checked against and `evaluation.evaluate(..., save_clouds=...)` run whole on the host."""
import ctypes

from port_build import build_port, call_port
import compare_port
import postproc_port
import syns_port

CLOUD_CALLS = ("bbd_point_cloud",)


def build():
    return build_port("libbbd_cloud_port.so", ["bbd_cloud_port.cpp"])


class _Sizes:
    def __init__(self, dll, syns_dll):
        self._dll, self._syns = dll, syns_dll

    def point_cloud_scratch_ints(self, n, max_h, max_w, stride):
        return self._dll.hp_point_cloud_scratch_ints(n, max_h, max_w, stride)

    def syns_scratch_ints(self, n, px_stride):
        return self._syns.hp_syns_scratch_ints(n, px_stride)


class CloudPortBackend:
    name = "cloud-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())
        self.syns_dll = ctypes.CDLL(syns_port.build())
        self.compare_dll = ctypes.CDLL(compare_port.build())
        self.postproc_dll = ctypes.CDLL(postproc_port.build())
        self.lib = _Sizes(self.dll, self.syns_dll)

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def _dll_for(self, name):
        if name in CLOUD_CALLS:
            return self.dll
        if name == "bbd_depth_metrics":
            return self.compare_dll
        if name == "bbd_post_process_disp":
            return self.postproc_dll
        return self.syns_dll

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
        return call_port(self._dll_for(name), name, args)

    def run(self, name, anchor, *args):
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
