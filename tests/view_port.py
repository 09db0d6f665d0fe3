"""Build + bind the host port of the view rasteriser (tests/host_port/bbd_view_port.cpp).

Test infrastructure only, in the manner of tests/map_port.py: `ViewPortBackend` plugs into the `backend=` seam of
`ops.view_*` / `pointcloud.Canvas`, so the CPU tier runs the product's Python plumbing (canvas allocation, checks, view
matrices, the read-back) with the exact arithmetic of bbd_view.hip (bbd_view_math.h).  It IS a `MapPortBackend`, so
that `evaluation.evaluate_pose(..., save_map=, save_plot=)` runs whole on the host, and `bbd_point_cloud` goes to the
port of tests/cloud_port.py, so that `test_simple.py --cloud_view` does."""
import ctypes

from port_build import build_port, call_port
import cloud_port
from map_port import MapPortBackend

VIEW_CALLS = ("bbd_view_clear", "bbd_view_points", "bbd_view_lines", "bbd_view_resolve")


def build():
    return build_port("libbbd_view_port.so", ["bbd_view_port.cpp"])


class _Sizes:
    """The size helpers of the map port and of the cloud port under one roof."""

    def __init__(self, *parts):
        self._parts = parts

    def __getattr__(self, name):
        for part in self._parts:
            if hasattr(part, name):
                return getattr(part, name)
        raise AttributeError(name)


class ViewPortBackend(MapPortBackend):
    name = "view-host-port"

    def __init__(self):
        super().__init__()
        self.view_dll = ctypes.CDLL(build())
        self.cloud = cloud_port.CloudPortBackend()
        self.lib = _Sizes(self.lib, self.cloud.lib)

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
        if name in VIEW_CALLS:
            return call_port(self.view_dll, name, args)
        if name in cloud_port.CLOUD_CALLS:
            return self.cloud.status(name, *args)
        return super().status(name, *args)
