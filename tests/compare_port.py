"""Build + bind the host port of the comparison-sheet kernels (tests/host_port/bbd_compare_port.cpp).

Test infrastructure only, in the manner of tests/viz_port.py: `ComparePortBackend` plugs into the `backend=` seam of
`ops.gt_viz`, `ops.error_map` and `evaluation.depth_metrics`, so the CPU tier runs the product's Python plumbing
(descriptor rows, ragged views, the shifted base of a batch) with the exact per-pixel arithmetic of bbd_compare.hip
(bbd_compare_math.h).  `bbd_disp_viz` goes to the port of bbd_viz.hip and the image kernels to the port of
bbd_image.hip, so that `compare.compare_batch` runs whole on the host."""
import ctypes

from host_port import HostPortBackend
from port_build import build_port, call_port
import viz_port

COMPARE_CALLS = ("bbd_gt_viz", "bbd_error_map", "bbd_depth_metrics")


def build():
    return build_port("libbbd_compare_port.so", ["bbd_compare_port.cpp"])


class _Sizes:
    def __init__(self, dll, viz_dll):
        self._dll, self._viz = dll, viz_dll

    def gt_viz_scratch_ints(self, n):
        return self._dll.hp_gt_viz_scratch_ints(n)

    def disp_viz_scratch_ints(self, n):
        return self._viz.hp_disp_viz_scratch_ints(n)


class ComparePortBackend(HostPortBackend):
    name = "compare-host-port"

    def __init__(self):
        super().__init__()
        self.compare_dll = ctypes.CDLL(build())
        self.viz = viz_port.VizPortBackend()
        self.lib = _Sizes(self.compare_dll, self.viz.dll)

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
        return call_port(self.compare_dll, name, args)

    def run(self, name, anchor, *args):
        if name == "bbd_disp_viz":
            return self.viz.run(name, anchor, *args)
        if name not in COMPARE_CALLS:
            return super().run(name, anchor, *args)
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
