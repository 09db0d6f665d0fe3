"""Build + bind the host port of the colour-mapped disparity (tests/host_port/bbd_viz_port.cpp).

Test infrastructure only, in the manner of tests/host_port.py: `VizPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.disp_viz`, so the CPU tier runs the product's Python plumbing (descriptor table, ragged views,
LUT) with the exact per-pixel arithmetic of bbd_viz.hip (bbd_viz_math.h)."""
import ctypes

from port_build import build_port, call_port


def build():
    return build_port("libbbd_viz_port.so", ["bbd_viz_port.cpp"])


class _Sizes:
    def __init__(self, dll):
        self._dll = dll

    def disp_viz_scratch_ints(self, n):
        return self._dll.hp_disp_viz_scratch_ints(n)


class VizPortBackend:
    name = "viz-host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())
        self.lib = _Sizes(self.dll)

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def run(self, name, anchor, *args):
        rc = call_port(self.dll, name, args)
        assert rc == 0, (name, rc)
