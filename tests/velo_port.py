"""Build + bind the host port of the Velodyne depth maps (tests/host_port/bbd_velo_port.cpp).

Test infrastructure only, in the manner of tests/viz_port.py: `VeloPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.velo_depth` (and of `kitti_utils.generate_depth_maps` above it), so the CPU tier runs the
product's Python plumbing (calibration, descriptor and projection tables, batching, the ragged buffer) with the exact
per-point arithmetic of bbd_velo.hip (bbd_velo_math.h)."""
import ctypes

from port_build import build_port, call_port


def build():
    return build_port("libbbd_velo_port.so", ["bbd_velo_port.cpp"])


class _Sizes:
    def __init__(self, dll):
        self._dll = dll

    def velo_depth_scratch_ints(self, total_pixels, n_frames):
        return self._dll.hp_velo_depth_scratch_ints(total_pixels, n_frames)


class VeloPortBackend:
    name = "velo-host-port"

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
