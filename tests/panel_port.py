"""Build + bind the host port of the training-log panel (tests/host_port/bbd_panel_port.cpp).

Test infrastructure only, in the manner of tests/postproc_port.py: `PanelPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.train_panel` / `argmin_hist`, so the CPU tier runs the product's Python plumbing (descriptor
table, LUT buffer, the trainer's tile layout) with the exact per-pixel arithmetic of bbd_panel.hip (bbd_panel_math.h).
It extends `HostPortBackend`: every other launch goes to the port of the fused kernels, so a whole `Trainer` step and
its log run on the host."""
import ctypes

from host_port import HostPortBackend
from port_build import build_port, call_port

PANEL_CALLS = ("bbd_train_panel", "bbd_argmin_hist")


def build():
    return build_port("libbbd_panel_port.so", ["bbd_panel_port.cpp"])


class _Sizes:
    def __init__(self, dll):
        self._dll = dll

    def train_panel_scratch_ints(self, n_tiles):
        return self._dll.hp_train_panel_scratch_ints(n_tiles)


class PanelPortBackend(HostPortBackend):
    name = "panel-host-port"

    def __init__(self):
        super().__init__()
        self.panel_dll = ctypes.CDLL(build())
        self.lib = _Sizes(self.panel_dll)

    def status(self, name, *args):
        """The port's return code (0 = done, < 0 = the ABI's argument errors)."""
        return call_port(self.panel_dll, name, args)

    def run(self, name, anchor, *args):
        if name not in PANEL_CALLS:
            return super().run(name, anchor, *args)
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
