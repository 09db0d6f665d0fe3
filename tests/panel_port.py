"""Build + bind the host port of the training-log panel (tests/host_port/bbd_panel_port.cpp).

Test infrastructure only, in the manner of tests/postproc_port.py: `PanelPortBackend` plugs into the `backend=` seam of
`baseboostdepth_amd.ops.train_panel` / `argmin_hist`, so the CPU tier runs the product's Python plumbing (descriptor
table, LUT buffer, the trainer's tile layout) with the exact per-pixel arithmetic of bbd_panel.hip (bbd_panel_math.h).
It extends `HostPortBackend`: every other launch goes to the port of the fused kernels, so a whole `Trainer` step and
its log run on the host."""
import ctypes
import os
import subprocess

from host_port import HostPortBackend

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_panel_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_panel_port.so")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bbd_math.h"), os.path.join(CSRC, "bbd_viz_math.h"), os.path.join(CSRC, "bbd_panel_math.h"),
        os.path.join(HERE, "..", "include", "bbd_hip.h")]
PANEL_CALLS = ("bbd_train_panel", "bbd_argmin_hist")


def build():
    if os.path.isfile(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", LIB, SRC]
    subprocess.run(cmd, check=True)
    return LIB


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
        fn = getattr(self.panel_dll, name.replace("bbd_", "hp_"))
        fn.restype = ctypes.c_int
        return fn(*[ctypes.c_int(a) if isinstance(a, int) else a for a in args])

    def run(self, name, anchor, *args):
        if name not in PANEL_CALLS:
            return super().run(name, anchor, *args)
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
