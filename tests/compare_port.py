"""Build + bind the host port of the comparison-sheet kernels (tests/host_port/bbd_compare_port.cpp).

Test infrastructure only, in the manner of tests/viz_port.py: `ComparePortBackend` plugs into the `backend=` seam of
`ops.gt_viz`, `ops.error_map` and `evaluation.depth_metrics`, so the CPU tier runs the product's Python plumbing
(descriptor rows, ragged views, the shifted base of a batch) with the exact per-pixel arithmetic of bbd_compare.hip
(bbd_compare_math.h).  `bbd_disp_viz` goes to the port of bbd_viz.hip and the image kernels to the port of
bbd_image.hip, so that `compare.compare_batch` runs whole on the host."""
import ctypes
import os
import subprocess

from host_port import HostPortBackend
import viz_port

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_port", "bbd_compare_port.cpp")
LIB = os.path.join(HERE, "host_port", "libbbd_compare_port.so")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, n) for n in ("bbd_math.h", "bbd_viz_math.h", "bbd_panel_math.h", "bbd_eval_math.h",
                                                "bbd_compare_math.h")] + [os.path.join(HERE, "..", "include", "bbd_hip.h")]
COMPARE_CALLS = ("bbd_gt_viz", "bbd_error_map", "bbd_depth_metrics")


def build():
    if os.path.isfile(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", LIB, SRC]
    subprocess.run(cmd, check=True)
    return LIB


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
        fn = getattr(self.compare_dll, name.replace("bbd_", "hp_"))
        fn.restype = ctypes.c_int
        conv = []
        for a in args:
            if isinstance(a, float):
                conv.append(ctypes.c_double(a))
            elif isinstance(a, int):
                conv.append(ctypes.c_int(a))
            else:
                conv.append(a)
        return fn(*conv)

    def run(self, name, anchor, *args):
        if name == "bbd_disp_viz":
            return self.viz.run(name, anchor, *args)
        if name not in COMPARE_CALLS:
            return super().run(name, anchor, *args)
        rc = self.status(name, *args)
        assert rc == 0, (name, rc)
