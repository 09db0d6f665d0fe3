"""What every host-port binding (tests/*_port.py) shares: building a port library and calling into it.

Test infrastructure only."""
import ctypes
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PORTS = os.path.join(HERE, "host_port")
CSRC = os.path.join(HERE, "..", "baseboostdepth_amd", "csrc")


def default_headers():
    """Every header a port can reach: a port rebuilds when any of them changes."""
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "bbd_hip.h")]


def build_port(lib_name, sources, headers=None):
    """tests/host_port/<lib_name> from tests/host_port/<sources>, rebuilt when a source or header is newer."""
    lib = os.path.join(PORTS, lib_name)
    srcs = [os.path.join(PORTS, s) for s in sources]
    deps = srcs + (default_headers() if headers is None else list(headers))
    if os.path.isfile(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps):
        return lib
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", lib] + srcs
    subprocess.run(cmd, check=True)
    return lib


def call_port(dll, name, args):
    """Calls the port's twin (hp_*) of the ABI function `name` (bbd_*): Python floats travel as doubles, ints as C ints,
    everything else (ctypes pointers) as it is.  Returns the status code."""
    fn = getattr(dll, name.replace("bbd_", "hp_"))
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
