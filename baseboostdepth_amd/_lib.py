"""ctypes binding of the C-ABI shared library (include/bbd_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `baseboostdepth_amd/csrc/build.py`
(`hipcc --offload-arch=gfx950`).  There is NO fallback: if the library is missing or a call
fails, a RuntimeError is raised - the product path never silently runs anything else.
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported first: it owns the process's libamdhip64.so)

from . import _abi
from ._abi import BbdError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# BBD_HIP_LIB lets the tuning scripts load an alternative build of the SAME sources (tools/variants.sh)
LIB_PATH = os.environ.get("BBD_HIP_LIB", os.path.join(_HERE, "csrc", "libbbd_hip.so"))

# Every prototype and every `#define BBD_<NAME> <integer>` of include/bbd_hip.h (`_abi.py` reads the header; nothing about
# the ABI is written down a second time here): SIGNATURES = name -> argtypes, `void* stream` included, and each constant
# under its name without the prefix - POSE_STRIDE, EVAL_DESC, CLOUD_VERTEX, ABI_VERSION, ...
PROTOTYPES, CONSTANTS = _abi.read_header()
SIGNATURES = {name: [ctype for ctype, _ in proto.params] for name, proto in PROTOTYPES.items()}
globals().update(CONSTANTS)
TRAJ_MODES = {mode.lower(): CONSTANTS["TRAJ_" + mode] for mode in ("SIM3", "SE3", "SCALE", "NONE")}
# the host-side queries of bbd_conv3x3_wgrad have a header of their own (include/bbd_wgrad.h says why), read the same way
WGRAD_HELPERS, _ = _abi.read_header(os.path.join(os.path.dirname(_abi.HEADER), "bbd_wgrad.h"))
# ... and so have those of bbd_up2conv3x3_fwd / _bwd (include/bbd_up2conv.h)
UP2CONV_HELPERS, _ = _abi.read_header(os.path.join(os.path.dirname(_abi.HEADER), "bbd_up2conv.h"))
# ... and the scratch query of bbd_sgm_hints (include/bbd_sgm.h)
SGM_HELPERS, _ = _abi.read_header(os.path.join(os.path.dirname(_abi.HEADER), "bbd_sgm.h"))
# ... and the two queries of bbd_stem_conv7s2_fwd / _wgrad (include/bbd_stemconv.h)
STEMCONV_HELPERS, _ = _abi.read_header(os.path.join(os.path.dirname(_abi.HEADER), "bbd_stemconv.h"))
# ... and the two queries of bbd_conv1x1s2_fwd / _bwd_data / _wgrad (include/bbd_conv1x1.h)
CONV1X1_HELPERS, _ = _abi.read_header(os.path.join(os.path.dirname(_abi.HEADER), "bbd_conv1x1.h"))


class HipLibrary:
    """Thin typed wrapper; every call checks the int status the ABI returns."""

    def __init__(self, path=LIB_PATH):
        if not os.path.isfile(path):
            raise BbdError(
                "HIP extension %s not found - run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
        self.path = path
        self._dll = ctypes.CDLL(path)
        for name, proto in PROTOTYPES.items():
            fn = getattr(self._dll, name)   # AttributeError here = header/library mismatch
            fn.argtypes, fn.restype = SIGNATURES[name], proto.restype
            if not proto.has_stream:
                # the host-side helpers, under their ABI name minus `bbd_`: lib.num_tiles(H, W), lib.map_state_bytes(T);
                # one without parameters is a constant of the build and is bound as its value: lib.tile_w, lib.smooth_chunks
                setattr(self, name[len("bbd_"):], fn if proto.params else fn())
        for name, proto in list(WGRAD_HELPERS.items()) + list(UP2CONV_HELPERS.items()) + list(SGM_HELPERS.items()) \
                + list(STEMCONV_HELPERS.items()) + list(CONV1X1_HELPERS.items()):
            fn = getattr(self._dll, name)
            fn.argtypes, fn.restype = [ctype for ctype, _ in proto.params], proto.restype
            setattr(self, name[len("bbd_"):], fn)
        # the shorter names the depth-wise weight-gradient helpers had before the binding was read from the header; callers
        # outside the package (tests/test_gpu_vit_f64.py) still use them
        self.dwconv_wgrad_scratch_floats = self.dwconv_tokens_wgrad_scratch_floats
        self.dwconv_groups_wgrad_scratch_floats = self.dwconv_tokens_groups_wgrad_scratch_floats
        if self.abi_version != CONSTANTS["ABI_VERSION"]:
            raise BbdError("libbbd_hip.so ABI version mismatch")

    def call(self, name, *args):
        rc = getattr(self._dll, name)(*args)
        if rc != 0:
            raise BbdError("%s failed with status %d" % (name, rc))

    @staticmethod
    def stream_for(tensor):
        # raw handle of torch's CURRENT stream on the tensor's device (the C accessor: this is on the
        # path of every launch, torch.cuda.current_stream() builds a Python Stream object each time)
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(tensor.get_device()))


_LIB = None


def get_lib():
    global _LIB
    if _LIB is None:
        _LIB = HipLibrary()
    return _LIB


def ptr(t):
    """Device (or host, for the test port) address of a contiguous tensor; None -> NULL."""
    if t is None:
        return ctypes.c_void_p(0)
    assert t.is_contiguous(), "C-ABI tensors must be contiguous"
    return ctypes.c_void_p(t.data_ptr())
