"""CPU tier: the plumbing of the finest decoder level's up-sample + pad + 3x3 convolution in sub-pixel form
(ops.up2_conv3x3, ops.UP2CONV_ROUTES, ops.FUSED_UP2CONV; include/bbd_hip.h, bbd_up2conv3x3_*) and the host walk of its
index arithmetic under the sanitizers (tests/sanitize/up2conv_index_main.cpp).  The kernels themselves:
tests/test_gpu_up2conv.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# N, h, w: the shapes of tests/test_gpu_up2conv.py (the last one: one source pixel past the 8 x 32 forward tile each way)
SMALL = [(1, 1, 1), (1, 1, 2), (2, 2, 3), (1, 3, 17), (2, 5, 33), (2, 17, 40), (1, 9, 33)]
MD2 = [(12, 96, 320), (1, 96, 320)]
REFUSED = [(1, 24, 16, 4, 4), (1, 16, 8, 4, 4), (1, 16, 16, 0, 4), (1, 16, 16, 4, 0), (0, 16, 16, 4, 4), (1, 32, 32, 4, 4),
           (1, 16, 16, 46341, 46341)]


@pytest.fixture(scope="module")
def lib():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    build()
    return _lib.get_lib()


def test_abi_constants_and_prototypes(lib):
    from baseboostdepth_amd import _lib
    assert _lib.ABI_VERSION >= 26 and lib.abi_version == _lib.ABI_VERSION
    assert 64 < _lib.UP2CONV_ROUNDINGS <= 152                    # more than the 64 products of a chain, no more than nine taps'
    fwd, bwd = _lib.PROTOTYPES["bbd_up2conv3x3_fwd"], _lib.PROTOTYPES["bbd_up2conv3x3_bwd"]
    for call in (fwd, bwd):
        assert call.has_stream and call.restype is ctypes.c_int
    assert [n for _, n in fwd.params] == ["z", "bias", "w", "out", "N", "C", "K", "h", "w_", "stream"]
    assert [n for _, n in bwd.params] == ["grad_out", "z", "bias", "w", "grad_z", "grad_bias", "scratch", "scratch_doubles",
                                          "N", "C", "K", "h", "w_", "stream"]
    # the two queries: declared in include/bbd_up2conv.h only, typed from it, bound under their names minus `bbd_`
    assert sorted(_lib.UP2CONV_HELPERS) == ["bbd_up2conv3x3_scratch_doubles", "bbd_up2conv3x3_supported"]
    assert not set(_lib.UP2CONV_HELPERS) & set(_lib.PROTOTYPES) and not set(_lib.UP2CONV_HELPERS) & set(_lib.WGRAD_HELPERS)
    with open(os.path.join(ROOT, "include", "bbd_hip.h")) as f:
        text = f.read()
    assert "bbd_up2conv3x3_supported(int" not in text and "bbd_up2conv3x3_scratch_doubles(int" not in text
    for helper, proto in _lib.UP2CONV_HELPERS.items():
        assert not proto.has_stream and proto.restype is ctypes.c_int
        assert [(t, n) for t, n in proto.params] == [(ctypes.c_int, n) for n in ("N", "C", "K", "h", "w")]
        bound = getattr(lib, helper[len("bbd_"):])
        assert bound.argtypes == [ctypes.c_int] * 5 and bound.restype is ctypes.c_int
    with pytest.raises(ctypes.ArgumentError):
        lib.up2conv3x3_supported(1.0, 16, 16, 4, 4)


def test_supported_scratch_and_the_routing_table_agree(lib):
    from baseboostdepth_amd import ops
    for N, h, w in SMALL + MD2:
        assert lib.up2conv3x3_supported(N, 16, 16, h, w) == 1
        assert lib.up2conv3x3_scratch_doubles(N, 16, 16, h, w) == 16 * N * h     # one per channel and source row
    for shape in REFUSED:
        assert lib.up2conv3x3_supported(*shape) == 0 and lib.up2conv3x3_scratch_doubles(*shape) == 0
    # every row of the table is a shape the calls take, at the measured batch and at batch 1
    assert all(len(row) == 4 for row in ops.UP2CONV_ROUTES)
    for C, K, h, w in ops.UP2CONV_ROUTES:
        assert lib.up2conv3x3_supported(12, C, K, h, w) == 1 and lib.up2conv3x3_supported(1, C, K, h, w) == 1
    assert set(ops.UP2CONV_ROUTES) <= {(16, 16, 96, 320)}


def test_the_calls_refuse_bad_arguments_before_any_launch(lib):
    """NULL pointers, refused shapes and a short scratch return BBD_E_BADARG; nothing is launched (no GPU is needed to ask)."""
    from baseboostdepth_amd import _lib
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert lib._dll.bbd_up2conv3x3_fwd(null, one, one, one, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    assert lib._dll.bbd_up2conv3x3_bwd(one, one, one, one, one, one, null, 64, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    assert lib._dll.bbd_up2conv3x3_bwd(one, one, one, one, one, one, one, 63, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    for N, C, K, h, w in REFUSED:
        assert lib._dll.bbd_up2conv3x3_fwd(one, one, one, one, N, C, K, h, w, null) == _lib.E_BADARG
        assert lib._dll.bbd_up2conv3x3_bwd(one, one, one, one, one, one, one, 1 << 30, N, C, K, h, w, null) == _lib.E_BADARG


def test_host_tensors_are_never_routed_and_the_call_refuses_them(lib):
    from baseboostdepth_amd import ops, _lib
    z, bias, w = torch.randn(1, 16, 96, 320), torch.randn(16), torch.randn(16, 16, 3, 3)
    assert ops.up2_conv3x3_shape(z, bias, w) is None and not ops.up2_conv3x3_routed(z, bias, w)
    with pytest.raises(_lib.BbdError):
        ops.up2_conv3x3(z, bias, w)


def test_the_switch_is_read_from_the_environment():
    code = "from baseboostdepth_amd import ops; print(int(ops.FUSED_UP2CONV))"
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "BBD_FUSED_UP2CONV"}
        if value is not None:
            env["BBD_FUSED_UP2CONV"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_each_of_the_three_switches_turns_routing_off(monkeypatch):
    from baseboostdepth_amd import ops

    class Fake:                                                  # what up2_conv3x3_routed asks of a tensor
        def __init__(self, *shape, dtype=torch.float32, contiguous=True):
            self.shape, self.is_cuda, self.dtype, self._contiguous = torch.Size(shape), True, dtype, contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._contiguous

    class Backend:
        class lib:
            up2conv3x3_supported = staticmethod(lambda *a: 1)

    z, bias, w = Fake(12, 16, 96, 320), Fake(16), Fake(16, 16, 3, 3)
    assert ops.up2_conv3x3_shape(z, bias, w) == (12, 16, 16, 96, 320)
    for switch in ("FUSED_UP2CONV", "FUSED_NN", "FUSED_DECODER_GLUE"):
        monkeypatch.setattr(ops, switch, True)
    monkeypatch.setattr(ops, "UP2CONV_ROUTES", {(16, 16, 96, 320)})
    assert ops.up2_conv3x3_routed(z, bias, w, Backend)
    assert ops.up2_conv3x3_routed(Fake(1, 16, 96, 320), bias, w, Backend)                 # any batch
    assert not ops.up2_conv3x3_routed(Fake(12, 16, 48, 160), bias, w, Backend)            # supported, not measured
    assert not ops.up2_conv3x3_routed(Fake(12, 16, 96, 320, contiguous=False), bias, w, Backend)
    assert not ops.up2_conv3x3_routed(Fake(12, 16, 96, 320, dtype=torch.float16), bias, w, Backend)
    assert not ops.up2_conv3x3_routed(z, None, w, Backend)
    assert not ops.up2_conv3x3_routed(z, bias, Fake(16, 16, 1, 1), Backend)
    for switch in ("FUSED_UP2CONV", "FUSED_NN", "FUSED_DECODER_GLUE"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            assert not ops.up2_conv3x3_routed(z, bias, w, Backend)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "up2conv_index_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "up2conv_index_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_every_address_of_both_launches_is_inside_its_tensor_and_every_element_is_written_once(walk, lib):
    """The stand-alone walk (its own `main`, nothing loaded into Python): addresses, coverage, and for the small shapes the
    exact result on small integers against the plain loops.  Its plan is the library's: the same scratch size."""
    shapes = SMALL + MD2
    args = [str(v) for shape in shapes for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([walk] + args, env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    lines = done.stdout.strip().splitlines()
    assert len(lines) == len(shapes) and all(line.endswith(": ok") for line in lines)
    for (N, h, w), line in zip(shapes, lines):
        assert "%d scratch doubles" % lib.up2conv3x3_scratch_doubles(N, 16, 16, h, w) in line
        assert ("values compared" in line) == ((N, h, w) in SMALL)
    assert "4 tiles, 9 groups" in lines[6] and "1440 tiles, 1152 groups" in lines[7]
