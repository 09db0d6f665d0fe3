"""CPU tier: the plumbing of the ConvBlock weight gradient from the NCHW tensors (ops.conv3x3_wgrad, ops.WGRAD_ROUTES,
ops.FUSED_WGRAD; include/bbd_hip.h, bbd_conv3x3_wgrad*) and the host walk of its index arithmetic under the sanitizers
(tests/sanitize/wgrad_index_main.cpp).  The kernels themselves: tests/test_gpu_conv_wgrad.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# N, C, K, H, W: the shapes of tests/test_gpu_conv_wgrad.py
SMALL = [(1, 16, 16, 1, 4), (2, 16, 16, 3, 16), (1, 16, 16, 2, 18), (3, 32, 16, 5, 36), (2, 64, 32, 4, 40), (1, 96, 32, 6, 20),
         (2, 16, 16, 48, 160), (2, 32, 16, 7, 50)]
MD2 = [(12, 16, 16, 192, 640), (12, 32, 16, 96, 320), (12, 64, 32, 48, 160), (12, 96, 32, 96, 320)]


@pytest.fixture(scope="module")
def lib():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    build()
    return _lib.get_lib()


def test_abi_constants_and_prototypes(lib):
    from baseboostdepth_amd import _lib
    assert _lib.ABI_VERSION >= 24 and lib.abi_version == _lib.ABI_VERSION
    assert _lib.WGRAD_RUN % 16 == 0 and 16 <= _lib.WGRAD_RUN <= 1024       # whole strips; a chain short enough to bound
    call = _lib.PROTOTYPES["bbd_conv3x3_wgrad"]
    assert call.has_stream and call.restype is ctypes.c_int
    assert [n for _, n in call.params] == ["xp", "grad_z", "grad_w", "scratch", "N", "C", "K", "H", "W", "stream"]
    # the two queries: declared in include/bbd_wgrad.h, typed from it, bound under their names minus `bbd_`
    assert sorted(_lib.WGRAD_HELPERS) == ["bbd_conv3x3_wgrad_scratch_doubles", "bbd_conv3x3_wgrad_supported"]
    assert not set(_lib.WGRAD_HELPERS) & set(_lib.PROTOTYPES)
    for helper, proto in _lib.WGRAD_HELPERS.items():
        assert not proto.has_stream and proto.restype is ctypes.c_int
        assert [(t, n) for t, n in proto.params] == [(ctypes.c_int, n) for n in ("N", "C", "K", "H", "W")]
        bound = getattr(lib, helper[len("bbd_"):])
        assert bound.argtypes == [ctypes.c_int] * 5 and bound.restype is ctypes.c_int
    with pytest.raises(ctypes.ArgumentError):
        lib.conv3x3_wgrad_supported(1.0, 16, 16, 4, 4)


def test_supported_scratch_and_the_routing_table_agree(lib):
    from baseboostdepth_amd import ops
    for shape in SMALL + MD2:
        N, C, K, H, W = shape
        assert lib.conv3x3_wgrad_supported(*shape) == 1
        doubles = lib.conv3x3_wgrad_scratch_doubles(*shape)
        # whole records of one double per weight, and no more of them than workgroups that find 12 strips per wave
        assert doubles % (9 * C * K) == 0 and 1 <= doubles // (9 * C * K) <= max(1, -(-N * H * -(-W // 16) // 96))
    for shape in ((1, 24, 16, 4, 4), (1, 16, 8, 4, 4), (1, 16, 16, 0, 4), (1, 16, 16, 4, 0), (0, 16, 16, 4, 4),
                  (1, 2048, 16, 4, 4), (1, 16, 16, 46341, 46341)):
        assert lib.conv3x3_wgrad_supported(*shape) == 0 and lib.conv3x3_wgrad_scratch_doubles(*shape) == 0
    # every row of the table is a shape the call takes, at the measured batch and at batch 1
    assert ops.WGRAD_ROUTES and all(len(row) == 4 for row in ops.WGRAD_ROUTES)
    for C, K, H, W in ops.WGRAD_ROUTES:
        assert lib.conv3x3_wgrad_supported(12, C, K, H, W) == 1 and lib.conv3x3_wgrad_supported(1, C, K, H, W) == 1
    assert {(16, 16, 192, 640), (32, 16, 96, 320)} <= set(ops.WGRAD_ROUTES)
    assert (96, 32, 96, 320) not in ops.WGRAD_ROUTES             # supported, measured slower than MIOpen


def test_host_tensors_are_never_routed_and_the_call_refuses_them(lib):
    from baseboostdepth_amd import ops, _lib, layers
    xp, w = torch.randn(1, 16, 194, 642), torch.randn(16, 16, 3, 3)
    assert ops.conv3x3_wgrad_shape(xp, w) is None and not ops.conv3x3_wgrad_routed(xp, w)
    assert ops.conv3x3_wgrad_shape(torch.empty(0, device="meta"), w) is None
    with pytest.raises(_lib.BbdError):
        ops.conv3x3_wgrad(xp, torch.randn(1, 16, 192, 640))
    block = layers.ConvBlock(16, 16)
    small = torch.randn(1, 16, 6, 6, requires_grad=True)
    block.conv_raw(small).sum().backward()                       # today's line
    assert block.conv.conv.weight.grad is not None


def test_the_switch_is_read_from_the_environment():
    code = "from baseboostdepth_amd import ops; print(int(ops.FUSED_WGRAD))"
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "BBD_FUSED_WGRAD"}
        if value is not None:
            env["BBD_FUSED_WGRAD"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_the_switch_and_the_glue_switch_turn_routing_off(monkeypatch):
    from baseboostdepth_amd import ops

    class Fake:                                                  # what conv3x3_wgrad_routed asks of a tensor
        def __init__(self, *shape):
            self.shape, self.is_cuda, self.dtype = torch.Size(shape), True, torch.float32

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True

    class Backend:
        class lib:
            conv3x3_wgrad_supported = staticmethod(lambda *a: 1)

    xp, w = Fake(12, 16, 194, 642), Fake(16, 16, 3, 3)
    assert ops.conv3x3_wgrad_shape(xp, w) == (12, 16, 16, 192, 640)
    monkeypatch.setattr(ops, "FUSED_WGRAD", True)
    monkeypatch.setattr(ops, "FUSED_NN", True)
    assert ops.conv3x3_wgrad_routed(xp, w, Backend)
    assert not ops.conv3x3_wgrad_routed(Fake(12, 16, 98, 322), w, Backend)             # supported, not measured
    assert not ops.conv3x3_wgrad_routed(xp, Fake(16, 16, 1, 1), Backend)
    for switch in ("FUSED_WGRAD", "FUSED_NN"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            assert not ops.conv3x3_wgrad_routed(xp, w, Backend)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "wgrad_index_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "wgrad_index_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_every_offset_of_a_launch_is_inside_its_tensor_and_every_pixel_is_taken_once(walk, lib):
    """The stand-alone walk (its own `main`, nothing loaded into Python): offsets, coverage, and the exact result on small
    integers for the shapes of the GPU tier.  Its plan is the library's: the same scratch size."""
    args = [str(v) for shape in SMALL for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([walk] + args, env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    lines = done.stdout.strip().splitlines()
    assert len(lines) == len(SMALL) and all(line.endswith(": ok") for line in lines)
    for shape, line in zip(SMALL, lines):
        assert "%d scratch doubles" % lib.conv3x3_wgrad_scratch_doubles(*shape) in line
    assert "10 groups, 12 strips per wave" in lines[6]           # more than one workgroup, and 12 > RUN / 16 = 8: two runs
