"""CPU tier: the plumbing of the ResNet shortcut convolution on fp32 MFMA (ops.conv1x1_s2, ops.block_entry,
ops.CONV1X1_ROUTES, ops.FUSED_CONV1X1; include/bbd_hip.h, bbd_conv1x1s2_*) and the host walk of its index arithmetic under
the sanitizers (tests/sanitize/conv1x1_index_main.cpp).  The kernels themselves: tests/test_gpu_conv1x1.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# N, C, K, H, W: the shapes of tests/test_gpu_conv1x1.py
SMALL = [(1, 16, 16, 2, 2), (2, 16, 32, 5, 7), (3, 32, 16, 6, 34), (2, 64, 128, 8, 40), (1, 256, 512, 6, 20)]
# the six shortcuts of an MD2 step
MD2 = [(N, C, 2 * C, H, W) for N in (12, 24) for C, H, W in ((64, 48, 160), (128, 24, 80), (256, 12, 40))]
REFUSED = [(2, 8, 16, 8, 8), (2, 16, 8, 8, 8), (2, 24, 16, 8, 8), (2, 16, 40, 8, 8), (2, 0, 16, 8, 8), (0, 16, 16, 8, 8),
           (2, 16, 16, 0, 8), (2, 16, 16, 8, 0), (-1, 16, 16, 8, 8), (2, 16, 16, 46341, 46341), (1 << 20, 64, 128, 48, 160),
           (1 << 27, 16, 16, 1, 1), (1, 1 << 16, 1 << 16, 1, 1)]


@pytest.fixture(scope="module")
def lib():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    build()
    return _lib.get_lib()


def _records(C, K):
    blocks = -(-K // 64) * -(-C // 64)
    return 1 if blocks >= 512 else 512 // blocks


def test_abi_constants_and_prototypes(lib):
    from baseboostdepth_amd import _lib
    assert _lib.ABI_VERSION >= 30 and lib.abi_version == _lib.ABI_VERSION and _lib.WGRAD_RUN == 128
    fwd, dgrad, wgrad = (_lib.PROTOTYPES["bbd_conv1x1s2_" + n] for n in ("fwd", "bwd_data", "wgrad"))
    for call in (fwd, dgrad, wgrad):
        assert call.has_stream and call.restype is ctypes.c_int
    assert [n for _, n in fwd.params] == ["x", "w", "y", "N", "C", "K", "H", "W", "stream"]
    assert [n for _, n in dgrad.params] == ["grad_y", "w", "grad_x", "N", "C", "K", "H", "W", "accumulate", "stream"]
    assert [n for _, n in wgrad.params] == ["x", "grad_y", "grad_w", "scratch", "scratch_doubles", "N", "C", "K", "H", "W", "stream"]
    # the two queries: declared in include/bbd_conv1x1.h only, typed from it, bound under their names minus `bbd_`
    assert sorted(_lib.CONV1X1_HELPERS) == ["bbd_conv1x1s2_supported", "bbd_conv1x1s2_wgrad_scratch_doubles"]
    others = (set(_lib.PROTOTYPES) | set(_lib.WGRAD_HELPERS) | set(_lib.UP2CONV_HELPERS) | set(_lib.SGM_HELPERS)
              | set(_lib.STEMCONV_HELPERS))
    assert not set(_lib.CONV1X1_HELPERS) & others
    with open(os.path.join(ROOT, "include", "bbd_hip.h")) as f:
        text = f.read()
    assert "bbd_conv1x1s2_supported(int" not in text and "bbd_conv1x1s2_wgrad_scratch_doubles(int" not in text
    for helper, proto in _lib.CONV1X1_HELPERS.items():
        assert not proto.has_stream and proto.restype is ctypes.c_int
        assert [(t, n) for t, n in proto.params] == [(ctypes.c_int, n) for n in ("N", "C", "K", "H", "W")]
        bound = getattr(lib, helper[len("bbd_"):])
        assert bound.argtypes == [ctypes.c_int] * 5 and bound.restype is ctypes.c_int
    with pytest.raises(ctypes.ArgumentError):
        lib.conv1x1s2_supported(1.0, 16, 16, 4, 4)


def test_supported_scratch_and_the_routing_table_agree(lib):
    from baseboostdepth_amd import ops
    for N, C, K, H, W in SMALL + MD2 + [(236, 256, 512, 12, 40), (1, 48, 80, 1, 1)]:
        assert lib.conv1x1s2_supported(N, C, K, H, W) == 1
        # one [K][C] record of doubles per split; the number of splits depends on K and C only
        assert lib.conv1x1s2_wgrad_scratch_doubles(N, C, K, H, W) == _records(C, K) * K * C
    for shape in REFUSED:
        assert lib.conv1x1s2_supported(*shape) == 0 and lib.conv1x1s2_wgrad_scratch_doubles(*shape) == 0, shape
    # every row of the table is a direction of one of the step's shortcut shapes, which the calls take at any batch
    assert all(len(row) == 5 and row[4] in ("fwd", "dgrad", "wgrad") for row in ops.CONV1X1_ROUTES)
    assert {row[:4] for row in ops.CONV1X1_ROUTES} <= {(C, K, H, W) for _, C, K, H, W in MD2}
    for C, K, H, W, _ in ops.CONV1X1_ROUTES:
        for N in (1, 12, 24, 236):
            assert lib.conv1x1s2_supported(N, C, K, H, W) == 1
    assert ops.BLOCK_ENTRY_ROUTES <= {row[:4] for row in ops.CONV1X1_ROUTES if row[4] == "dgrad"}
    # no row may fire at the sizes whose launch lists tests/test_gpu_network_routes.py pins
    assert not [row for row in ops.CONV1X1_ROUTES if (row[2], row[3]) in ((16, 32), (8, 16), (4, 8), (32, 64), (16, 32), (8, 16))]


def test_the_calls_refuse_bad_arguments_before_any_launch(lib):
    """NULL pointers, refused shapes and a short scratch return BBD_E_BADARG; nothing is launched (no GPU is needed to ask)."""
    from baseboostdepth_amd import _lib
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    dll = lib._dll
    assert dll.bbd_conv1x1s2_fwd(null, one, one, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    assert dll.bbd_conv1x1s2_fwd(one, one, null, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    assert dll.bbd_conv1x1s2_bwd_data(one, null, one, 1, 16, 16, 4, 4, 0, null) == _lib.E_BADARG
    assert dll.bbd_conv1x1s2_bwd_data(one, one, null, 1, 16, 16, 4, 4, 1, null) == _lib.E_BADARG
    need = lib.conv1x1s2_wgrad_scratch_doubles(1, 16, 16, 4, 4)
    assert dll.bbd_conv1x1s2_wgrad(one, one, one, null, need, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    assert dll.bbd_conv1x1s2_wgrad(one, one, one, one, need - 1, 1, 16, 16, 4, 4, null) == _lib.E_BADARG
    for N, C, K, H, W in REFUSED:
        assert dll.bbd_conv1x1s2_fwd(one, one, one, N, C, K, H, W, null) == _lib.E_BADARG
        assert dll.bbd_conv1x1s2_bwd_data(one, one, one, N, C, K, H, W, 0, null) == _lib.E_BADARG
        assert dll.bbd_conv1x1s2_wgrad(one, one, one, one, 1 << 30, N, C, K, H, W, null) == _lib.E_BADARG


def test_host_tensors_are_never_routed_and_the_module_keeps_its_keys(lib, monkeypatch):
    from baseboostdepth_amd import ops, _lib, networks
    monkeypatch.setattr(ops, "CONV1X1_ROUTES", {(64, 128, 16, 32, d) for d in ("fwd", "dgrad", "wgrad")})
    x, w = torch.rand(1, 64, 16, 32), torch.randn(128, 64, 1, 1)
    assert ops.conv1x1s2_shape(x, w) is None
    assert not any(ops.conv1x1s2_routed(x, w, d) for d in ("fwd", "dgrad", "wgrad"))
    with pytest.raises(_lib.BbdError):
        ops.conv1x1s2_fwd(x, w)
    with pytest.raises(_lib.BbdError):
        ops.conv1x1s2_bwd_data(torch.randn(1, 128, 8, 16), w, x.shape)
    with pytest.raises(_lib.BbdError):
        ops.conv1x1s2_wgrad(x, w, torch.randn(1, 128, 8, 16))
    # the state-dict keys of an encoder are what they were, and on the host a block computes what its modules compute
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False).eval()
    keys = list(enc.state_dict())
    for layer in (2, 3, 4):
        for key in ("downsample.0.weight", "downsample.1.weight", "downsample.1.bias", "downsample.1.running_mean",
                    "downsample.1.running_var", "downsample.1.num_batches_tracked", "conv1.weight"):
            assert "encoder.layer%d.0.%s" % (layer, key) in keys
    assert not [k for k in keys if "downsample.0.bias" in k or "layer1.0.downsample" in k]
    block = enc.encoder.layer2[0]
    f1 = torch.rand(1, 64, 16, 32)
    with torch.no_grad():
        out, identity = block._entry(f1)
        assert torch.equal(out, block.conv1(f1)) and torch.equal(identity, block.downsample(f1))


def test_the_module_side_conditions():
    from baseboostdepth_amd.networks import encoder
    ok = nn.Conv2d(64, 128, 1, 2, bias=False)
    assert encoder._plain_conv(ok, 1, 2, 0)
    assert not encoder._plain_conv(nn.Conv2d(64, 128, 1, 1, bias=False), 1, 2, 0)            # stride 1
    assert not encoder._plain_conv(nn.Conv2d(64, 128, 1, 2, bias=True), 1, 2, 0)             # a bias
    assert not encoder._plain_conv(nn.Conv2d(64, 128, 3, 2, 1, bias=False), 1, 2, 0)         # another kernel
    assert not encoder._plain_conv(nn.Conv2d(64, 128, 1, 2, 1, bias=False), 1, 2, 0)         # padding
    assert not encoder._plain_conv(nn.Conv2d(64, 128, 1, 2, groups=2, bias=False), 1, 2, 0)  # groups
    assert not encoder._plain_conv(None, 1, 2, 0)
    assert encoder._plain_conv(nn.Conv2d(64, 128, 3, 2, 1, bias=False), 3, 2, 1)


def test_the_switch_is_read_from_the_environment():
    code = "from baseboostdepth_amd import ops; print(int(ops.FUSED_CONV1X1))"
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "BBD_FUSED_CONV1X1"}
        if value is not None:
            env["BBD_FUSED_CONV1X1"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_each_switch_the_table_and_the_tensor_kind_turn_routing_off(monkeypatch):
    from baseboostdepth_amd import ops

    class Fake:                                                  # what conv1x1s2_routed asks of a tensor
        def __init__(self, *shape, dtype=torch.float32, contiguous=True, cuda=True):
            self.shape, self.is_cuda, self.dtype, self._contiguous = torch.Size(shape), cuda, dtype, contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._contiguous

    class Backend:
        class lib:
            conv1x1s2_supported = staticmethod(lambda N, C, K, H, W: int(C % 16 == 0 and K % 16 == 0))

    x, w = Fake(24, 64, 48, 160), Fake(128, 64, 1, 1)
    assert ops.conv1x1s2_shape(x, w) == (24, 64, 128, 48, 160)
    for switch in ("FUSED_CONV1X1", "FUSED_NN"):
        monkeypatch.setattr(ops, switch, True)
    monkeypatch.setattr(ops, "CONV1X1_ROUTES", {(64, 128, 48, 160, "fwd"), (64, 128, 48, 160, "dgrad"), (24, 40, 48, 160, "fwd")})
    assert ops.conv1x1s2_routed(x, w, "fwd", Backend) and ops.conv1x1s2_routed(x, w, "dgrad", Backend)
    assert not ops.conv1x1s2_routed(x, w, "wgrad", Backend)                                # not in the table
    monkeypatch.setattr(ops, "BLOCK_ENTRY_ROUTES", {(64, 128, 48, 160), (24, 40, 48, 160)})
    assert ops.block_entry_routed(x, w, Backend) and not ops.block_entry_routed(Fake(24, 24, 48, 160), Fake(40, 24, 1, 1), Backend)
    with monkeypatch.context() as m:
        m.setattr(ops, "BLOCK_ENTRY_ROUTES", set())
        assert not ops.block_entry_routed(x, w, Backend)
    with monkeypatch.context() as m:                                                       # not without the data gradient's row
        m.setattr(ops, "CONV1X1_ROUTES", {(64, 128, 48, 160, "fwd")})
        assert not ops.block_entry_routed(x, w, Backend)
    assert ops.conv1x1s2_routed(Fake(1, 64, 48, 160), w, "fwd", Backend)                   # any batch
    assert not ops.conv1x1s2_routed(Fake(24, 64, 24, 80), w, "fwd", Backend)               # supported, not measured
    assert not ops.conv1x1s2_routed(Fake(24, 24, 48, 160), Fake(40, 24, 1, 1), "fwd", Backend)     # in the table, not supported
    assert not ops.conv1x1s2_routed(Fake(24, 64, 48, 160, contiguous=False), w, "fwd", Backend)    # channels-last
    assert not ops.conv1x1s2_routed(Fake(24, 64, 48, 160, dtype=torch.float16), w, "fwd", Backend)
    assert not ops.conv1x1s2_routed(Fake(24, 64, 48, 160, cuda=False), w, "fwd", Backend)
    assert not ops.conv1x1s2_routed(x, Fake(128, 32, 1, 1), "fwd", Backend)                # the weight is for other channels
    assert not ops.conv1x1s2_routed(x, Fake(128, 64, 3, 3), "fwd", Backend)                # not a 1x1 kernel
    assert not ops.conv1x1s2_routed(Fake(0, 64, 48, 160), w, "fwd", Backend)               # empty
    assert ops.conv1x1s2_shape(Fake(64, 48, 160), w) is None
    # a channels-last activation is not contiguous in the sense the predicate asks
    assert not torch.rand(2, 64, 8, 8).to(memory_format=torch.channels_last).is_contiguous()
    for switch in ("FUSED_CONV1X1", "FUSED_NN"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            assert not any(ops.conv1x1s2_routed(x, w, d, Backend) for d in ("fwd", "dgrad", "wgrad"))
            assert not ops.block_entry_routed(x, w, Backend)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "conv1x1_index_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "conv1x1_index_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_every_address_of_every_launch_is_inside_its_tensor_and_every_element_is_written_once(walk, lib):
    """The stand-alone walk (its own `main`, nothing loaded into Python): addresses, coverage - plain data gradient: every
    element once; accumulate: the even positions only - and the exact result on small integers against the plain loops.
    Its plan is the library's: the same scratch size."""
    shapes = SMALL + [(2, 48, 80, 7, 9)]                         # ... and one with C and K no multiples of 64
    args = [str(v) for shape in shapes for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([walk] + args, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, (done.stdout[-2000:],
                                                                                                        done.stderr[-2000:])
    lines = done.stdout.strip().splitlines()
    assert len(lines) == len(shapes) and all(line.endswith(": ok") for line in lines)
    for (N, C, K, H, W), line in zip(shapes, lines):
        assert line.startswith("%d %d %d %d %d: " % (N, C, K, H, W))
        assert "%d scratch doubles" % lib.conv1x1s2_wgrad_scratch_doubles(N, C, K, H, W) in line
    assert "3 tiles, 10 strips" in lines[2] and "16 splits of 1" in lines[4]
