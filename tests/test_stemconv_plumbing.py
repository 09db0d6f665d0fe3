"""CPU tier: the plumbing of the encoder stems' conv1 on fp32 MFMA (ops.stem_conv, ops.STEMCONV_ROUTES,
ops.FUSED_STEMCONV; include/bbd_hip.h, bbd_stem_conv7s2_*) and the host walk of its index arithmetic under the sanitizers
(tests/sanitize/stemconv_index_main.cpp).  The kernels themselves: tests/test_gpu_stemconv.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "baseboostdepth_amd", "csrc", "bbd_stemconv_math.h")) as _f:
    _TEXT = _f.read()
TH = int(re.search(r"#define BBD_STEM_TH (\d+)", _TEXT).group(1))
TW = int(re.search(r"#define BBD_STEM_TW (\d+)", _TEXT).group(1))
# N, C, H, W: the shapes of tests/test_gpu_stemconv.py
SMALL = [(1, 3, 2, 2), (1, 6, 7, 9), (2, 3, 5, 33), (2, 6, 2 * TH, 2 * TW + 2), (3, 6, 2 * TH + 1, 2 * TW - 1), (2, 3, 32, 64)]
MD2 = [(12, 3, 192, 640), (24, 6, 192, 640)]
# N, C, K, H, W, R, S
REFUSED = [(2, 3, 32, 8, 8, 7, 7), (2, 3, 128, 8, 8, 7, 7), (2, 4, 64, 8, 8, 7, 7), (2, 1, 64, 8, 8, 7, 7), (2, 12, 64, 8, 8, 7, 7),
           (2, 3, 64, 8, 8, 3, 3), (2, 3, 64, 8, 8, 7, 5), (2, 3, 64, 8, 8, 5, 7), (0, 3, 64, 8, 8, 7, 7), (2, 3, 64, 0, 8, 7, 7),
           (2, 3, 64, 8, 0, 7, 7), (2, 3, 64, 46341, 46341, 7, 7), (1 << 20, 6, 64, 192, 640, 7, 7), (1 << 26, 3, 64, 2, 2, 7, 7)]


@pytest.fixture(scope="module")
def lib():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    build()
    return _lib.get_lib()


def test_abi_constants_and_prototypes(lib):
    from baseboostdepth_amd import _lib
    assert _lib.ABI_VERSION >= 29 and lib.abi_version == _lib.ABI_VERSION and _lib.WGRAD_RUN == 128
    fwd, wgrad = _lib.PROTOTYPES["bbd_stem_conv7s2_fwd"], _lib.PROTOTYPES["bbd_stem_conv7s2_wgrad"]
    for call in (fwd, wgrad):
        assert call.has_stream and call.restype is ctypes.c_int
    assert [n for _, n in fwd.params] == ["x", "w", "out", "N", "C", "K", "H", "W", "normalize", "stream"]
    assert [n for _, n in wgrad.params] == ["x", "grad_out", "grad_w", "scratch", "scratch_doubles", "N", "C", "K", "H", "W",
                                            "normalize", "stream"]
    # the two queries: declared in include/bbd_stemconv.h only, typed from it, bound under their names minus `bbd_`
    assert sorted(_lib.STEMCONV_HELPERS) == ["bbd_stem_conv7s2_supported", "bbd_stem_conv7s2_wgrad_scratch_doubles"]
    others = set(_lib.PROTOTYPES) | set(_lib.WGRAD_HELPERS) | set(_lib.UP2CONV_HELPERS) | set(_lib.SGM_HELPERS)
    assert not set(_lib.STEMCONV_HELPERS) & others
    with open(os.path.join(ROOT, "include", "bbd_hip.h")) as f:
        text = f.read()
    assert "bbd_stem_conv7s2_supported(int" not in text and "bbd_stem_conv7s2_wgrad_scratch_doubles(int" not in text
    for helper, proto in _lib.STEMCONV_HELPERS.items():
        assert not proto.has_stream and proto.restype is ctypes.c_int
        assert [(t, n) for t, n in proto.params] == [(ctypes.c_int, n) for n in ("N", "C", "K", "H", "W", "R", "S")]
        bound = getattr(lib, helper[len("bbd_"):])
        assert bound.argtypes == [ctypes.c_int] * 7 and bound.restype is ctypes.c_int
    with pytest.raises(ctypes.ArgumentError):
        lib.stem_conv7s2_supported(1.0, 3, 64, 4, 4, 7, 7)


def test_supported_scratch_and_the_routing_table_agree(lib):
    from baseboostdepth_amd import ops
    for N, C, H, W in SMALL + MD2 + [(236, 6, 192, 640)]:
        assert lib.stem_conv7s2_supported(N, C, 64, H, W, 7, 7) == 1
        tiles = N * (-(-((H + 1) // 2) // TH)) * (-(-((W + 1) // 2) // TW))
        groups = -(-tiles // -(-tiles // min(tiles, 256)))
        # one record of 8 waves x nct column tiles x 256 doubles per workgroup; nct = 5 (C = 3) or 10 (C = 6)
        assert lib.stem_conv7s2_wgrad_scratch_doubles(N, C, 64, H, W, 7, 7) == groups * 8 * (5 if C == 3 else 10) * 256
    for shape in REFUSED:
        assert lib.stem_conv7s2_supported(*shape) == 0 and lib.stem_conv7s2_wgrad_scratch_doubles(*shape) == 0, shape
    # every row of the table is a direction of a shape the calls take, at the measured batches and at batch 1
    assert all(len(row) == 4 and row[3] in ("fwd", "wgrad") for row in ops.STEMCONV_ROUTES)
    for C, H, W, _ in ops.STEMCONV_ROUTES:
        for N in (1, 12, 24):
            assert lib.stem_conv7s2_supported(N, C, 64, H, W, 7, 7) == 1
    assert set(ops.STEMCONV_ROUTES) <= {(C, 192, 640, d) for C in (3, 6) for d in ("fwd", "wgrad")}


def test_the_calls_refuse_bad_arguments_before_any_launch(lib):
    """NULL pointers, refused shapes and a short scratch return BBD_E_BADARG; nothing is launched (no GPU is needed to ask)."""
    from baseboostdepth_amd import _lib
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert lib._dll.bbd_stem_conv7s2_fwd(null, one, one, 1, 3, 64, 4, 4, 0, null) == _lib.E_BADARG
    assert lib._dll.bbd_stem_conv7s2_fwd(one, one, null, 1, 3, 64, 4, 4, 0, null) == _lib.E_BADARG
    need = lib.stem_conv7s2_wgrad_scratch_doubles(1, 3, 64, 4, 4, 7, 7)
    assert lib._dll.bbd_stem_conv7s2_wgrad(one, one, one, null, need, 1, 3, 64, 4, 4, 0, null) == _lib.E_BADARG
    assert lib._dll.bbd_stem_conv7s2_wgrad(one, one, one, one, need - 1, 1, 3, 64, 4, 4, 0, null) == _lib.E_BADARG
    for N, C, K, H, W, R, S in REFUSED:
        if (R, S) == (7, 7):
            assert lib._dll.bbd_stem_conv7s2_fwd(one, one, one, N, C, K, H, W, 0, null) == _lib.E_BADARG
            assert lib._dll.bbd_stem_conv7s2_wgrad(one, one, one, one, 1 << 30, N, C, K, H, W, 0, null) == _lib.E_BADARG


def test_host_tensors_are_never_routed_and_the_calls_refuse_them(lib, monkeypatch):
    from baseboostdepth_amd import ops, _lib
    monkeypatch.setattr(ops, "STEMCONV_ROUTES", {(3, 192, 640, "fwd"), (3, 192, 640, "wgrad")})
    x, w = torch.rand(1, 3, 192, 640), torch.randn(64, 3, 7, 7)
    assert ops.stem_conv_shape(x, w) is None
    assert not ops.stem_conv_routed(x, w, "fwd") and not ops.stem_conv_routed(x, w, "wgrad")
    with pytest.raises(_lib.BbdError):
        ops.stem_conv_fwd(x, w)
    with pytest.raises(_lib.BbdError):
        ops.stem_conv_wgrad(x, w, torch.randn(1, 64, 96, 320))
    # the module keeps its own convolution and the torch normalisation
    from baseboostdepth_amd import networks
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False).eval()
    image = torch.rand(1, 3, 32, 64)
    with torch.no_grad():
        want = enc.encoder.conv1((image - 0.45) / 0.225)
        assert torch.equal(enc._conv1(image, False), want)
        assert torch.equal(enc._conv1((image - 0.45) / 0.225, True), want)


def test_the_switch_is_read_from_the_environment():
    code = "from baseboostdepth_amd import ops; print(int(ops.FUSED_STEMCONV))"
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "BBD_FUSED_STEMCONV"}
        if value is not None:
            env["BBD_FUSED_STEMCONV"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_each_switch_the_table_and_the_tensor_kind_turn_routing_off(monkeypatch):
    from baseboostdepth_amd import ops

    class Fake:                                                  # what stem_conv_routed asks of a tensor
        def __init__(self, *shape, dtype=torch.float32, contiguous=True, cuda=True):
            self.shape, self.is_cuda, self.dtype, self._contiguous = torch.Size(shape), cuda, dtype, contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._contiguous

    class Backend:
        class lib:
            stem_conv7s2_supported = staticmethod(lambda N, C, K, H, W, R, S: int(K == 64 and C in (3, 6) and (R, S) == (7, 7)))

    x, w = Fake(24, 6, 192, 640), Fake(64, 6, 7, 7)
    assert ops.stem_conv_shape(x, w) == (24, 6, 64, 192, 640, 7, 7)
    for switch in ("FUSED_STEMCONV", "FUSED_NN"):
        monkeypatch.setattr(ops, switch, True)
    monkeypatch.setattr(ops, "STEMCONV_ROUTES", {(6, 192, 640, "fwd"), (12, 192, 640, "fwd")})
    assert ops.stem_conv_routed(x, w, "fwd", Backend)
    assert not ops.stem_conv_routed(x, w, "wgrad", Backend)                               # the other direction: not in the table
    assert ops.stem_conv_routed(Fake(1, 6, 192, 640), w, "fwd", Backend)                  # any batch
    assert not ops.stem_conv_routed(Fake(24, 6, 96, 320), w, "fwd", Backend)              # supported, not measured
    assert not ops.stem_conv_routed(Fake(24, 12, 192, 640), Fake(64, 12, 7, 7), "fwd", Backend)    # in the table, not supported
    assert not ops.stem_conv_routed(Fake(24, 6, 192, 640, contiguous=False), w, "fwd", Backend)
    assert not ops.stem_conv_routed(Fake(24, 6, 192, 640, dtype=torch.float16), w, "fwd", Backend)
    assert not ops.stem_conv_routed(Fake(24, 6, 192, 640, cuda=False), w, "fwd", Backend)
    assert not ops.stem_conv_routed(x, Fake(64, 3, 7, 7), "fwd", Backend)                 # the weight is for other channels
    assert not ops.stem_conv_routed(Fake(0, 6, 192, 640), w, "fwd", Backend)              # empty
    assert ops.stem_conv_shape(Fake(6, 192, 640), w) is None
    for switch in ("FUSED_STEMCONV", "FUSED_NN"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            assert not ops.stem_conv_routed(x, w, "fwd", Backend)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "stemconv_index_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "stemconv_index_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_every_address_of_both_calls_is_inside_its_tensor_and_every_element_is_written_once(walk, lib):
    """The stand-alone walk (its own `main`, nothing loaded into Python): addresses, coverage, and for the small shapes the
    exact result on small integers against the plain loops.  Its plan is the library's: the same scratch size."""
    shapes = SMALL + MD2
    args = [str(v) for shape in shapes for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([walk] + args, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    lines = done.stdout.strip().splitlines()
    assert len(lines) == len(shapes) and all(line.endswith(": ok") for line in lines)
    for (N, C, H, W), line in zip(shapes, lines):
        assert "%d scratch doubles" % lib.stem_conv7s2_wgrad_scratch_doubles(N, C, 64, H, W, 7, 7) in line
        assert ("values compared" in line) == ((N, C, H, W) in SMALL)
    assert "4 tiles, 4 groups" in lines[3] and "1440 tiles, 240 groups" in lines[6] and "2880 tiles, 240 groups" in lines[7]
