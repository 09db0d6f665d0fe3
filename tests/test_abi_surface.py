"""CPU tier: the C-ABI library loads (no GPU needed) and exports exactly what include/bbd_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bbd_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|long)\s+(bbd_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from baseboostdepth_amd.csrc.build import build
    return build()


def test_header_declares_the_hot_path_entry_points():
    names = declared_functions()
    for must in ("bbd_identity_loss_fwd", "bbd_warp_ssim_min_fwd", "bbd_warp_ssim_min_bwd",
                 "bbd_disp_to_depth_fwd", "bbd_disp_to_depth_bwd"):
        assert must in names


def test_library_exports_every_declared_symbol(lib_path):
    dll = ctypes.CDLL(lib_path)
    for name in declared_functions():
        assert hasattr(dll, name), "libbbd_hip.so lacks %s" % name


def test_binding_signatures_cover_the_header(lib_path):
    from baseboostdepth_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_functions()
    lib = _lib.get_lib()
    assert lib.tile_w == 64 and lib.tile_h == 16
    assert lib.num_tiles(192, 640) == 120
    assert _lib.POSE_STRIDE == 40 and _lib.MAX_CAND == 20


def test_constants_match_header():
    from baseboostdepth_amd import _lib
    text = open(HEADER).read()
    for macro, val in (("BBD_MAX_FRAME_SLOTS", _lib.MAX_FRAME_SLOTS), ("BBD_MAX_CAND", _lib.MAX_CAND),
                       ("BBD_POSE_STRIDE", _lib.POSE_STRIDE), ("BBD_ABI_VERSION", _lib.ABI_VERSION)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == val


def test_product_refuses_cpu_tensors(lib_path):
    """No CPU fallback: the HIP backend raises on host tensors instead of computing anything."""
    import torch
    from baseboostdepth_amd import ops, _lib
    be = ops.HipBackend()
    with pytest.raises(_lib.BbdError):
        ops.disp_to_depth_fullres(torch.rand(1, 1, 8, 8), 16, 16, 0.1, 100.0, be)


def test_missing_library_is_loud(tmp_path):
    from baseboostdepth_amd import _lib
    with pytest.raises(_lib.BbdError):
        _lib.HipLibrary(str(tmp_path / "nope.so"))


# ------------------------------------------------------------------------------------ the header reader (_abi.py)
C = ctypes
POINTER_SPELLINGS = ("const bbd_cand_t*", "const double*", "const float*", "const int32_t*", "const uint32_t*",
                     "const uint64_t*", "const uint8_t*", "const void*", "const void* const*", "double*", "float*",
                     "int32_t*", "int64_t*", "long long*", "uint32_t*", "uint64_t*", "uint8_t*", "void*", "void* const*")
BY_VALUE = {"int": C.c_int, "long": C.c_long, "unsigned": C.c_uint, "double": C.c_double}
LONG_RESULTS = ["bbd_ground_scale_scratch_floats", "bbd_map_state_bytes", "bbd_dwconv_tokens_wgrad_scratch_floats",
                "bbd_dwconv_tokens_groups_wgrad_scratch_floats", "bbd_token_ln_scratch_floats", "bbd_colsum_scratch_floats",
                "bbd_factor_att_scratch_floats"]


def test_reader_types_every_parameter_spelling_of_the_header():
    from baseboostdepth_amd import _abi
    spellings = list(POINTER_SPELLINGS) + list(BY_VALUE)
    assert len(spellings) == 23
    text = "int bbd_all(%s, void* stream);" % ", ".join("%s a%d" % (s, i) for i, s in enumerate(spellings))
    protos, constants = _abi.parse(text)
    proto = protos["bbd_all"]
    assert constants == {} and list(protos) == ["bbd_all"] and proto.restype is C.c_int and proto.has_stream
    assert [name for _, name in proto.params] == ["a%d" % i for i in range(23)] + ["stream"]
    assert [t for t, _ in proto.params] == [C.c_void_p] * 19 + [C.c_int, C.c_long, C.c_uint, C.c_double] + [C.c_void_p]
    # the pointer star may stand with the name, and a by-value spelling is never mistaken for a pointer
    other = _abi.parse("long bbd_other(const float *x, double *y, long n);")[0]
    assert other["bbd_other"] == _abi.Prototype(C.c_long, ((C.c_void_p, "x"), (C.c_void_p, "y"), (C.c_long, "n")), False)


def test_reader_takes_prototypes_over_several_lines_and_skips_comments():
    from baseboostdepth_amd import _abi
    text = """
    /* int bbd_in_a_comment(int a, void* stream);
     * #define BBD_IN_A_COMMENT 5 */
    #ifndef BBD_HIP_H
    #define BBD_HIP_H
    #include <stdint.h>
    extern "C" {
    typedef struct bbd_cand { int32_t kind; } bbd_cand_t;
    #define BBD_TEN 10            /* a trailing remark */
    #define BBD_HEX 0x100
    #define BBD_NEGATIVE (-1)
    int bbd_nothing(void);
    int bbd_split(const float* x,    /* a remark between parameters */
                  int n,
                  double eps, void* stream);
    long
    bbd_size(int n);
    }
    #endif
    """
    protos, constants = _abi.parse(text)
    assert constants == {"TEN": 10, "HEX": 256, "NEGATIVE": -1}             # the include guard is no constant
    assert list(protos) == ["bbd_nothing", "bbd_split", "bbd_size"]
    assert protos["bbd_nothing"] == _abi.Prototype(C.c_int, (), False)
    assert protos["bbd_split"] == _abi.Prototype(
        C.c_int, ((C.c_void_p, "x"), (C.c_int, "n"), (C.c_double, "eps"), (C.c_void_p, "stream")), True)
    assert protos["bbd_size"] == _abi.Prototype(C.c_long, ((C.c_int, "n"),), False)


@pytest.mark.parametrize("text, names", [
    ("int bbd_f(const float* a, float x, void* stream);", ("bbd_f", "float x")),
    ("long bbd_g(size_t n);", ("bbd_g", "size_t n")),
    ("int bbd_h(bbd_cand_t c, void* stream);", ("bbd_h", "bbd_cand_t c")),
    ("int bbd_k(unsigned int n);", ("bbd_k", "unsigned int n")),
    ("float bbd_r(int n);", ("bbd_r", "float")),
    ("int bbd_s(void* stream, int n);", ("bbd_s", "stream")),
    ("int bbd_t(int stream);", ("bbd_t", "stream")),
    ("#define BBD_X (1 << 3)", ("BBD_X", "(1 << 3)")),
    ("#define BBD_Y 1L", ("BBD_Y", "1L")),
    ("#define BBD_Z(a) 3", ("BBD_Z",)),
    ("#define BBD_W BBD_V", ("BBD_W", "BBD_V")),
])
def test_reader_raises_on_what_it_does_not_understand_and_names_it(text, names):
    from baseboostdepth_amd import _abi
    with pytest.raises(_abi.BbdError) as err:
        _abi.parse(text)
    for name in names:
        assert name in str(err.value)


def test_reader_on_the_real_header():
    from baseboostdepth_amd import _abi, _lib, ops
    protos, constants = _abi.read_header(HEADER)
    assert sorted(protos) == declared_functions() and len(protos) >= 110
    assert [n for n, p in protos.items() if p.restype is C.c_long] == LONG_RESULTS
    assert all(p.restype in (C.c_int, C.c_long) for p in protos.values())
    for name, proto in protos.items():
        where = [i for i, (_, pname) in enumerate(proto.params) if pname == "stream"]
        assert where == ([len(proto.params) - 1] if proto.has_stream else []), name
        assert _lib.SIGNATURES[name] == [t for t, _ in proto.params], name
    assert sum(p.has_stream for p in protos.values()) >= 80 and sum(not p.params for p in protos.values()) == 5
    # one constant of every literal form and origin
    assert constants["FLAG_NO_POSE_GRAD"] == 0x100 == _lib.FLAG_NO_POSE_GRAD
    assert constants["E_BADARG"] == -1 == _lib.E_BADARG and _lib.E_TOOMANY == -2
    assert constants["MAP_MAX_T"] == 1 << 30 == _lib.MAP_MAX_T
    assert constants["VIEW_MAX_CELLS"] == 1 << 28 == _lib.VIEW_MAX_CELLS and _lib.VIEW_MAX_LAYER == 65535
    assert constants["BN_MAX_GROUPS"] == 32 == ops.BN_MAX_GROUPS
    assert _lib.TRAJ_MODES == {"sim3": 0, "se3": 1, "scale": 2, "none": 3}
    assert _lib.CONSTANTS == constants and all(getattr(_lib, k) == v for k, v in constants.items())


def test_library_binds_every_host_side_helper_under_its_abi_name(lib_path):
    import nn_f64_ref as R
    from baseboostdepth_amd import _lib
    lib = _lib.get_lib()
    helpers = [n for n, p in _lib.PROTOTYPES.items() if not p.has_stream]
    assert len(helpers) == 30
    for name in helpers:
        bound = getattr(lib, name[len("bbd_"):])
        if _lib.PROTOTYPES[name].params:
            assert bound is getattr(lib._dll, name) and bound.argtypes == _lib.SIGNATURES[name]
            assert bound.restype is _lib.PROTOTYPES[name].restype
        else:
            assert type(bound) is int, name                  # a constant of the build
    assert (lib.tile_w, lib.tile_h, lib.abi_version) == (64, 16, _lib.ABI_VERSION)
    assert lib.smooth_chunks >= 1 and lib.project3d_bwd_blocks >= 1
    assert lib.num_tiles(192, 640) == 120
    for N, Cn, H, W in R.BN_SHAPES:
        assert lib.bn_scratch_doubles(N, Cn, H * W) == Cn * R.pick_split(N, H * W) * 2
    assert lib.map_state_bytes(1024) == 1024 * 48 + 32
    with pytest.raises(ctypes.ArgumentError):
        lib.num_tiles(192.0, 640)
    # the two helpers that older callers know under a shorter name
    assert lib.dwconv_wgrad_scratch_floats is lib.dwconv_tokens_wgrad_scratch_floats
    assert lib.dwconv_groups_wgrad_scratch_floats is lib.dwconv_tokens_groups_wgrad_scratch_floats


def test_missing_header_is_loud(tmp_path):
    from baseboostdepth_amd import _abi, _lib
    with pytest.raises(_lib.BbdError, match="nope.h not found"):
        _abi.read_header(str(tmp_path / "nope.h"))
