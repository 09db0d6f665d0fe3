"""CPU tier: the binding of the host ports itself (tests/ports.py) - what the one library exports, the error contract
it shares with `HipLibrary.call`, a missing port, and the typing of every call from include/bbd_hip.h."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ports  # noqa: E402
from baseboostdepth_amd import _lib  # noqa: E402
from baseboostdepth_amd._lib import ptr  # noqa: E402

# exports with no twin in the ABI: two diagnostics of the tests, and the image port's whole-table sweeps
NOT_IN_ABI = ("hp_check_div", "hp_map_points", "hp_img_rgb2hsv_all", "hp_img_hsv2rgb_all", "hp_img_luma_all",
              "hp_img_blend_all")


@pytest.fixture(scope="module")
def port():
    return ports.PortBackend()


def test_every_export_is_the_twin_of_an_abi_name():
    out = subprocess.run(["nm", "-D", "--defined-only", ports.build()], check=True, capture_output=True, text=True).stdout
    exports = {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("hp_")}
    assert len(exports) > len(NOT_IN_ABI)
    twins = {"hp_" + name[len("bbd_"):] for name in _lib.SIGNATURES}
    assert exports - twins == set(NOT_IN_ABI)


def test_run_raises_the_error_of_the_hip_library_and_records_the_call(port):
    disp, out = torch.zeros(1, 3, 4), torch.zeros(1, 3, 4)
    args = (ptr(disp), ptr(out), disp.shape[0] // 2, 3, 4)       # an odd leading dimension: no pair to blend
    rc = port.status("bbd_post_process_disp", *args)
    assert rc != 0
    before = len(port.calls)
    with pytest.raises(_lib.BbdError) as err:
        port.run("bbd_post_process_disp", disp, *args)
    assert str(err.value) == "bbd_post_process_disp failed with status %d" % rc
    assert port.calls[before:] == ["bbd_post_process_disp"]


def test_a_missing_port_names_its_symbol(port):
    with pytest.raises(AttributeError, match="hp_no_such_entry"):
        port.status("bbd_no_such_entry")


def test_size_helpers_follow_the_typing_rule_of_the_hip_library(port):
    assert port.lib.map_state_bytes(1024) == 1024 * 48 + 32
    assert port.lib.map_state_bytes(1000) == -1


def _ground_scale_on_the_smallest_scene(port, camera_height):
    """`bbd_ground_scale` through the port on the 3 x 3 scene of ground_checks' case 3: (status, rows, mask)."""
    import ground_checks
    call = ground_checks.case(3)[0][-1]
    n, h, w = call.pred.shape
    assert (n, h, w) == (1, 3, 3)
    pred, inv_K = torch.from_numpy(call.pred), torch.from_numpy(call.inv_K).reshape(1, 3, 3).contiguous()
    rows, mask = torch.full((n, _lib.EVAL_OUT), 77.0), torch.full((n, h, w), 77, dtype=torch.uint8)
    scratch = torch.zeros(port.lib.ground_scale_scratch_floats(n, h, w))
    rc = port.status("bbd_ground_scale", ptr(pred), ptr(inv_K), ptr(rows), ptr(mask), ptr(scratch), n, h, w,
                     camera_height, math.cos(math.radians(5.0)), call.kw["min_count"], 0)
    return rc, rows, mask


def test_a_python_int_in_a_double_slot_travels_as_the_equal_float(port):
    """The port converts by the header's types, like `HipLibrary`: camera_height = 2 is the double 2.0, not a C int."""
    import ground_checks
    rc_f, rows_f, mask_f = _ground_scale_on_the_smallest_scene(port, 2.0)
    rc_i, rows_i, mask_i = _ground_scale_on_the_smallest_scene(port, 2)
    assert rc_f == 0 and rows_f[0, 1] == 1 and abs(float(rows_f[0, 7]) * ground_checks.HEIGHT / 2.0 - 1.0) < 1e-5
    assert rc_i == rc_f
    assert rows_i.numpy().tobytes() == rows_f.numpy().tobytes() and mask_i.numpy().tobytes() == mask_f.numpy().tobytes()


def test_a_float_in_an_int_slot_is_refused_like_the_hip_library_refuses_it(port):
    disp, out = torch.zeros(2, 3, 4), torch.zeros(1, 3, 4)
    assert port.status("bbd_post_process_disp", ptr(disp), ptr(out), 1, 3, 4) == 0
    with pytest.raises(ctypes.ArgumentError):
        port.status("bbd_post_process_disp", ptr(disp), ptr(out), 1.0, 3, 4)
    with pytest.raises(ctypes.ArgumentError):
        port.lib.map_state_bytes(1024.0)
    from baseboostdepth_amd.csrc.build import build
    lib = _lib.HipLibrary(build())
    with pytest.raises(ctypes.ArgumentError):            # refused before anything is called: no GPU is needed
        lib.call("bbd_post_process_disp", ptr(disp), ptr(out), 1.0, 3, 4, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.map_state_bytes(1024.0)


def test_every_ported_entry_is_typed_by_the_header_minus_the_stream(port):
    typed = 0
    for name, proto in _lib.PROTOTYPES.items():
        fn = getattr(port.dll, "hp_" + name[len("bbd_"):], None)
        if fn is not None:
            typed += 1
            assert list(fn.argtypes) == _lib.SIGNATURES[name][:len(proto.params) - proto.has_stream], name
            assert fn.restype is proto.restype, name
    assert typed > 40
    assert port.dll.hp_gather_pairs.argtypes[5] is ctypes.c_long          # `long chw`, as the ABI has it
    with pytest.raises(AttributeError):
        port.lib.post_process_disp                       # takes a stream: no host-side helper
