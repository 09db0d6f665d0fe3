"""CPU tier: the binding of the host ports itself (tests/ports.py) - what the one library exports, the error contract
it shares with `HipLibrary.call`, a missing port, and the typing rule of the size helpers."""
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
