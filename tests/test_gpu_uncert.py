"""GPU tier of the uncertainty kernels (bbd_uncert.hip through the C ABI): on every case of
tests/uncert_checks.py the device equals the host port byte for byte over the whole `out` tensor, and a second identical
call gives the same bytes; the flip pass; the argument errors.

No tolerance anywhere: the float32 terms are one IEEE operation where written, the sort is exact and the float64 sums
are added in the one order bbd_uncert_math.h writes down for the device and the port alike, so a difference - in a
division, a square root, a tie - would be a finding, not noise."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncert_checks as uc  # noqa: E402
import uncert_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.mark.parametrize("name", uc.CASES)
def test_device_matches_the_port(hip, port, name):
    uc.precondition(name)
    got, want = uc.run(name, hip, DEV), uc.run(name, port, "cpu")
    differ = (got.view("uint64") != want.view("uint64"))
    print("%s: %d of %d values differ from the port" % (name, int(differ.sum()), differ.size))
    assert uc.same_bytes(got, want)                                    # byte for byte the host port
    assert uc.same_bytes(got, uc.run(name, hip, DEV))                  # identical calls, identical bytes


@pytest.mark.parametrize("w", uc.FLIP_WIDTHS)
def test_flip_pass(hip, w):
    out, uncert, blended = uc.run_flip(w, hip, DEV)
    assert uc.same_bytes(out, blended)
    assert uc.same_bytes(uncert, ref.flip_uncert(uc.make_flip(w)))


def test_argument_errors_launch_nothing(hip, port):
    lib = hip.lib

    def status(name, *args):
        return getattr(lib._dll, name)(*args, None)

    assert uc.same_bytes(uc.bad_argument_sweep(status, DEV), uc.run("ragged", port, "cpu"))
