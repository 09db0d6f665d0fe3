"""The uncertainty host port under AddressSanitizer and UndefinedBehaviorSanitizer, as a STAND-ALONE program
(tests/sanitize/uncert_port_main.cpp with its own `main`, built with -fsanitize=address,undefined and run as a child
process on the `tiny`, `ragged` and `exact` inputs of tests/uncert_checks.py): nothing sanitized is loaded into Python,
and the runtimes are linked statically into the program, so its environment is the caller's, untouched.
The port is the kernels' arithmetic, indexing and scratch rule (bbd_uncert_math.h) in serial loops, so an index past a
window, a slot past N or a bucket past K would be a report here.  CPU tier."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncert_checks as uc  # noqa: E402
from baseboostdepth_amd import _lib, evaluation  # noqa: E402


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sanitize") / "uncert_port_main")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-fast-math", "-std=c++17", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "sanitize", "uncert_port_main.cpp"),
           os.path.join(ROOT, "tests", "host_port", "bbd_uncert_port.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("name", ["tiny", "ragged", "exact"])
def test_port_runs_clean_under_the_sanitizers(program, tmp_path, name):
    case = uc.make(name)
    n, h, w = case["pred"].shape
    gts = evaluation.GroundTruthSet(case["gts"], "cpu", crop=case["crop"])
    flags = 0 if case["median_scaling"] else _lib.EVAL_NO_MEDIAN_SCALING
    gt = gts.buffer.numpy()
    with open(tmp_path / "case.bin", "wb") as f:
        f.write(np.array([n, h, w, case["K"], flags, gt.size], "<i4").tobytes())
        f.write(np.array([case["min_depth"], case["max_depth"], case["scale_factor"]], "<f8").tobytes())
        for arr in (case["pred"], case["uncert"], gt, gts.desc_host, uc.rows(name)):
            f.write(np.ascontiguousarray(arr).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], env=env, capture_output=True,
                          text=True, timeout=60)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-2000:]
    got = np.fromfile(tmp_path / "out.bin", "<f8").reshape(n, -1)
    import ports
    assert uc.same_bytes(got, uc.run(name, ports.PortBackend(), "cpu"))       # -O1 sanitized = -O2 port: the same bytes
