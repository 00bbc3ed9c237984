"""k_jvp_sweep / k_jvp_sweep_pi (csrc/jvp.h) as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host_harness/jvp_harness.cpp, a stand-alone program over hip_shim.h's lock-step 64-lane wavefront): exact-size,
NaN-poisoned buffers with seeded well-conditioned data and a non-identity orig; B = 13 and 61 (padding lanes), N = 2 and 10, both
kernels, with and without dtheta, against a plain serial restatement of the recursion in the same program (relative bound: 10 x
the measured maximum, in the program), exact zeros where ok = 0.  Test infrastructure only: the package never builds or loads this."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")
EXE = os.path.join(HARNESS_DIR, "jvp_harness")


@pytest.fixture(scope="module")
def jvp_harness():
    srcs = [os.path.join(HARNESS_DIR, f) for f in ("jvp_harness.cpp", "hip_shim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    srcs.append(os.path.join(ROOT, "include", "ltompc.h"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLTOMPC_HOST_HARNESS",
                               "-I", CSRC, "-I", HARNESS_DIR, os.path.join(HARNESS_DIR, "jvp_harness.cpp"), "-o", EXE, "-lpthread"])
    return EXE


def test_jvp_sweeps_are_sanitizer_clean_and_match_the_serial_recursion(jvp_harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([jvp_harness], capture_output=True, text=True, env=env, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])  # a failed check, a sanitizer report or a mismatched collective
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr and "MISMATCHED" not in out.stderr, out.stderr[-3000:]
    cases = re.findall(r"^case B=(\d+) N=(\d+) pi=(\d) dtheta=(\d): max_rel (\S+) bad (\d+)$", out.stdout, re.M)
    assert sorted((int(b), int(n), int(p), int(t)) for b, n, p, t, _, _ in cases) == sorted(
        (b, n, p, t) for b in (13, 61) for n in (2, 10) for p in (0, 1) for t in (0, 1))
    assert all(int(bad) == 0 for *_, bad in cases)
    m = re.search(r"^max_rel (\S+) bound (\S+) failed 0$", out.stdout, re.M)
    assert m and float(m.group(1)) <= float(m.group(2))
