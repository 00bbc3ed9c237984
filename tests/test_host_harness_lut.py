"""The batched table look-up (csrc/model.h: slot_luts_fetch / slot_luts_pin / slot_luts_finish) against lut_eval as host C++ under
ASan + UBSan: tests/host_harness/lut_harness.cpp runs k_test_lut, the kernel behind ltompc_test_lut, on the arc lengths of
tests/test_gpu_lut_batch.py (every knot of both grids, first and last interval, extrapolation on both sides, inside and outside the
smoothing width of a knot, points where the interval estimate is off; one and two laps on for the periodic table) at eps = 0 and
at the default smooth_eps_min, every table row allocated on its own at its exact size, and compares the two forms bit for bit.
The batched form loads the knots of all five look-ups whether or not the caller uses them: a knot taken from past either end of a
row would abort the run here."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_lut_batch import SMOOTH_EPS_MIN, _estimate_off, _points, _pwl

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")
EXE = os.path.join(HARNESS_DIR, "lut_harness")


@pytest.fixture(scope="module")
def lut_harness():
    srcs = [os.path.join(HARNESS_DIR, f) for f in ("lut_harness.cpp", "hip_shim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    srcs.append(os.path.join(ROOT, "include", "ltompc.h"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLTOMPC_HOST_HARNESS",
                               "-I", CSRC, "-I", HARNESS_DIR, os.path.join(HARNESS_DIR, "lut_harness.cpp"), "-o", EXE, "-lpthread"])
    return EXE


@pytest.mark.parametrize("periodic", [0, 1])
def test_batched_lookup_equals_lut_eval_under_sanitizers(lut_harness, tables, tmp_path, periodic):
    s, off = _points(tables)
    assert off.sum() >= 20 and _estimate_off(tables.s_arc, s[off]).all(), off.sum()
    if periodic:
        span = tables.s_arc[-1] - tables.s_arc[0]
        s = np.concatenate([s, s + span, s + 2.0 * span])
    eps = [0.0, SMOOTH_EPS_MIN]
    prob = tmp_path / "lut.txt"
    with open(prob, "w") as f:
        f.write(f"{tables.n} {periodic} {len(eps)} {len(s)}\n")
        np.savetxt(f, np.array(eps)[None], fmt="%.17g")
        np.savetxt(f, tables.packed(), fmt="%.17g")
        np.savetxt(f, s[None], fmt="%.17g")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([lut_harness, str(prob)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(eps) + 1
    for e, line in zip(eps, [lines[0]] + lines[2:]):
        w = line.split()
        assert w[0] == "eps" and float(w[1]) == e and int(w[3]) == len(s) and int(w[5]) == 0, line
    # ... and the harness looked up what it says, where it says (eps = 0: piece-wise linear, no curvature)
    assert lines[1].startswith("direct ")
    direct = np.array([float(v) for v in lines[1].split()[1:]]).reshape(len(s), 5, 3)
    assert np.all(np.isfinite(direct)) and np.all(direct[:, :, 2] == 0.0)
    if not periodic:
        sx = s[::-1]
        ref = np.stack([_pwl(tables.s_kappa, tables.kappa, s), _pwl(tables.s_kappa, tables.kappa, sx), _pwl(tables.s_arc, tables.v_ref, sx),
                        _pwl(tables.s_arc, tables.n_left, sx), _pwl(tables.s_arc, tables.n_right, sx)], axis=1)
        assert np.abs(direct[:, :, 0] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
