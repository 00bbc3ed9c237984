"""The solver's device code as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_harness): whole
interior-point solves on the CPU with every work buffer NaN-poisoned and allocated at its exact size; any out-of-bounds access or
undefined operation aborts the run, a read of a never-written word shows up as a NaN result.

This file: the thread-per-slot kernels (k_init, k_eval, k_expand, k_linesearch, k_update, k_plant, ...) with the serial Riccati
kernel (the LTOMPC_RICCATI=serial path) and k_pick on the harness's lock-step wavefront.  test_host_harness_wave.py, with the
same fixture: the wave kernels k_riccati8, k_riccati1, k_eval8 / k_expand8, k_sens_eval8, k_sens_riccati8, k_sens_forward,
k_psens_sweep, k_adj_sweep, the thread-per-slot kernels of the derivative passes (k_sens_eval, k_psens_cond, k_plant_sens,
k_planes_rows, k_loop_begin, k_loop_accum, k_theta_rows, k_slip_forces, k_test_ellipse, k_velocity_profile) and every _pi form.
test_host_harness_multiwave.py: the kernels whose workgroups have several wavefronts (k_riccati1q, k_step1, k_compact,
k_pack_perm), k_pack / k_pack_inverse and the rollout kernels, every multi-wavefront run in both wavefront orders.
Not modelled by the harness: several lanes adding to one LDS word in the same instruction, the ordering of global memory between
workgroups, the rollout's two streams.

The numbers are compared with the oracle (the GPU library's own results are compared with the oracle in test_gpu_parity.py).
Test infrastructure only: the package never builds or loads this."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")
EXE = os.path.join(HARNESS_DIR, "harness")


@pytest.fixture(scope="module")
def harness():
    srcs = [os.path.join(HARNESS_DIR, f) for f in ("harness.cpp", "hip_shim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    srcs.append(os.path.join(ROOT, "include", "ltompc.h"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLTOMPC_HOST_HARNESS",
                               "-I", CSRC, "-I", HARNESS_DIR, os.path.join(HARNESS_DIR, "harness.cpp"), "-o", EXE, "-lpthread"])
    return EXE


def _run(exe, tmp_path, tables, x0, N, any_bounds=0, soft_rho=0.0, ticks=2, ell=(0.0, 0.0, 0.0, 0.0), rows=None, cot=None, u=None, args=(),
         **options):
    """rows: B x 16 per-instance rows (section `rows` of the problem file); cot: a list of cotangents (gX (B,N+1,8), gU (B,N,2))
    for the adjoint sweeps of derivs=1; u: B x 2 controls for plant_sens=<n_sub>; args: further key=value arguments as they are
    (param.<field>=...); options: key=value arguments (a string as it is: riccati="8", eval="slot")."""
    prob = tmp_path / "problem.txt"
    tab = tables.packed()
    with open(prob, "w") as f:
        f.write(f"{tab.shape[1]} {N} {x0.shape[0]} {any_bounds} {soft_rho!r} {ticks} {ell[0]!r} {ell[1]!r} {ell[2]!r} {ell[3]!r}\n")
        np.savetxt(f, tab.ravel()[None], fmt="%.17g")
        np.savetxt(f, x0.ravel()[None], fmt="%.17g")
        if rows is not None:
            f.write("rows\n")
            np.savetxt(f, np.asarray(rows, dtype=np.float64).ravel()[None], fmt="%.17g")
        if u is not None:
            f.write("u\n")
            np.savetxt(f, np.asarray(u, dtype=np.float64).ravel()[None], fmt="%.17g")
        if cot:
            f.write(f"cot {len(cot)}\n")
            for gX, gU in cot:
                np.savetxt(f, np.concatenate([np.ravel(gX), np.ravel(gU)])[None], fmt="%.17g")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    argv = [exe, str(prob)] + [f"{k}={v if isinstance(v, str) else repr(v)}" for k, v in options.items()] + list(args)
    out = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]   # a sanitizer report or a mismatched collective ends the process with a non-zero code
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr and "MISMATCHED" not in out.stderr, out.stderr[-3000:]
    res, cur = [], None
    for line in out.stdout.splitlines():
        if line.startswith("tick"):
            cur = []; res.append(cur)
        else:
            cur.append([float(v) for v in line.split()])
    return [np.array(r) for r in res]


@pytest.mark.parametrize("any_bounds", [0, 1])
def test_device_code_is_sanitizer_clean_and_matches_the_oracle(harness, tmp_path, oracle, pkg, tables, any_bounds):
    """Two closed-loop ticks of a small batch (cold start + warm start through k_plant), N = 8: ASan / UBSan silent, no NaN
    from the poisoned buffers, statuses and controls as the oracle's.  The batch holds the reference's x0, sampled states, a
    state that needs the restoration phase and one that is off the track (INFEASIBLE)."""
    N = 8
    x0 = np.vstack([pkg.X0_REFERENCE[None], pkg.sample_x0(tables, 5, seed=61),
                    [[226.623754, -0.545036120, -0.0112268024, 8.52329373, 0.122918012, 0.161888169, 0.0837443810, 0.371730909]],
                    [[100.0, 4.0, 0.0, 10.0, 0, 0, 0, 0]]])
    res = _run(harness, tmp_path, tables, x0, N, any_bounds=any_bounds)
    x, ref, up = x0, None, np.zeros((len(x0), 2))
    for tick, r in enumerate(res):
        ref = oracle.solve(x, N, up, ref, nthreads=4, prev_status=None if ref is None else ref["status"])
        assert np.all(np.isfinite(r)), tick
        assert np.array_equal(r[:, 1].astype(int), ref["status"]), (tick, r[:, 1], ref["status"])
        both = ref["status"] == 0
        assert both.sum() >= 6 and np.abs(r[:, 3:5] - ref["u0"])[both].max() < 1e-6, tick
        assert (np.abs(r[:, 2] - ref["iters"])[both] <= 2).all(), tick
        # the harness continues from its own controls (k_plant, 100 sub-steps)
        x, up = oracle.plant_step(x, r[:, 3:5], n_sub=100), r[:, 3:5]
    assert len(res) == 2


def test_device_code_soft_constraints_under_sanitizers(harness, tmp_path, orc, pkg, tables):
    """The elastic planes (options.soft_rho) on the same harness."""
    N = 6
    x0 = pkg.sample_x0(tables, 4, seed=62)
    res = _run(harness, tmp_path, tables, x0, N, soft_rho=100.0, ticks=1)
    o = orc.default_options(); o.soft_rho = 100.0
    ref = orc.Oracle(tables.packed(), options=o).solve(x0, N, nthreads=4)
    assert np.all(np.isfinite(res[0])) and np.array_equal(res[0][:, 1].astype(int), ref["status"])
    assert np.abs(res[0][:, 3:5] - ref["u0"]).max() < 1e-6


def test_device_code_friction_ellipse_under_sanitizers(harness, tmp_path, orc, pkg, tables):
    """The friction-ellipse constraints (params.ell_*; kernels instantiated with ELL) on the same harness, against the oracle."""
    N = 6
    x0 = pkg.sample_x0(tables, 4, seed=63)
    ell = (10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0)
    res = _run(harness, tmp_path, tables, x0, N, ticks=1, ell=ell)
    p = orc.default_params(); p.ell_penalty, p.ell_rho, p.ell_D_f, p.ell_D_r = ell
    ref = orc.Oracle(tables.packed(), params=p).solve(x0, N, nthreads=4)
    assert np.all(np.isfinite(res[0])) and np.array_equal(res[0][:, 1].astype(int), ref["status"])
    ok = ref["status"] == 0
    assert ok.sum() >= 3 and np.abs(res[0][:, 3:5] - ref["u0"])[ok].max() < 1e-6
