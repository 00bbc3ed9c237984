"""The table-gradient pass (csrc/table_sensitivity.h) as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/host_harness/tabgrad_harness.cpp, a stand-alone program, runs the re-linearisation, the head-less sweep, k_adj_sweep_tab,
k_tab_cond and k_tab_scatter (and the _pi forms) on the lock-step wavefront of hip_shim.h at oracle iterates, every buffer at its
exact size and NaN-filled, the instances in permuted slots.  Its slot_grad and grad_tables are compared with the dense
reference (table_sens_reference.py) - the mathematics of the kernels checked without a GPU - and `lut_basis` with `lut_eval`
at the look-up edges of synthetic_tracks.  Shapes: N = 2 and 11, B = 1 and 13, on a 12-knot jittered table (many slots hit one
knot, the interval estimate misses and the fallback search runs) and on the shipped one.
Test infrastructure only: the package never builds or loads the harness."""
import os
import subprocess

import numpy as np
import pytest

import synthetic_tracks as ST
import table_sens_reference as TR
from conftest import ROOT
from test_sens_reference import KEYS

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")
EXE = os.path.join(HARNESS_DIR, "tabgrad_harness")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
# |harness - reference| / max(scale, 1), scale = the sum of the absolute terms of the reference's contraction.  Both sides work
# at the same iterate in float64; what separates them is the rounding of the stage solves, amplified along the horizon.  Measured
# with this program (g++ -O1, x86-64) over the cases below: 2e-15 .. 2e-12 in seven of the eight cases, and in the eighth (the
# shipped table, N = 11, B = 13: one instance on the right-hand boundary) slot_grad 3.90e-8, grad_tables 5.9e-9.  The bound is
# 10 x the largest, 25 times below §9's cap of 1e-5.
BOUND = 3.9e-7


@pytest.fixture(scope="module")
def tabgrad():
    srcs = [os.path.join(HARNESS_DIR, f) for f in ("tabgrad_harness.cpp", "hip_shim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    srcs.append(os.path.join(ROOT, "include", "ltompc.h"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLTOMPC_HOST_HARNESS",
                               "-I", CSRC, "-I", HARNESS_DIR, os.path.join(HARNESS_DIR, "tabgrad_harness.cpp"), "-o", EXE, "-lpthread"])
    return EXE


def _start(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=ENV, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr and "MISMATCHED" not in out.stderr, out.stderr[-3000:]
    return out.stdout


def twelve_knots():
    """The chicane on 12 jittered knots per grid (spacings differ by up to a factor of 9): an N <= 11 horizon stays inside two
    or three intervals."""
    return ST.chicane(n=12, jitter=8.0, seed=5, noise=4.0)


def _run(exe, tmp_path, track, r, x0, N, eps, gX, gU, rows=None):
    B = x0.shape[0]
    prob = tmp_path / "tabgrad.txt"
    with open(prob, "w") as f:
        f.write(f"{track.n} {N} {B} {eps!r} 0 {0 if rows is None else 1}\n")
        for a in (track.packed(), x0, r["X"], r["C"], r["L1"], r["L2"], r["U"]):
            np.savetxt(f, np.ravel(a)[None], fmt="%.17g")
        f.write(f"{r['T'].shape[2]}\n")
        for a in (r["T"], r["NU"], r["mu"], gX, gU) + (() if rows is None else (rows,)):
            np.savetxt(f, np.ravel(a)[None], fmt="%.17g")
    lines = _start(exe, str(prob)).splitlines()
    assert lines[0].startswith("ok ") and len(lines) == 3
    ok = np.array(lines[0].split()[1:], dtype=int)
    return ok, np.array(lines[1].split(), float).reshape(B, N, TR.NS), np.array(lines[2].split(), float).reshape(4, track.n)


def test_lut_basis_matches_lut_eval(tabgrad, tmp_path, tables):
    """lut_basis' weights reproduce lut_eval's value and slope (two rows per grid) at every look-up edge of the jittered
    synthetic tracks - knots +- 1e-9, window borders, estimate misses, beyond both ends - with eps = 1e-4 and 0, periodic with
    points some laps away, and on the shipped table; the knots are the numpy lut_basis' and the weights agree to rounding."""
    cases = [(ST.get(n), 0, ST.edges(n)) for n in ("chicane40_jit20", "chicane200_jit8_neg", "chicane5_jit5", "stadium4")]
    per = ST.get(ST.PERIODIC)
    L = per.s_arc[-1] - per.s_arc[0]
    e = ST.edges(ST.PERIODIC, max_knots=40)
    cases.append((per, 1, np.concatenate([e, e[::7] + 3 * L, e[::11] - 2 * L])))
    cases.append((tables, 0, ST.lookup_edges(tables, max_knots=48)))
    cases.append((twelve_knots(), 0, ST.lookup_edges(twelve_knots())))
    for track, periodic, pts in cases:
        for eps in (1e-4, 0.0):
            path = tmp_path / "lut.txt"
            with open(path, "w") as f:
                f.write(f"{track.n} {periodic} {eps!r} {len(pts)}\n")
                np.savetxt(f, track.packed().ravel()[None], fmt="%.17g")
                np.savetxt(f, np.asarray(pts)[None], fmt="%.17g")
            out = np.array([ln.split() for ln in _start(tabgrad, "lut", str(path)).splitlines()], float).reshape(len(pts), 2, 20)
            for gi, (grid, ys) in enumerate(((track.s_kappa, (track.kappa, track.kappa)), (track.s_arc, (track.n_left, track.v_ref)))):
                o = out[:, gi]
                dmin = np.diff(grid).min()
                for c, y in enumerate(ys):
                    sc = np.abs(y).max() + 1e-300
                    assert np.abs(o[:, 4 + 2 * c] - o[:, 2 * c]).max() <= 1e-13 * sc, (track.n, periodic, eps, gi, c)
                    assert np.abs(o[:, 5 + 2 * c] - o[:, 1 + 2 * c]).max() <= 1e-12 * sc / dmin, (track.n, periodic, eps, gi, c)
                period = grid[-1] - grid[0] if periodic else 0.0
                for q, s in enumerate(pts):
                    idx, wv, ws = TR.lut_basis(grid, s, eps, period)
                    assert np.array_equal(o[q, 8:12].astype(int), idx), (track.n, s, eps)
                    assert np.abs(o[q, 12:16] - wv).max() <= 1e-12 and np.abs(o[q, 16:20] - ws).max() <= 1e-11 / dmin, (track.n, s, eps)


@pytest.mark.parametrize("track_name", ["twelve", "shipped"])
@pytest.mark.parametrize("N,B,pi", [(2, 1, False), (2, 13, True), (11, 1, True), (11, 13, False)])
def test_pass_is_sanitizer_clean_and_matches_the_dense_reference(tabgrad, tmp_path, pkg, orc, tables, track_name, N, B, pi):
    """slot_grad of every ok instance at every slot and grad_tables per row against the dense reference at the same (oracle)
    iterate, measure and bound above; instances that are not ok contribute exactly 0.  With pi the rows are the handle's values
    in every instance (the _pi kernels must then give what the reference's default vehicle gives)."""
    track = twelve_knots() if track_name == "twelve" else tables
    x0 = ST.sample(track, B, seed=40 + N, margin=40.0) if track_name == "twelve" else pkg.sample_x0(tables, B, seed=40 + N)
    O = orc.Oracle(track.packed())
    r = O.solve(x0, N, nthreads=4)
    eps = O.o.smooth_eps_min
    assert (r["mu"][r["status_solver"] <= 1] <= eps).all()
    rng = np.random.default_rng(N + B)
    gX, gU = rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))
    params = pkg.default_params()
    import param_sens_reference as PR
    rows = np.tile(PR.theta_values(params), (B, 1)) if pi else None
    ok, sg, gt = _run(tabgrad, tmp_path, track, r, x0, N, eps, gX, gU, rows)
    conv = r["status_solver"] <= 1
    assert (ok[~conv] == 0).all() and ok.sum() >= max(1, (3 * B) // 4), (ok, r["status_solver"])
    use = np.flatnonzero(ok == 1)
    ref = TR.table_gradients_batch({k: r[k][use] for k in KEYS}, x0[use], np.zeros((use.size, 2)), track, eps, params, gX[use], gU[use])
    assert ref["ok_expected"].all()
    assert (sg[ok == 0] == 0).all() and np.isfinite(sg).all() and np.isfinite(gt).all()
    e_slot = np.abs(sg[use] - ref["slot_grad"]) / np.maximum(ref["slot_scale"], 1.0)
    want, mag = np.zeros_like(gt), np.zeros_like(gt)
    for m, b in enumerate(use):
        X = r["X"][b].copy()
        X[0] = x0[b]
        _, mg = TR.scatter(ref["slot_grad"][m], r["C"][b][:, 0], X[1:, 0], track, eps)
        want += ref["grad_tables"][m]
        mag += mg
    e_tab = np.abs(gt - want).max(axis=1) / np.maximum(mag.sum(axis=1), 1.0)
    print(f"{track_name} N {N} B {B} pi {pi}: ok {ok.sum()} slot err max {e_slot.max():.3e} (column {int(np.argmax(e_slot.max(axis=(0, 1))))}) "
          f"table err per row {e_tab}")
    assert np.abs(ref["slot_grad"]).max(axis=(0, 1)).min() > 0 or N == 2      # every one of the ten scalars is exercised
    assert e_slot.max() <= BOUND, (e_slot.max(), np.unravel_index(np.argmax(e_slot), e_slot.shape))
    assert e_tab.max() <= BOUND, e_tab
    assert (gt[mag == 0] == 0).all()   # knots that no look-up touches: exactly 0
