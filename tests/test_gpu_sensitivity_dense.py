"""Parametric sensitivities (ltompc_get_sensitivities) against a reference without truncation error: at the
GPU's own final iterate, the implicit-function system of the barrier problem is assembled from the torch restatement of the
NLP and solved by a sparse LU with refinement in extended precision (sens_reference.py).  Every instance whose solver status
is SOLVED or ACCEPTABLE is compared, at every stage of dX and dU, through both evaluation paths (8 lanes per slot and thread
per slot), cold and after closed-loop ticks (u_prev != 0), with the default and a non-default bound pattern, with exact
tables and after re-packing.  ok is checked against an independent inertia test, margin against its definition."""
import os

import numpy as np
import pytest

import sens_reference as SR

pytestmark = pytest.mark.gpu

SOLVED_OR_ACCEPTABLE = (0, 1)
# Largest per-entry relative error |G - D| / max(1, |D|) on an instance with margin >= 1e-4, and the median over instances.
# Measured on MI355X (both paths, cold and two ticks): max 4.3e-10 / 3.7e-6 / 7.6e-6 / 7.3e-7 at N = 2 / 10 / 40 / 80, 7.4e-6
# with the other bound pattern, 2.4e-7 with exact tables, 1.4e-7 re-packed; medians 2e-15 .. 2e-14 at N <= 10, 1.0e-8 ..
# 2.4e-8 at N = 40 and 80; 1.0e-5 .. 2.2e-5 on three ill-conditioned N = 40 instances (below).  margin < 1e-4: at most 2.1e-6.
CAP = 1e-5
MEDIAN_CAP = 1e-7
# ok is compared with the reference's inertia outside this band of the smallest reduced-Hessian eigenvalue (there the
# float64 sweep and the LU may legitimately disagree on its sign).  Measured: the smallest |lam_min| was 1.6e-3.
BAND = 1e-6


def _log(name, text):
    f = os.environ.get("LTOMPC_TEST_RATES")
    if f:
        with open(f, "a") as fh:
            fh.write(f"{name} {text}\n")


def _x0_batch(pkg, tables, n, seed):
    """X0_REFERENCE, sampled states, and every fifth sampled state moved next to the right-hand edge of the band."""
    x = np.vstack([pkg.X0_REFERENCE[None], pkg.sample_x0(tables, n - 1, seed=seed)])
    s = x[5::5, 0]
    nl, nr = np.interp(s, tables.s_arc, tables.n_left), np.interp(s, tables.s_arc, tables.n_right)
    mid, w = 0.5 * (nl - nr), 0.5 * (nl + nr - 2.3)
    x[5::5, 1] = mid - 0.97 * w
    return x


def _eps(mpc, st, use):
    """The smoothing length of the sensitivity evaluation (ST_EPS): max(smooth_eps_min, smooth_scale * mu) at the final
    iterate (linesearch.h, riccati.h).  The tests only use instances where this is smooth_eps_min (or 0: exact tables)."""
    o = mpc.options
    if o.smooth_eps_min == 0 and o.smooth_scale == 0:
        return 0.0
    assert (o.smooth_scale * st["mu"][use] <= o.smooth_eps_min).all(), st["mu"][use].max()
    return o.smooth_eps_min


def _kernel_margin(T, NU):
    """The kernel's margin: min over every (slack, multiplier) plane pair m < ni of every stage of max(T, NU)."""
    return np.maximum(T, NU).min(axis=(1, 2))


def check_against_reference(pkg, tables, mpc, S, label, params=None, subset=None, layout=False):
    """Compare S = mpc.sensitivities(trajectory=True) of the last make_step with the dense reference at mpc's iterate.
    Returns the per-instance relative errors of the compared instances."""
    params = params or pkg.default_params()
    st, it = mpc.stats(), mpc.iterate()
    x0, up, _ = mpc.solved_parameters()
    B, N = mpc.B, mpc.N
    conv = np.isin(st["status_solver"], SOLVED_OR_ACCEPTABLE)
    if subset is not None:
        conv &= np.isin(np.arange(B), subset)
    idx = np.flatnonzero(conv)
    assert idx.size >= 0.6 * (B if subset is None else len(subset)), (label, idx.size)
    eps = _eps(mpc, st, conv)
    nb = len(SR.bound_rows(params))
    T, NU = it["T"], it["NU"]
    assert T.shape[2] == nb + 3
    if layout:
        # the plane mapping of ltompc_get_ineq: T = -h(w) at a SOLVED iterate on every constraint row
        for b in np.flatnonzero(st["status_solver"] == 0)[:16]:
            hv = SR.inequality_values({k: it[k][b] for k in ("X", "C", "U")}, x0[b], tables, eps, params)
            m = ~np.isnan(hv)
            assert np.abs(T[b][m] + hv[m]).max() <= 1e-7, (label, b, np.abs(T[b][m] + hv[m]).max())
    # margin, bit for bit: the kernel's loop covers m < ni at every stage, stage N-1's track planes included.  Those are not
    # constraints; their pair stays at its start (t = 1, nu = mu_init), so that the minimum is the one over the constraint
    # pairs whenever it is below 1.
    ok = S["ok"]
    host = _kernel_margin(T, NU)
    assert np.array_equal(S["margin"][ok], host[ok]), label
    assert (S["margin"][~ok] == 0).all()
    cons = np.ones(T.shape[1:], dtype=bool)
    cons[N - 1, nb:] = False
    on_cons = np.maximum(T, NU)[:, cons].min(axis=1)
    assert np.array_equal(host[ok & (on_cons < 1)], on_cons[ok & (on_cons < 1)]), label
    R = SR.sensitivities_batch({k: v[idx] for k, v in it.items()}, x0[idx], up[idx], tables, eps, params)
    G0 = np.concatenate([S["du0_dx0"], S["du0_duprev"]], axis=2)
    err, mg, gaps, band = [], [], [], []
    for b, r in zip(idx, R):
        assert r["backward"] < 1e-16, (label, b, r["backward"])
        if abs(r["lam_min"]) <= BAND:
            band.append(b)
            _log(f"dense_band_{label}", f"b {b} lam_min {r['lam_min']:.3e} scale {r['lam_scale']:.3e} ok {ok[b]} expected {r['ok_expected']}")
        else:
            assert ok[b] == r["ok_expected"], (label, b, ok[b], r["lam_min"], r["lam_scale"])
        if not ok[b]:
            continue
        e = max((np.abs(S["dX"][b] - r["dX"]) / np.maximum(1.0, np.abs(r["dX"]))).max(),
                (np.abs(S["dU"][b] - r["dU"]) / np.maximum(1.0, np.abs(r["dU"]))).max(),
                (np.abs(G0[b] - r["du0"]) / np.maximum(1.0, np.abs(r["du0"]))).max())
        err.append(e), mg.append(S["margin"][b]), gaps.append(r["gap"])
        assert r["margin"] == S["margin"][b] or S["margin"][b] >= 1, (label, b)
    err, mg, gaps = np.array(err), np.array(mg), np.array(gaps)
    hi = mg >= 1e-4
    _log(f"dense_{label}", f"conv {idx.size}/{B} ok {ok[idx].sum()} band {len(band)} compared {err.size} (margin >= 1e-4: {hi.sum()}) "
         f"err_pct50/90/100 {np.percentile(err[hi], [50, 90, 100]) if hi.any() else None} "
         f"low-margin err max {err[~hi].max() if (~hi).any() else None} err/gap max {(err[~hi] / np.maximum(gaps[~hi], 1e-16)).max() if (~hi).any() else None} "
         f"gap max {gaps.max() if gaps.size else None}")
    assert err.size >= 0.5 * idx.size, (label, err.size, idx.size)
    for e, g, m in zip(err[err > CAP], gaps[err > CAP], mg[err > CAP]):
        _log(f"dense_above_cap_{label}", f"err {e:.3e} gap {g:.3e} margin {m:.3e}")
    # CAP on every instance whose system is well conditioned; on the others (the unrefined float64 LU of the same system is
    # off by more than CAP: measured up to 1.6e-3 at N = 40) the kernels' float64 sweep may be off by as much as that gap.
    # Measured at N = 40: 1.0e-5, 1.2e-5, 2.2e-5 on three instances with gaps 6.6e-4, 3.8e-5, 9.9e-4 (the rest <= 7.6e-6).
    assert (err[hi] <= np.maximum(CAP, gaps[hi])).all(), (label, err[hi].max(), gaps[hi][np.argmax(err[hi])])
    assert np.median(err[hi]) <= MEDIAN_CAP, (label, np.median(err[hi]))
    # weakly active pairs (margin < 1e-4): worse conditioned still; bound scaled by the same gap
    low = err[~hi] <= np.maximum(CAP, 1e3 * gaps[~hi])
    assert low.all(), (label, err[~hi][~low], gaps[~hi][~low], mg[~hi][~low])
    return err


def _ticks(pkg, tables, x, N, label, options=None, params=None, ticks=3, layout=False):
    mpc = pkg.BatchedMPC(tables, N, x.shape[0], params=params, options=options)
    mpc.set_initial_guess(x)
    for t in range(ticks):
        u = mpc.make_step(x)
        S = mpc.sensitivities(trajectory=True)
        if t > 0:
            assert np.abs(mpc.solved_parameters()[1]).max() > 0  # u_prev != 0: the du0/du_prev columns at a real u_prev
        check_against_reference(pkg, tables, mpc, S, f"{label}_t{t}", params=params, layout=layout and t == 0)
        x = mpc.plant_step(x, u, 50)
    mpc.close()


# (batch sizes not a multiple of 8: padding lanes in both paths; at N = 2 and 10 not of 64 either)
@pytest.mark.parametrize("N,B", [(2, 197), (10, 197), (40, 61), (80, 29)])
@pytest.mark.parametrize("mode", [1, 2])
def test_sensitivities_match_the_dense_reference(pkg, tables, gpu_lib, N, B, mode):
    """latency_mode 1: k_sens_eval8 (8 lanes per slot), 2: k_sens_eval<BoundsRef, false> (thread per slot, the one used
    at the headline batch); the same states through both, a cold solve and two closed-loop ticks."""
    o = pkg.default_options()
    o.latency_mode = mode
    _ticks(pkg, tables, _x0_batch(pkg, tables, B, seed=70 + N), N, f"N{N}_mode{mode}", options=o, layout=True)


@pytest.mark.parametrize("mode", [1, 2])
def test_other_bound_pattern_matches_the_dense_reference(pkg, tables, gpu_lib, mode):
    """No bound on vx, an upper bound on n: k_sens_eval<BoundsAny, false> (mode 2) and d_eval8 with the run-time pattern."""
    p = pkg.default_params()
    p.x_lb[3] = -pkg.NO_BOUND
    p.x_ub[1] = 50.0
    o = pkg.default_options()
    o.latency_mode = mode
    _ticks(pkg, tables, _x0_batch(pkg, tables, 61, seed=81), 10, f"bounds_mode{mode}", options=o, params=p, layout=True)


def test_exact_tables_match_the_dense_reference(pkg, tables, gpu_lib):
    """smooth_eps_min = smooth_scale = 0: the reference's piece-wise-linear tables (eps = 0 in the sensitivity pass)."""
    o = pkg.default_options()
    o.smooth_eps_min = o.smooth_scale = 0.0
    _ticks(pkg, tables, _x0_batch(pkg, tables, 61, seed=83), 10, "exact", options=o, ticks=2)


def test_repacked_instances_match_the_dense_reference(pkg, tables, gpu_lib):
    """B >= 1024, warm ticks (instances re-packed): sensitivities(), then iterate() (un-packs, sets sens_moved), then
    sensitivities(True), which refactorises at the new slots."""
    x = _x0_batch(pkg, tables, 1024, seed=85)
    mpc = pkg.BatchedMPC(tables, 10, x.shape[0])
    mpc.set_initial_guess(x)
    for _ in range(3):
        u = mpc.make_step(x)
        x = mpc.plant_step(x, u, 50)
    u = mpc.make_step(x)
    S1 = mpc.sensitivities()
    mpc.iterate()
    S = mpc.sensitivities(trajectory=True)
    for k in ("du0_dx0", "du0_duprev", "ok", "margin"):
        assert np.array_equal(S1[k], S[k]), k
    G = np.concatenate([S["du0_dx0"], S["du0_duprev"]], axis=2)
    assert np.array_equal(S["dU"][:, 0], G)
    check_against_reference(pkg, tables, mpc, S, "repacked", subset=np.arange(0, 1024, 11))
    mpc.close()
