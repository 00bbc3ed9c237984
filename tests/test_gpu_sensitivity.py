"""Parametric sensitivities of the solution w.r.t. p = (x0, u_prev) (ltompc_get_sensitivities): against
central differences of independent oracle solves, second order of the tangential predictor, scheduling invariance, no side
effects on the solver, edge cases."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Central-difference step, the same for every column.  A step relative to |p_j| is 2e-3 m for s ~ 200 m: of the order of the
# smallest max(t, nu) of many solutions, and the difference then carries a truncation error of 1e-2 .. 4e-1 (measured; it falls
# as h^2 down to h = 1e-7).  At h = 1e-6 truncation and rounding (u0 to ~1e-12) are both below 1e-5.
H_ABS = 1e-6


def _tol(margin):
    """Agreement expected between the barrier derivative and central differences of converged solves: 1e-4, plus the
    O(mu / margin^2) term of a weakly active pair at mu = mu_min = 1e-9 (measured: 3.2e-4 at margin 1.5e-3)."""
    return 1e-4 + 1e-9 / np.maximum(np.asarray(margin), 1e-12) ** 2


def _rate(name, value, minimum):
    """A measured rate against its floor; LTOMPC_TEST_RATES=<file> logs the measured values."""
    f = os.environ.get("LTOMPC_TEST_RATES")
    if f:
        with open(f, "a") as fh:
            fh.write(f"{name} {float(value):.4f} (min {minimum})\n")
    assert value >= minimum, (name, float(value), minimum)


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


def _central_differences(orc, tables, x, N, options=None, h=None):
    """du0/dp by central differences of oracle solves, warm-started from the oracle's own solve at p; (B,2,10), base, and
    whether all 20 perturbed solves of an instance ended SOLVED (the solver's own status)."""
    O = orc.Oracle(tables.packed(), options=options)
    base = O.solve(x, N)
    B = x.shape[0]
    P = np.hstack([x, np.zeros((B, 2))])
    H = np.full_like(P, H_ABS if h is None else h)
    warm = {k: np.repeat(base[k], 10, 0) for k in ("X", "C", "U", "L1", "L2")}
    S = np.zeros((B, 2, 10))
    solved = np.ones(B, dtype=bool)
    for sgn in (1.0, -1.0):
        X, U = np.repeat(x, 10, 0), np.zeros((B * 10, 2))
        for j in range(10):
            if j < 8:
                X[j::10, j] += sgn * H[:, j]
            else:
                U[j::10, j - 8] += sgn * H[:, j]
        r = O.solve(X, N, uprev=U, warm=warm, prev_status=np.repeat(base["status_solver"], 10))
        S += sgn * r["u0"].reshape(B, 10, 2).transpose(0, 2, 1)
        solved &= (r["status_solver"].reshape(B, 10) == 0).all(axis=1)
    return S / (2.0 * H[:, None, :]), base, solved


def _gpu(pkg, tables, x, N, options=None, trajectory=False):
    mpc = pkg.BatchedMPC(tables, N, x.shape[0], options=options)
    mpc.set_initial_guess(x)
    u0 = mpc.make_step(x)
    S = mpc.sensitivities(trajectory=trajectory)
    st = mpc.stats()
    return mpc, u0, S, st


def _du0(S):
    return np.concatenate([S["du0_dx0"], S["du0_duprev"]], axis=2)


@pytest.mark.parametrize("N", [10, 40])
def test_sensitivities_match_central_differences(pkg, tables, orc, gpu_lib, N):
    x = _x0_batch(pkg, tables, 64, seed=11 + N)
    mpc, u0, S, st = _gpu(pkg, tables, x, N, trajectory=True)
    fd, base, fd_solved = _central_differences(orc, tables, x, N)
    # the reference itself: differences at 10 h must agree with those at h, else the solution is not smooth at the scale of
    # the step (a weakly active constraint switching sides inside it; measured on 1 of 25 / 1 of 16 used instances)
    fd10, _, fd10_solved = _central_differences(orc, tables, x, N, h=10 * H_ABS)
    smooth = (np.abs(fd - fd10) / np.maximum(1.0, np.abs(fd))).max(axis=(1, 2)) <= 1e-4
    ok, margin = S["ok"], S["margin"]
    G = _du0(S)
    # every solve an instance's check rests on ended SOLVED: the GPU's, the oracle's at p and its 20 perturbed ones
    use = ok & (margin >= 1e-3) & (st["status_solver"] == 0) & (base["status_solver"] == 0) & fd_solved & \
        fd10_solved & smooth & (np.abs(u0 - base["u0"]).max(axis=1) < 1e-6)
    err = (np.abs(G - fd) / np.maximum(1.0, np.abs(G))).max(axis=(1, 2))
    _log(f"sens_fd_N{N}", f"ok {ok.mean():.4f} used {use.sum()} not smooth {(~smooth & ok & (margin >= 1e-3)).sum()} err_pct50/90/100 {np.percentile(err[use], [50, 90, 100])} "
         f"err/tol max {(err[use] / _tol(margin[use])).max():.3f} "
         f"margin_hist {np.histogram(np.log10(np.maximum(margin[ok], 1e-16)), bins=[-16, -6, -4, -3, -2, -1, 0, 9])[0].tolist()}")
    _rate(f"sens_ok_fraction_N{N}", ok.mean(), 0.9)
    # (margin >= 1e-3 keeps 25 / 64 at N = 10 and 16 / 64 at N = 40: most solutions have a weakly active constraint somewhere
    #  on the horizon)
    assert use.sum() >= 12, use.sum()
    for b in np.flatnonzero(use & (err > _tol(margin))):
        e = np.abs(G[b] - fd[b]) / np.maximum(1.0, np.abs(G[b]))
        r, c = np.unravel_index(np.argmax(e), e.shape)
        _log(f"sens_fd_worst_N{N}", f"b {b} margin {margin[b]:.2e} row {r} col {c} G {G[b, r, c]:.6e} fd {fd[b, r, c]:.6e} u0 {u0[b]}")
    bad = err[use] > _tol(margin[use])
    assert not bad.any(), (np.flatnonzero(use)[bad], err[use][bad], margin[use][bad])
    # trajectories on a subset: dU_k and dX_{k+1} against the differences of the oracle's U and X, every stage
    dX, dU = S["dX"], S["dU"]
    O = orc.Oracle(tables.packed())
    for b in np.flatnonzero(use)[:8]:
        warm = {k: np.repeat(base[k][b:b + 1], 10, 0) for k in ("X", "C", "U", "L1", "L2")}
        fds = {}
        for h in (H_ABS, 10 * H_ABS):
            res = []
            for sgn in (1.0, -1.0):
                X, U = np.repeat(x[b:b + 1], 10, 0), np.zeros((10, 2))
                for j in range(10):
                    if j < 8:
                        X[j, j] += sgn * h
                    else:
                        U[j, j - 8] += sgn * h
                res.append(O.solve(X, N, uprev=U, warm=warm, prev_status=np.repeat(base["status_solver"][b], 10)))
                assert (res[-1]["status_solver"] == 0).all()
            fds[h] = [(res[0][k] - res[1][k]).transpose(1, 2, 0) / (2 * h) for k in ("U", "X")]
        # stages 0 .. 2 (dU_0, dU_1, dX_0 .. dX_2); later stages are logged, not asserted: DESIGN.md §9 (open point, measured
        # up to 7e-4 / 6.5e-3 on 1 of 4 instances while du0 agrees to 1e-5)
        for name, D, F, F10 in (("dU", dU[b][:2], *[f[0][:2] for f in fds.values()]), ("dX", dX[b][:3], *[f[1][:3] for f in fds.values()])):
            # entries whose differences are smooth at the scale of the step (the same validation as for du0)
            valid = np.abs(F - F10) / np.maximum(1.0, np.abs(F)) <= 1e-4
            e = np.abs(D - F) / np.maximum(1.0, np.abs(D))
            _log(f"sens_traj_N{N}", f"b {b} {name} margin {margin[b]:.2e} valid {valid.mean():.3f} err {e[valid].max():.2e} "
                 f"(all entries {e.max():.2e})")
            assert valid.mean() >= 0.9, (b, name, valid.mean())
            assert e[valid].max() <= _tol(margin[b]), (b, name, e[valid].max(), margin[b])
    mpc.close()


def test_predictor_is_second_order(pkg, tables, gpu_lib):
    M = 64
    rng = np.random.default_rng(5)
    x0 = pkg.sample_x0(tables, M, seed=21)
    scale = 0.02 * np.array([0.5, 0.05, 0.01, 0.2, 0.02, 0.02, 0.005, 0.02])  # small enough that no bound changes sides
    d = rng.normal(size=(M, 8)) * scale
    mpc = pkg.BatchedMPC(tables, 20, 3 * M)
    mpc.set_initial_guess(np.vstack([x0, x0, x0]))
    u = mpc.make_step(np.vstack([x0, x0 + d, x0 + 0.5 * d]))
    S = mpc.sensitivities()
    st = mpc.stats()
    u0, u1, uh = u[:M], u[M:2 * M], u[2 * M:]
    J = S["du0_dx0"][:M]
    e1 = np.abs(u1 - (u0 + np.einsum("bij,bj->bi", J, d))).max(axis=1)
    eh = np.abs(uh - (u0 + np.einsum("bij,bj->bi", J, 0.5 * d))).max(axis=1)
    move = np.abs(u1 - u0).max(axis=1)
    conv = (st["status_solver"][:M] == 0) & (st["status_solver"][M:2 * M] == 0) & (st["status_solver"][2 * M:] == 0)
    # the same inputs at their bounds in the three solves: across a change of the active set the predictor is first order only
    p = mpc.params
    lo, hi = np.array([p.u_lb[0], p.u_lb[1]]), np.array([p.u_ub[0], p.u_ub[1]])
    act = [(np.abs(v - lo) < 1e-6) | (np.abs(v - hi) < 1e-6) for v in (u0, u1, uh)]
    same = (act[0] == act[1]).all(axis=1) & (act[0] == act[2]).all(axis=1)
    # (errors above 1e-7: well clear of the solves' own accuracy, ~1e-9 in u0)
    use = S["ok"][:M] & (S["margin"][:M] >= 1e-3) & conv & same & (eh > 1e-7) & (e1 > 1e-7)
    ratio = e1[use] / eh[use]
    _log("sens_second_order", f"used {use.sum()} ratio {np.round(np.sort(ratio), 3).tolist()} err/move {np.round(np.sort(e1[use] / move[use]), 4).tolist()}")
    assert use.sum() >= 8, use.sum()
    # measured: 7 of 9 in 3.8 .. 4.3; the other two (16, 56) have the largest errors of the set: the full step crosses a kink
    # of a track constraint, which the input-bound filter above does not see - hence a floor of 0.75, not 1
    _rate("sens_second_order_ratio_in_3_5", np.mean((ratio >= 3.0) & (ratio <= 5.0)), 0.75)
    assert (e1[use] / move[use] < 0.05).all(), e1[use] / move[use]
    mpc.close()


def test_feedback_is_the_tangential_predictor(pkg, tables, gpu_lib):
    x0 = pkg.sample_x0(tables, 8, seed=9)
    mpc = pkg.BatchedMPC(tables, 10, 8)
    mpc.set_initial_guess(x0)
    u0 = mpc.make_step(x0)
    S = mpc.sensitivities()
    dx = (x0 + 1e-3) - x0
    fb = mpc.feedback(x0 + 1e-3)
    want = np.where(S["ok"][:, None], u0 + np.einsum("bij,bj->bi", S["du0_dx0"], dx), u0)
    assert np.array_equal(fb, want)
    assert np.array_equal(mpc.feedback(x0), u0)
    # the next tick: u_prev of that solve was u0
    u1 = mpc.make_step(x0)
    S1 = mpc.sensitivities()
    fb1 = mpc.feedback(x0, u_prev=u0 + 1e-3)
    want1 = np.where(S1["ok"][:, None], u1 + np.einsum("bij,bj->bi", S1["du0_duprev"], np.full((8, 2), 1e-3)), u1)
    assert np.allclose(fb1, want1, rtol=0, atol=1e-14)
    mpc.close()


def _solve_sens(pkg, tables, x, N, width=None, trajectory=False):
    mpc = pkg.BatchedMPC(tables, N, x.shape[0])
    if width is not None:
        mpc.set_narrow_width(width)
    mpc.set_initial_guess(x)
    u = mpc.make_step(x)
    S = mpc.sensitivities(trajectory)
    mpc.close()
    return u, S


def _same(S, T, keys=("du0_dx0", "du0_duprev", "ok", "margin")):
    for k in keys:
        assert np.array_equal(S[k], T[k]), k


def test_scheduling_only(pkg, tables, gpu_lib):
    import torch
    x = _x0_batch(pkg, tables, 64, seed=31)
    # narrow widths
    runs = [_solve_sens(pkg, tables, x, 40, w) for w in (0, 64, 512)]
    for u, S in runs[1:]:
        assert np.array_equal(u, runs[0][0])
        _same(S, runs[0][1])
    # alone and inside the batch
    for b in (0, 7, 33):
        u, S = _solve_sens(pkg, tables, x[b:b + 1], 40)
        assert np.array_equal(u[0], runs[0][0][b])
        _same(S, {k: v[b:b + 1] for k, v in runs[0][1].items()})
    # re-packed (warm ticks at 1024 instances) against the same ticks unpacked
    X = _x0_batch(pkg, tables, 1024, seed=32)
    res = []
    for pack in ("1", "0"):
        os.environ["LTOMPC_PACK"] = pack
        try:
            mpc = pkg.BatchedMPC(tables, 10, X.shape[0])
        finally:
            os.environ.pop("LTOMPC_PACK", None)
        mpc.set_initial_guess(X)
        for _ in range(3):
            u = mpc.make_step(X)
        res.append((u, mpc.sensitivities(True)))
        mpc.close()
    assert np.array_equal(res[0][0], res[1][0])
    _same(res[0][1], res[1][1], ("du0_dx0", "du0_duprev", "ok", "margin", "dX", "dU"))
    # SplitMPC, 1 and 4 parts; host and device entry points
    dev = torch.device("cuda", 0)
    Y = _x0_batch(pkg, tables, 512, seed=33)
    out = []
    for parts in (1, 4):
        sp = pkg.SplitMPC(tables, 10, Y.shape[0], n_parts=parts)
        xa = torch.from_numpy(Y).to(dev)
        ua = torch.zeros(Y.shape[0], 2, dtype=torch.float64, device=dev)
        sp.set_initial_guess_dev(xa.data_ptr())
        sp.make_step_dev(xa.data_ptr(), ua.data_ptr())
        sp.synchronize()
        S = sp.sensitivities()
        g = torch.zeros(Y.shape[0], 2, 10, dtype=torch.float64, device=dev)
        ok = torch.zeros(Y.shape[0], dtype=torch.int32, device=dev)
        sp.sensitivities_dev(g.data_ptr(), ok.data_ptr())
        sp.synchronize()
        assert np.array_equal(g.cpu().numpy(), _du0(S)) and np.array_equal(ok.cpu().numpy() != 0, S["ok"])
        out.append((ua.cpu().numpy(), S))
        sp.close()
    assert np.array_equal(out[0][0], out[1][0])
    _same(out[0][1], out[1][1])


def _tick_record(mpc, u, x):
    X, U = mpc.prediction()
    it = mpc.iterate()
    return [u, mpc.status.copy(), mpc.iters.copy(), X, U] + [it[k] for k in sorted(it)]


def test_no_side_effects(pkg, tables, gpu_lib):
    import torch
    x = _x0_batch(pkg, tables, 600, seed=41)
    a, b = pkg.BatchedMPC(tables, 10, x.shape[0]), pkg.BatchedMPC(tables, 10, x.shape[0])
    dev = torch.device("cuda", 0)
    g = torch.zeros(x.shape[0], 2, 10, dtype=torch.float64, device=dev)
    ok = torch.zeros(x.shape[0], dtype=torch.int32, device=dev)
    xa, xb = x.copy(), x.copy()
    a.set_initial_guess(xa), b.set_initial_guess(xb)
    for tick in range(6):
        ua, ub = a.make_step(xa), b.make_step(xb)
        b.sensitivities(trajectory=True)
        b.sensitivities_dev(g.data_ptr(), ok.data_ptr())
        b.synchronize()
        ra, rb = _tick_record(a, ua, xa), _tick_record(b, ub, xb)
        for i, (p, q) in enumerate(zip(ra, rb)):
            assert np.array_equal(p, q), (tick, i)
        xa, xb = a.plant_step(xa, ua, 50), b.plant_step(xb, ub, 50)
    a.close(), b.close()
    # after a closed-loop rollout (thread-per-slot evaluation: more than 64 instances)
    x = _x0_batch(pkg, tables, 128, seed=42)
    a, b = pkg.BatchedMPC(tables, 10, x.shape[0]), pkg.BatchedMPC(tables, 10, x.shape[0])
    ta, tb = torch.from_numpy(x).to(dev), torch.from_numpy(x).to(dev)
    for m, t in ((a, ta), (b, tb)):
        m.set_initial_guess(x)
        m.rollout_dev(t.data_ptr(), 2, 50)
    S = b.sensitivities(trajectory=True)
    assert S["ok"].mean() > 0.5
    xs = ta.cpu().numpy()
    assert np.array_equal(xs, tb.cpu().numpy())
    ua, ub = a.make_step(xs), b.make_step(xs)
    for i, (p, q) in enumerate(zip(_tick_record(a, ua, xs), _tick_record(b, ub, xs))):
        assert np.array_equal(p, q), i
    a.close(), b.close()


def test_edge_cases(pkg, tables, orc, gpu_lib):
    import ctypes as C
    L = gpu_lib
    x = _x0_batch(pkg, tables, 16, seed=51)
    mpc = pkg.BatchedMPC(tables, 10, x.shape[0])
    # before any solve, and after an initial guess: a usage error, not a crash
    with pytest.raises(pkg.LtompcError):
        mpc.sensitivities()
    assert L.ltompc_sensitivities_dev(mpc._h, None, None) != 0
    mpc.set_initial_guess(x)
    u = mpc.make_step(x)
    assert L.ltompc_get_sensitivities(mpc._h, None, None, None, None, None) == 0
    assert L.ltompc_sensitivities_dev(mpc._h, None, None) == 0
    mpc.synchronize()
    S = mpc.sensitivities(trajectory=True)
    ok = S["ok"]
    assert ok.mean() >= 0.75, ok
    G = _du0(S)
    eye = np.zeros((8, 10)); eye[:, :8] = np.eye(8)
    assert (S["dX"][ok, 0] == eye).all()
    assert np.array_equal(S["dU"][:, 0], G)
    mpc.set_initial_guess(x)
    with pytest.raises(pkg.LtompcError):
        mpc.sensitivities()
    mpc.close()
    # an instance far off the track: the solver reports it INFEASIBLE, ok = 0 and exact zeros; its neighbours unaffected
    y = x.copy()
    y[4, 1] += 40.0
    m2 = pkg.BatchedMPC(tables, 10, y.shape[0])
    m2.set_initial_guess(y)
    m2.make_step(y)
    T = m2.sensitivities(trajectory=True)
    sst = m2.stats()["status_solver"]
    m2.close()
    assert sst[4] not in (0, 1), sst[4]
    bad = ~np.isin(sst, (0, 1))
    assert not T["ok"][bad].any()
    for k in ("du0_dx0", "du0_duprev", "margin", "dX", "dU"):
        assert (T[k][bad] == 0).all(), k
    others = np.setdiff1d(np.arange(y.shape[0]), [4])
    for k in ("du0_dx0", "du0_duprev", "ok", "margin", "dX", "dU"):
        assert np.array_equal(T[k][others], S[k][others]), k
    # soft track constraints (soft_rho = 100): the same check against central differences on a few instances
    o = pkg.default_options()
    o.soft_rho = 100.0
    oo = orc.default_options()
    oo.soft_rho = 100.0
    z = x[:6]
    ms, uz, Sz, stz = _gpu(pkg, tables, z, 10, options=o)
    fd, base, fd_solved = _central_differences(orc, tables, z, 10, options=oo)
    use = Sz["ok"] & (Sz["margin"] >= 1e-3) & (stz["status_solver"] == 0) & (base["status_solver"] == 0) & fd_solved & \
        (np.abs(uz - base["u0"]).max(axis=1) < 1e-6)
    assert use.sum() >= 3, use
    err = (np.abs(_du0(Sz) - fd) / np.maximum(1.0, np.abs(_du0(Sz)))).max(axis=(1, 2))
    _log("sens_fd_soft", f"used {use.sum()} err {err[use].tolist()}")
    assert (err[use] <= _tol(Sz["margin"][use])).all(), err[use]
    ms.close()
