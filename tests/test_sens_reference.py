"""The dense sensitivity reference (sens_reference.py) pinned without a GPU: its Hessian and Jacobian blocks against the
oracle's own forward-mode jets, its plane layout and inertia test, and its derivatives against central differences of oracle
re-solves at every stage of the horizon."""
import numpy as np
import pytest

import sens_reference as SR

H_ABS = 1e-6
KEYS = ("X", "C", "U", "L1", "L2", "T", "NU")


def _x0_batch(pkg, tables, n, seed):
    """X0_REFERENCE, sampled states, and every fifth sampled state moved next to the right-hand edge of the band."""
    x = np.vstack([pkg.X0_REFERENCE[None], pkg.sample_x0(tables, n - 1, seed=seed)])
    s = x[5::5, 0]
    nl, nr = np.interp(s, tables.s_arc, tables.n_left), np.interp(s, tables.s_arc, tables.n_right)
    mid, w = 0.5 * (nl - nr), 0.5 * (nl + nr - 2.3)
    x[5::5, 1] = mid - 0.97 * w
    return x


def _close(a, b, tol=1e-10):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("eps", [1e-4, 0.0])
def test_stage_blocks_match_the_oracle_jets(pkg, tables, oracle, eps):
    """The torch restatement's blocks at oracle solutions against rhs_derivs / cost_derivs / cons_derivs, to 1e-10."""
    N = 10
    x = _x0_batch(pkg, tables, 6, seed=3)
    r = oracle.solve(x, N)
    params = pkg.default_params()
    nb = len(SR.bound_rows(params))
    blk = SR.stage_blocks({k: r[k] for k in KEYS}, x, np.zeros((6, 2)), tables, eps, params)
    h = oracle.o.t_step
    for b in range(6):
        X, C, L1, L2, NU = r["X"][b].copy(), r["C"][b], r["L1"][b], r["L2"][b], r["NU"][b]
        X[0] = x[b]
        for k in (0, 1, 5, N - 2, N - 1):
            H, JG, Jnl = blk["H"][b, k], blk["JG"][b, k], blk["Jnl"][b, k]
            c, xk, xp = slice(SR.SC, SR.SC + 8), slice(SR.SX, SR.SX + 8), slice(SR.SXP, SR.SXP + 8)
            _, fc, Hc = oracle.rhs_derivs(C[k], L1[k], eps)
            assert _close(H[c, c], h * Hc), (b, k)
            assert _close(JG[:8, c], h * fc - 1.5 * np.eye(8)) and _close(JG[8:, c], 4.5 * np.eye(8)), (b, k)
            assert _close(H[xk, xk], oracle.cost_derivs(X[k], False, eps)[2]), (b, k)
            _, fp, Hp = oracle.rhs_derivs(X[k + 1], L2[k], eps)
            want = h * Hp
            v, g, Hg = oracle.cons_derivs(X[k + 1], eps)
            if k < N - 1:
                want = want + np.einsum("q,qij->ij", NU[k, nb:nb + 3], Hg)
                assert _close(Jnl[:, xp], g), (b, k)
            else:
                want = want + oracle.cost_derivs(X[N], True, eps)[2]
            assert _close(H[xp, xp], want), (b, k)
            assert _close(JG[8:, xp], h * fp - 2.5 * np.eye(8)), (b, k)
            # the Delta-u term: 2 r on u_k, -2 r against u_{k-1} (u_prev at k = 0)
            r2 = 2 * np.array(params.r_du)
            assert _close(H[SR.SU:SR.SU + 2, SR.SUM:SR.SUM + 2], -np.diag(r2)), (b, k)


def test_layout_and_inertia(pkg, tables, oracle):
    """At SOLVED oracle iterates: T = -h(w) on every constraint row (the plane mapping of the inequalities), and the
    reference's inertia verdict against the eigenvalues of the whole KKT matrix."""
    N = 10
    x = _x0_batch(pkg, tables, 8, seed=5)
    r = oracle.solve(x, N)
    params = pkg.default_params()
    eps = oracle.o.smooth_eps_min
    use = np.flatnonzero(r["status_solver"] == 0)
    assert use.size >= 6
    R = SR.sensitivities_batch({k: r[k][use] for k in KEYS}, x[use], np.zeros((use.size, 2)), tables, eps, params)
    for b, q in zip(use, R):
        hv = SR.inequality_values({k: r[k][b] for k in ("X", "C", "U")}, x[b], tables, eps, params)
        m = ~np.isnan(hv)
        assert np.abs(r["T"][b][m] + hv[m]).max() <= 1e-7, b
        ev = np.linalg.eigvalsh(q["kkt"].toarray())
        assert ((ev > 0).sum() == q["n_w"] and (ev < 0).sum() == q["n_lambda"]) == q["ok_expected"], b
        assert q["backward"] < 1e-16 and q["gap"] < 1e-6, (b, q["backward"], q["gap"])
        assert (q["dX"][0] == np.eye(8, 10)).all()


def _differences(oracle, r, x, N):
    """Central differences at h and 10 h and one-sided differences at h of the oracle's U and X w.r.t. p = (x0, u_prev),
    warm-started from the solve at p: dict of (B, N, 2, 10) / (B, N+1, 8, 10) arrays, and whether every solve ended SOLVED."""
    B = x.shape[0]
    warm = {k: np.repeat(r[k], 10, 0) for k in ("X", "C", "U", "L1", "L2")}
    out, solved = {}, r["status_solver"] == 0
    for h in (H_ABS, 10 * H_ABS):
        res = []
        for sgn in (1.0, -1.0):
            X, U = np.repeat(x, 10, 0), np.zeros((B * 10, 2))
            for j in range(10):
                if j < 8:
                    X[j::10, j] += sgn * h
                else:
                    U[j::10, j - 8] += sgn * h
            q = oracle.solve(X, N, uprev=U, warm=warm, prev_status=np.repeat(r["status_solver"], 10))
            solved &= (q["status_solver"].reshape(B, 10) == 0).all(axis=1)
            res.append({k: q[k].reshape(B, 10, *q[k].shape[1:]).transpose(0, 2, 3, 1) for k in ("U", "X")})
        for k in ("U", "X"):
            out[k, h] = (res[0][k] - res[1][k]) / (2 * h)
            if h == H_ABS:
                base = r[k][..., None]
                out[k, "fwd"], out[k, "bwd"] = (res[0][k] - base) / h, (base - res[1][k]) / h
    return out, solved


@pytest.mark.parametrize("N,B", [(10, 24), (40, 12)])
def test_dense_reference_matches_central_differences_at_every_stage(pkg, tables, oracle, N, B):
    """At oracle solutions, dX and dU at every stage against central differences (h = 1e-6) wherever the solution is
    differentiable at the scale of the step and the differences are accurate: central differences at h and 10 h agree to
    1e-5 (the existing filter, tightened) and no direction has a kink at p (forward and backward differences agree).  Bound: 1e-4 + mu / margin^2 as in
    tests/test_gpu_sensitivity.py."""
    x = _x0_batch(pkg, tables, B, seed=11 + N)
    r = oracle.solve(x, N)
    fd, solved = _differences(oracle, r, x, N)
    params = pkg.default_params()
    eps = oracle.o.smooth_eps_min
    use = np.flatnonzero(solved)
    assert (oracle.o.smooth_scale * r["mu"][use] <= eps).all()
    assert use.size >= 0.7 * B, use.size
    R = SR.sensitivities_batch({k: r[k][use] for k in KEYS}, x[use], np.zeros((use.size, 2)), tables, eps, params)
    checked, worst = 0, 0.0
    for b, q in zip(use, R):
        tol = 1e-4 + max(r["mu"][b], 1e-9) / q["margin"] ** 2
        # a direction j in which the solution map has a kink at p (one-sided differences disagree anywhere on the horizon)
        # has no derivative; the barrier derivative is a smoothed value there along the whole trajectory
        kink = np.zeros(10, dtype=bool)
        for k in ("U", "X"):
            sc = np.maximum(1.0, np.abs(fd[k, H_ABS][b]))
            kink |= (np.abs(fd[k, "fwd"][b] - fd[k, "bwd"][b]) / sc > 1e-2).any(axis=(0, 1))
        for k, D in (("U", q["dU"]), ("X", q["dX"])):
            F, F10 = fd[k, H_ABS][b], fd[k, 10 * H_ABS][b]
            smooth = (np.abs(F - F10) / np.maximum(1.0, np.abs(F)) <= 1e-5) & ~kink
            e = np.abs(D - F) / np.maximum(1.0, np.abs(D))
            assert not smooth.any() or e[smooth].max() <= tol, (b, k, e[smooth].max(), tol, np.unravel_index(np.argmax(np.where(smooth, e, 0)), e.shape))
            checked += smooth.sum()
            worst = max(worst, (e[smooth] / tol).max(initial=0.0))
    # (measured: 13.5 % of the entries at N = 10, 36 % at N = 40 are accurate enough to check, largest error 0.12 resp.
    #  0.064 of the bound.  At h = 1e-6 the differences carry ~1e-5 of rounding noise from the solves' own accuracy, and the
    #  1e-5 agreement between h and 10 h keeps only the entries where the reference itself is good to well below 1e-4.)
    print(f"N {N}: checked fraction {checked / (use.size * (N * 2 + (N + 1) * 8) * 10):.3f}, largest err / tol {worst:.3g}")
    assert checked >= 0.1 * use.size * (N * 2 + (N + 1) * 8) * 10, checked / (use.size * (N * 2 + (N + 1) * 8) * 10)
    if N == 10:
        # DESIGN.md §9's open point: X0_REFERENCE's throttle reaches its bound exactly at node 9 (x0[7] + 9 h = 1), so the
        # solution map has a kink at p in the direction of x0[7].  The central difference averages the one-sided slopes
        # (-9.9 and -0.12 at stage 8), nearly the same at h and 10 h (0.2 %); the barrier derivative lies in between.
        assert use[0] == 0
        F, D = fd["U", H_ABS][0, 8, 1, 7], R[0]["dU"][8, 1, 7]
        assert abs(F - fd["U", 10 * H_ABS][0, 8, 1, 7]) < 5e-3 * abs(F) and abs(D - F) > 0.1
        assert abs(fd["U", "fwd"][0, 8, 1, 7] - fd["U", "bwd"][0, 8, 1, 7]) > 5.0
        assert min(fd["U", "fwd"][0, 8, 1, 7], fd["U", "bwd"][0, 8, 1, 7]) < D < max(fd["U", "fwd"][0, 8, 1, 7], fd["U", "bwd"][0, 8, 1, 7])
