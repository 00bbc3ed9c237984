"""The dense parameter-sensitivity reference (param_sens_reference.py) pinned without a GPU: its x0 / u_prev columns against
sens_reference, and its theta columns against central differences of oracle re-solves with perturbed Params."""
import numpy as np
import pytest

import nlp_reference as R
import param_sens_reference as PR
import sens_reference as SR
from test_sens_reference import KEYS, _x0_batch

H_REL = 1e-6  # step of theta_j: H_REL |theta_j| (every default theta_j is non-zero)


def test_p_columns_reproduce_sens_reference_and_P_is_restored(pkg, tables, oracle):
    N = 10
    x = _x0_batch(pkg, tables, 6, seed=3)
    r = oracle.solve(x, N)
    params = pkg.default_params()
    eps = oracle.o.smooth_eps_min
    P0 = dict(R.P)
    it = {k: r[k] for k in KEYS}
    ref = SR.sensitivities_batch(it, x, np.zeros((6, 2)), tables, eps, params)
    got = PR.param_sensitivities_batch(it, x, np.zeros((6, 2)), tables, eps, params)
    assert R.P == P0 and all(type(v) is type(P0[k]) for k, v in R.P.items())
    for a, b in zip(got, ref):
        assert np.abs(a["dX_p"] - b["dX"]).max() <= 1e-12 * max(1.0, np.abs(b["dX"]).max())
        assert np.abs(a["dU_p"] - b["dU"]).max() <= 1e-12 * max(1.0, np.abs(b["dU"]).max())
        assert (a["dX"][0] == 0).all() and a["dX"].shape == (N + 1, 8, 16) and a["dU"].shape == (N, 2, 16)
        assert a["backward"] < 1e-16


def _theta_differences(orc, tables, x, r, N, base_params):
    """Central differences at h and 10 h of the oracle's U and X w.r.t. theta_j (h = H_REL |theta_j|), warm-started from the
    solve at theta: (B, N, 2, 16) / (B, N+1, 8, 16), and whether every solve of an instance ended SOLVED."""
    B = x.shape[0]
    th = PR.theta_values(base_params)
    warm = {k: r[k] for k in ("X", "C", "U", "L1", "L2")}
    out, solved = {}, r["status_solver"] == 0
    kink = {k: np.zeros(r[k].shape + (PR.NT,)) for k in ("U", "X")}  # |forward - backward difference| at h
    for f in (1.0, 10.0):
        D = {k: np.zeros(r[k].shape + (PR.NT,)) for k in ("U", "X")}
        for j in range(PR.NT):
            h = f * H_REL * abs(th[j])
            res = []
            for sgn in (1.0, -1.0):
                p = PR.set_theta(pkg_params_copy(base_params), j, th[j] + sgn * h)
                q = orc.Oracle(tables.packed(), params=p).solve(x, N, warm=warm, prev_status=r["status_solver"])
                solved &= q["status_solver"] == 0
                res.append(q)
            for k in ("U", "X"):
                D[k][..., j] = (res[0][k] - res[1][k]) / (2 * h)
                if f == 1.0:
                    kink[k][..., j] = np.abs((res[0][k] - r[k]) - (r[k] - res[1][k])) / h
        out[f] = D
    out["kink"] = kink
    return out, solved


def pkg_params_copy(p):
    q = type(p)()
    for name, _ in p._fields_:
        v = getattr(p, name)
        setattr(q, name, v if not hasattr(v, "_length_") else type(v)(*v))
    return q


@pytest.mark.parametrize("N,B", [(10, 24), (40, 12)])
def test_theta_columns_match_central_differences(pkg, tables, orc, oracle, N, B):
    """At oracle solutions, du0 and every stage of dX, dU w.r.t. theta against central differences of re-solves with perturbed
    Params, on instances whose solves all ended SOLVED and whose margin is >= 1e-3, entries where h and 10 h agree to 1e-5.
    Error measure: |G - D| |theta_j| / max(1, |D| |theta_j|); bound 1e-4 + mu / margin^2 as for x0 / u_prev."""
    x = _x0_batch(pkg, tables, B, seed=11 + N)
    r = oracle.solve(x, N)
    params = pkg.default_params()
    fd, solved = _theta_differences(orc, tables, x, r, N, params)
    eps = oracle.o.smooth_eps_min
    cand = np.flatnonzero(solved)
    R_ = PR.param_sensitivities_batch({k: r[k][cand] for k in KEYS}, x[cand], np.zeros((cand.size, 2)), tables, eps, params)
    th = PR.theta_values(params)
    used, checked, worst, cols = 0, 0, 0.0, np.zeros(PR.NT, dtype=int)
    for b, q in zip(cand, R_):
        if q["margin"] < 1e-3:
            continue
        used += 1
        tol = 1e-4 + max(r["mu"][b], 1e-9) / q["margin"] ** 2
        # a column in which the solution map has a kink at theta (one-sided differences disagree anywhere on the horizon) has
        # no derivative; the barrier derivative is a smoothed value there (as in test_sens_reference)
        kink = np.zeros(PR.NT, dtype=bool)
        for k in ("U", "X"):
            sc = np.maximum(1.0, np.abs(fd[1.0][k][b]) * th)
            kink |= (fd["kink"][k][b] * th / sc > 1e-2).reshape(-1, PR.NT).any(axis=0)
        for k, D in (("U", q["dU"]), ("X", q["dX"])):
            F, F10 = fd[1.0][k][b], fd[10.0][k][b]
            smooth = (np.abs(F - F10) * th / np.maximum(1.0, np.abs(F) * th) <= 1e-5) & ~kink
            e = PR.scaled_error(D, F)
            assert not smooth.any() or e[smooth].max() <= tol, (b, k, e[smooth].max(), tol,
                                                                np.unravel_index(np.argmax(np.where(smooth, e, 0)), e.shape))
            checked += smooth.sum()
            cols += smooth.reshape(-1, PR.NT).sum(axis=0)
            worst = max(worst, (e[smooth] / tol).max(initial=0.0))
    print(f"N {N}: {used} instances used, {checked} entries checked, per column {cols.tolist()}, largest err / tol {worst:.3g}")
    assert used >= 3, used
    assert (cols > 0).all(), cols  # every column is exercised
