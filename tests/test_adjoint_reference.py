"""The adjoint identity pinned without a GPU and without a kernel: at oracle iterates, ONE dense solve with the
cotangent as right-hand side, contracted with F_p and F_theta (adjoint_reference.adjoint_batch), reproduces the contraction of
the forward Jacobians of param_sens_reference with the same cotangent (adjoint_reference.contract)."""
import numpy as np
import pytest

import adjoint_reference as AR
import param_sens_reference as PR
from test_sens_reference import KEYS, _x0_batch


@pytest.mark.parametrize("N,B", [(2, 5), (10, 4)])
def test_one_adjoint_solve_reproduces_the_contracted_forward_jacobians(pkg, tables, oracle, N, B):
    """Dense random cotangents with entries O(1), and gX with only block 0 (which must come back in grad_x0 as it is).

    Bound.  Both sides solve with the same LU and refine in extended precision; what separates them is the error of that LU,
    which the forward reference reports as `gap` (unrefined against refined solve, per entry relative to max(1, |d| s)).  An
    error of that size in every entry moves column j of the contraction by at most gap * sum_e |g_e| max(1, |D_e,j| s_j) / s_j
    (contraction_scale).  gap is floored by the rounding of a float64 sum of n_e = 8 (N + 1) + 2 N terms, n_e 2^-52."""
    x = _x0_batch(pkg, tables, B, seed=17 + N)
    r = oracle.solve(x, N)
    assert (r["status_solver"] <= 1).sum() >= B - 1
    params = pkg.default_params()
    eps = oracle.o.smooth_eps_min
    it = {k: r[k] for k in KEYS}
    up = np.zeros((B, 2))
    rng = np.random.default_rng(5 + N)
    gX, gU = rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))
    fwd = PR.param_sensitivities_batch(it, x, up, tables, eps, params)
    got = AR.adjoint_batch(it, x, up, tables, eps, params, gX, gU, forward=fwd)
    th = PR.theta_values(params)
    n_e = 8 * (N + 1) + 2 * N
    worst = 0.0
    for b, (a, q) in enumerate(zip(got, fwd)):
        gp, gth = AR.contract(q, gX[b], gU[b])
        sp, st = AR.contraction_scale(q, gX[b], gU[b], th)
        tol = max(q["gap"], n_e * 2.0 ** -52)
        ep, et = np.abs(a["grad_p"] - gp) / sp, np.abs(a["grad_theta"] - gth) / st
        worst = max(worst, ep.max() / tol, et.max() / tol)
        assert (ep <= tol).all(), (b, ep.max(), tol)
        assert (et <= tol).all(), (b, et.max(), tol, int(np.argmax(et)))
        assert np.abs(gp).max() > 0 and np.abs(gth).max() > 0
    print(f"N {N}: largest error / bound {worst:.3g}")
    # block 0 alone: grad_x0 = gX[0], everything else 0 (dX block 0 is [I | 0] / 0 and the rest of the cotangent is 0)
    g0 = np.zeros_like(gX)
    g0[:, 0] = gX[:, 0]
    for b, a in enumerate(AR.adjoint_batch(it, x, up, tables, eps, params, g0, np.zeros_like(gU), forward=fwd)):
        assert np.array_equal(a["grad_p"][:8], gX[b, 0]) and (a["grad_p"][8:] == 0).all() and (a["grad_theta"] == 0).all(), b
