"""The directional identity pinned without a GPU and without a kernel: at oracle iterates, ONE dense solve with
the v-weighted right-hand side (jvp_reference.jvp_batch) reproduces the contraction of the forward Jacobians of
param_sens_reference with the same direction (jvp_reference.contract): the combined right-hand side, the signs of the r_du
columns' terms included."""
import numpy as np
import pytest

import jvp_reference as JR
import param_sens_reference as PR
from test_sens_reference import KEYS, _x0_batch


@pytest.mark.parametrize("N,B", [(2, 5), (10, 4)])
def test_one_weighted_solve_reproduces_the_contracted_forward_jacobians(pkg, tables, oracle, N, B):
    """Directions with dp of O(1) and dtheta a change of up to 5 % of every parameter; the r_du columns alone; dp alone (block 0
    comes back as it is).

    Bound.  Both sides solve with the same LU and refine in extended precision; what separates them is the error of that LU,
    which the forward reference reports as `gap` (unrefined against refined solve, per entry relative to max(1, |d| s)).  An
    error of that size in every entry moves element e of the contraction by at most gap * sum_j max(1, |D_e,j| s_j) / s_j |v_j|
    (contraction_scale).  gap is floored by the rounding of a float64 sum of 26 terms, 26 2^-52."""
    x = _x0_batch(pkg, tables, B, seed=17 + N)
    r = oracle.solve(x, N)
    assert (r["status_solver"] <= 1).sum() >= B - 1
    params = pkg.default_params()
    eps = oracle.o.smooth_eps_min
    it = {k: r[k] for k in KEYS}
    up = np.zeros((B, 2))
    th = PR.theta_values(params)
    rng = np.random.default_rng(5 + N)
    dp, dth = rng.standard_normal((B, 10)), rng.uniform(-0.05, 0.05, (B, 16)) * th
    only_r = np.zeros_like(dth)
    only_r[:, 14:] = dth[:, 14:]
    fwd = PR.param_sensitivities_batch(it, x, up, tables, eps, params)
    worst = 0.0
    for label, p, t in (("both", dp, dth), ("r_du", np.zeros_like(dp), only_r), ("dp", dp, np.zeros_like(dth))):
        got = JR.jvp_batch(it, x, up, tables, eps, params, p, t, forward=fwd)
        for b, (a, q) in enumerate(zip(got, fwd)):
            tX, tU = JR.contract(q, p[b], t[b])
            sX, sU = JR.contraction_scale(q, p[b], t[b], th)
            tol = max(q["gap"], 26 * 2.0 ** -52)
            eX, eU = np.abs(a["tX"] - tX) / np.where(sX > 0, sX, 1.0), np.abs(a["tU"] - tU) / np.where(sU > 0, sU, 1.0)
            worst = max(worst, eX.max() / tol, eU.max() / tol)
            assert (eX <= tol).all(), (label, b, eX.max(), tol)
            assert (eU <= tol).all(), (label, b, eU.max(), tol)
            assert np.abs(tU).max() > 0, (label, b)
            assert np.array_equal(a["tX"][0], p[b, :8]), (label, b)
    print(f"N {N}: largest error / bound {worst:.3g}")
