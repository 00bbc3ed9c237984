"""Reference for the directional sensitivities (ltompc_get_jvp): the Jacobians of the predicted trajectory
w.r.t. (x0, u_prev) and theta times one direction v = (dp (10,), dtheta (16,)).

    contract(q, dp, dth)  the definition: the forward Jacobians of param_sens_reference.param_sensitivities_batch (dX, dU, dX_p,
                          dU_p of one instance, q) contracted with the direction
    jvp_batch(...)        linearity, without the Jacobians: with A the KKT matrix of sens_reference and A w_j = b_j the forward
                          columns (b_j = -F_p or -F_theta), ONE solve  A w = sum_j b_j v_j  with the v-weighted right-hand side
                          (the r_du columns of F_theta enter it with dtheta[14], dtheta[15] like every other column); block 0 of
                          tX is dp[0..7] (block 0 of dX_dp is [I | 0], of dX_dth 0).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse.linalg as spla

import param_sens_reference as PR
import sens_reference as SR

NT = PR.NT


def contract(q, dp, dth):
    """(tX (N+1,8), tU (N,2)) of one instance from its forward Jacobians q and the direction."""
    return q["dX_p"] @ dp + q["dX"] @ dth, q["dU_p"] @ dp + q["dU"] @ dth


def contraction_scale(q, dp, dth, theta):
    """sum_j max(1, |D_e,j| s_j) / s_j |v_j| per element e (s_j = 1 for p, |theta_j| for theta): what a relative error `gap` of
    the Jacobians' entries (measured as |d64 - d| s / max(1, |d| s), sens_reference) can move the contraction by."""
    th = np.abs(theta)
    sX = np.maximum(1.0, np.abs(q["dX_p"])) @ np.abs(dp) + np.maximum(1.0, np.abs(q["dX"]) * th) @ (np.abs(dth) / th)
    sU = np.maximum(1.0, np.abs(q["dU_p"])) @ np.abs(dp) + np.maximum(1.0, np.abs(q["dU"]) * th) @ (np.abs(dth) / th)
    return sX, sU


def jvp_batch(it, x0, uprev, tab, eps, params, dp, dth, refine=3, h=0.1, forward=None):
    """For each of M instances a dict tX (N+1,8), tU (N,2), q (the forward reference of the instance, with its gap).
    dp (M,10), dth (M,16).  forward: param_sensitivities_batch of the same arguments when the caller has it already."""
    fwd = forward if forward is not None else PR.param_sensitivities_batch(it, x0, uprev, tab, eps, params, refine, h)
    FT, GT = PR.theta_blocks(it, x0, uprev, tab, eps, params, h)
    out = []
    for m, q in enumerate(fwd):
        N = FT.shape[1]
        idx, nz = SR._index(N)
        Fz = np.zeros((nz, NT))
        np.add.at(Fz, idx.ravel(), FT[m].reshape(N * SR.NV, NT))
        wi = np.arange(8, nz - 2)
        A = q["base"]["kkt"]
        Bm = np.hstack([q["base"]["rhs"], -np.vstack([Fz[wi], GT[m].reshape(16 * N, NT)])])  # the forward right-hand sides
        v = np.concatenate([np.asarray(dp[m], float), np.asarray(dth[m], float)])
        c = np.asarray((Bm.astype(np.longdouble) * v.astype(np.longdouble)[None, :]).sum(axis=1), dtype=np.float64)  # ONE right-hand side
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A")
        y = lu.solve(c).astype(np.longdouble)[:, None]
        cl = c.astype(np.longdouble)[:, None]
        for _ in range(refine):
            r = cl - SR._matvec_ld(A, y)
            y = y + lu.solve(np.asarray(r[:, 0], dtype=np.float64))[:, None]
        w = np.asarray(y[:, 0], dtype=np.float64)
        tX = np.zeros((N + 1, 8))
        tX[0] = np.asarray(dp[m], float)[:8]
        tX[1:] = w[:8 * N].reshape(N, 8)
        out.append(dict(tX=tX, tU=w[16 * N:18 * N].reshape(N, 2).copy(), q=q))
    return out
