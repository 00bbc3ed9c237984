"""Reference for the adjoint sensitivities (ltompc_get_adjoint): the gradient of a loss of the predicted
trajectory w.r.t. (x0, u_prev) and theta from its cotangents gX (N+1,8), gU (N,2).

    contract(q, gX, gU)   the definition: the forward Jacobians of param_sens_reference.param_sensitivities_batch (dX, dU, dX_p,
                          dU_p of one instance, q) contracted with the cotangent
    adjoint_batch(...)    the symmetry identity, without the Jacobians: with A the (symmetric) KKT matrix of sens_reference and
                          A w_j = b_j the forward columns (b_j = -F_p or -F_theta), c the cotangent in the rows of
                          (x_1..x_N, c, u, lambda) = (gX[1:], 0, gU, 0):   c' w_j = c' A^-1 b_j = (A^-1 c)' b_j
                          - ONE solve with the cotangent as right-hand side, then a contraction with F_p and F_theta.  gX[0]
                          goes to grad_x0 directly (block 0 of dX_dp is [I | 0]).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse.linalg as spla

import param_sens_reference as PR
import sens_reference as SR

NT = PR.NT


def contract(q, gX, gU):
    """(grad_p (10,), grad_theta (16,)) of one instance from its forward Jacobians q and the cotangent."""
    gp = np.einsum("ki,kij->j", gX, q["dX_p"]) + np.einsum("kc,kcj->j", gU, q["dU_p"])
    gth = np.einsum("ki,kij->j", gX, q["dX"]) + np.einsum("kc,kcj->j", gU, q["dU"])
    return gp, gth


def contraction_scale(q, gX, gU, theta):
    """sum_e |g_e| max(1, |D_e,j| s_j) / s_j per column (s_j = 1 for p, |theta_j| for theta): what a relative error `gap` of
    the Jacobians' entries (measured as |d64 - d| s / max(1, |d| s), sens_reference) can move the contraction by."""
    th = np.abs(theta)
    sp = np.einsum("ki,kij->j", np.abs(gX), np.maximum(1.0, np.abs(q["dX_p"]))) + \
        np.einsum("kc,kcj->j", np.abs(gU), np.maximum(1.0, np.abs(q["dU_p"])))
    st = np.einsum("ki,kij->j", np.abs(gX), np.maximum(1.0, np.abs(q["dX"]) * th)) + \
        np.einsum("kc,kcj->j", np.abs(gU), np.maximum(1.0, np.abs(q["dU"]) * th))
    return sp, st / th


def adjoint_batch(it, x0, uprev, tab, eps, params, gX, gU, refine=3, h=0.1, forward=None):
    """For each of M instances a dict grad_p (10,), grad_theta (16,), q (the forward reference of the instance, with its gap).
    gX (M,N+1,8), gU (M,N,2).  forward: param_sensitivities_batch of the same arguments when the caller has it already."""
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
        c = np.zeros(A.shape[0])
        c[:8 * N] = np.asarray(gX[m], float)[1:].ravel()
        c[16 * N:18 * N] = np.asarray(gU[m], float).ravel()
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A")
        y = lu.solve(c).astype(np.longdouble)[:, None]
        cl = c.astype(np.longdouble)[:, None]
        for _ in range(refine):
            r = cl - SR._matvec_ld(A, y)
            y = y + lu.solve(np.asarray(r[:, 0], dtype=np.float64))[:, None]
        g = np.asarray((y[:, 0][:, None] * Bm.astype(np.longdouble)).sum(axis=0), dtype=np.float64)
        gp = g[:10].copy()
        gp[:8] += np.asarray(gX[m], float)[0]
        out.append(dict(grad_p=gp, grad_theta=g[10:], q=q))
    return out
