"""Reference for the parametric sensitivities (ltompc_get_sensitivities) without truncation error: at a given
primal-dual iterate, the implicit-function system of the barrier problem is assembled from the torch restatement of the NLP
(nlp_reference.py) and solved by a general sparse LU with iterative refinement.

Unknowns w = (x_1..x_N, c_0..c_{N-1}, u_0..u_{N-1}), equality multipliers (L1_k, L2_k) of the collocation rows G1_k, G2_k,
parameters p = (x0, u_prev).  With Sigma = NU / T on every inequality row (the barrier's primal-dual weights at the iterate)
and delta_w = 0:

    [[H_ww + Jh' Sigma Jh, Jg_w'], [Jg_w, 0]] [dw; dlambda] = -[H_wp; Jg_p]

(the inequalities do not involve p: node 0 has no bound or track row, so Jh_p = 0).  H is the Hessian of
J + L1'G1 + L2'G2 + NU'h, h the rows of nlp_reference.inequalities with the bound pattern of the params (NO_BOUND = no row);
the track rows of node N are not constraints.  None of the kernels' condensed formulas is used: the LU does the
elimination of the collocation variables, slacks and multipliers.

Stages are independent given their variables, so every stage's Hessian and Jacobian blocks come from one batched reverse
pass per row over all stages (the stage Lagrangians are summed; a row of all Hessian blocks is one more backward pass).
(torch.func's vmap cannot batch the tables' data-dependent interval search, hence plain autograd.)"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import nlp_reference as R

NO_BOUND = 1e30
NV = 28  # stage variables: x_k, c_k, u_k, x_{k+1}, u_{k-1}
SX, SC, SU, SXP, SUM = 0, 8, 16, 18, 26


def bound_rows(params):
    """(kind, index, sign, value) in the solver's order: u bounds, c bounds, x+ bounds; per variable lower then upper
    (ltompc_get_ineq: only the bounds that are set).  kind 0: u_k, 1: c_k, 2: x_{k+1}."""
    ub = [(i, s, v) for i in range(2) for s, v, on in ((-1.0, params.u_lb[i], params.u_lb[i] > -NO_BOUND),
                                                       (1.0, params.u_ub[i], params.u_ub[i] < NO_BOUND)) if on]
    xb = [(i, s, v) for i in range(8) for s, v, on in ((-1.0, params.x_lb[i], params.x_lb[i] > -NO_BOUND),
                                                       (1.0, params.x_ub[i], params.x_ub[i] < NO_BOUND)) if on]
    return [(0, *r) for r in ub] + [(1, *r) for r in xb] + [(2, *r) for r in xb]


def check_params(params):
    """nlp_reference models the default vehicle and cost; the bounds may differ."""
    P = R.P
    want = dict(mass=P["m"], inertia_z=P["Iz"], length_f=P["lf"], length_r=P["lr"], width=P["W"], B_f=P["Bf"], C_f=P["Cf"],
                D_f=P["Df"], B_r=P["Br"], C_r=P["Cr"], D_r=P["Dr"], C_m=P["Cm"], Cr_0=P["Cr0"], Cr_2=P["Cr2"],
                gravity=P["g"], q_n=P["q_n"], q_mu=P["q_mu"], q_B=P["q_B"], q_vy=1.0, q_v=1.0, vref_scale=0.6, ptv=0.0,
                ell_penalty=0.0)
    for k, v in want.items():
        assert getattr(params, k) == v, (k, getattr(params, k), v)
    assert tuple(params.r_du) == P["r"]


def _stage_functions(V, L1, L2, NUnl, last, nlmask, tab, eps, h):
    """Per-stage Lagrangian (N,), collocation rows (N,16) and track rows (N,3) at the stage variables V (N,28)."""
    xk, c, u, xp, um = V[:, SX:SX + 8], V[:, SC:SC + 8], V[:, SU:SU + 2], V[:, SXP:SXP + 8], V[:, SUM:SUM + 2]
    G1 = h * R.rhs(c, u, tab, eps) + 2 * xk - 1.5 * c - 0.5 * xp
    G2 = h * R.rhs(xp, u, tab, eps) - 2 * xk + 4.5 * c - 2.5 * xp
    g = R.cons(xp, tab, eps)
    r = torch.as_tensor(R.P["r"])
    L = R.lterm(xk, tab, eps) + (r * (u - um) ** 2).sum(-1) + (L1 * G1).sum(-1) + (L2 * G2).sum(-1) + \
        last * R.mterm(xp) + nlmask * (NUnl * g).sum(-1)
    return L, torch.cat([G1, G2], dim=-1), g


def _rows(F, V):
    """d F[:, i] / dV for every i: (N, F.shape[1], 28), one batched backward pass per row."""
    out = torch.zeros(V.shape[0], F.shape[1], V.shape[1], dtype=V.dtype)
    for i in range(F.shape[1]):
        gi = torch.autograd.grad(F[:, i].sum(), V, retain_graph=True, allow_unused=True)[0]
        if gi is not None:
            out[:, i] = gi
    return out


def stage_blocks(it, x0, uprev, tab, eps, params, h=0.1):
    """Stage blocks at the iterates `it` of M instances (X (M,N+1,8), C, U, L1, L2, T, NU; x0 (M,8), uprev (M,2)), all
    stages of all instances in one batch: Lagrangian Hessians (M,N,28,28) without the barrier term, collocation Jacobians
    (M,N,16,28), track Jacobians (M,N,3,28)."""
    X = torch.tensor(np.asarray(it["X"], float)).clone()
    M, N = X.shape[0], X.shape[1] - 1
    X[:, 0] = torch.as_tensor(np.asarray(x0, float).reshape(M, 8))
    C, U = torch.tensor(np.asarray(it["C"], float)), torch.tensor(np.asarray(it["U"], float))
    Um = torch.cat([torch.as_tensor(np.asarray(uprev, float)).reshape(M, 1, 2), U[:, :-1]], dim=1)
    V = torch.cat([X[:, :-1], C, U, X[:, 1:], Um], dim=2).reshape(M * N, NV).requires_grad_(True)
    nb = len(bound_rows(params))
    NUnl = torch.tensor(np.asarray(it["NU"], float)[:, :, nb:nb + 3]).reshape(M * N, 3)
    last = torch.zeros(M, N); last[:, N - 1] = 1.0
    last = last.reshape(M * N)
    nlmask = 1.0 - last  # the track rows of node N are not constraints
    L1, L2 = (torch.tensor(np.asarray(it[k], float)).reshape(M * N, 8) for k in ("L1", "L2"))
    L, G, g = _stage_functions(V, L1, L2, NUnl, last, nlmask, tab, eps, h)
    gL = torch.autograd.grad(L.sum(), V, create_graph=True)[0]
    out = dict(H=_rows(gL, V), JG=_rows(G, V), Jnl=_rows(g, V))
    return {k: v.numpy().reshape(M, N, -1, NV) for k, v in out.items()}


def inequality_values(it, x0, tab, eps, params):
    """h(w) (N, ni) in the solver's row order; the track rows of node N are nan (not constraints)."""
    X, C, U = (np.asarray(it[k], float) for k in ("X", "C", "U"))
    N = U.shape[0]
    cols = []
    for kind, i, s, v in bound_rows(params):
        z = U[:, i] if kind == 0 else (C[:, i] if kind == 1 else X[1:, i])
        cols.append(s * (z - v))
    g = R.cons(torch.tensor(X[1:]), tab, eps).numpy().copy()
    g[N - 1] = np.nan
    return np.concatenate([np.stack(cols, axis=1), g], axis=1)


def _index(N):
    """Global index of the stage variables (N,28) in z = (x_0..x_N, c_0..c_{N-1}, u_0..u_{N-1}, u_prev)."""
    oc, ou, op = 8 * (N + 1), 16 * N + 8, 18 * N + 8
    k = np.arange(N)[:, None]
    e8, e2 = np.arange(8)[None], np.arange(2)[None]
    um = np.where(k == 0, op + e2, ou + 2 * (k - 1) + e2)
    return np.concatenate([8 * k + e8, oc + 8 * k + e8, ou + 2 * k + e2, 8 * (k + 1) + e8, um], axis=1), op + 2


def _matvec_ld(A, x):
    """A x with the products and sums in extended precision (A csr, x (n, m))."""
    xl = np.asarray(x, dtype=np.longdouble)
    prod = A.data.astype(np.longdouble)[:, None] * xl[A.indices]
    return np.add.reduceat(prod, A.indptr[:-1], axis=0)


def sensitivities(it, x0, uprev, tab, eps, params, refine=3, h=0.1):
    """sensitivities_batch for one instance (arrays without the leading instance axis)."""
    one = {k: np.asarray(v)[None] for k, v in it.items()}
    return sensitivities_batch(one, np.asarray(x0)[None], np.asarray(uprev)[None], tab, eps, params, refine, h)[0]


def sensitivities_batch(it, x0, uprev, tab, eps, params, refine=3, h=0.1):
    """For each of M instances (it: X (M,N+1,8), C, U, L1, L2, T (M,N,>=ni), NU; x0 (M,8), uprev (M,2)) a dict with
    dX (N+1,8,10), dU (N,2,10), du0 (2,10) and the diagnostics:
    ok_expected  the KKT matrix has |w| positive and |lambda| negative eigenvalues (reduced Hessian positive definite)
    lam_min      smallest eigenvalue of the reduced Hessian on an orthonormal basis of the null space of Jg_w
    lam_scale    largest |eigenvalue| of the same (lam_min / lam_scale: how far from singular)
    backward     final relative backward error max |b - A x| / (|A| |x| + |b|) (infinity norms, per column)
    gap          max |d64 - d| / max(1, |d|) over dX, dU between the unrefined float64 solve d64 and the refined d
    margin       min over the constraint pairs of max(T, NU)"""
    check_params(params)
    blk = stage_blocks(it, x0, uprev, tab, eps, params, h)
    return [_solve(blk["H"][m], blk["JG"][m], blk["Jnl"][m], np.asarray(it["T"][m], float), np.asarray(it["NU"][m], float),
                   params, refine) for m in range(blk["H"].shape[0])]


def _solve(H, JG, Jnl, T, NU, params, refine):
    N = H.shape[0]
    rows = bound_rows(params)
    nb = len(rows)
    assert T.shape[1] >= nb + 3
    H = H.copy()
    # barrier term Jh' Sigma Jh, row by row: bounds (unit rows) and the track rows of nodes 1..N-1
    Sig = NU[:, :nb + 3] / T[:, :nb + 3]
    for m, (kind, i, s, v) in enumerate(rows):
        j = (SU, SC, SXP)[kind] + i
        H[:, j, j] += Sig[:, m]
    Jnl = Jnl.copy()
    Jnl[N - 1] = 0.0
    H += np.einsum("kqa,kq,kqb->kab", Jnl, Sig[:, nb:nb + 3], Jnl)
    idx, nz = _index(N)
    Hz = sp.coo_matrix((H.ravel(), (np.repeat(idx, NV, axis=1).ravel(), np.tile(idx, (1, NV)).ravel())), shape=(nz, nz)).tocsr()
    Gz = sp.coo_matrix((JG.ravel(), (np.repeat(np.arange(16 * N).reshape(N, 16), NV, axis=1).ravel(),
                                            np.tile(idx, (1, 16)).ravel())), shape=(16 * N, nz)).tocsr()
    pi = np.r_[np.arange(8), nz - 2, nz - 1]
    wi = np.arange(8, nz - 2)
    nw, nl = wi.size, 16 * N
    Hww, Hwp = Hz[wi][:, wi], Hz[wi][:, pi].toarray()
    Gw, Gp = Gz[:, wi], Gz[:, pi].toarray()
    A = sp.bmat([[Hww, Gw.T], [Gw, None]], format="csr")
    b = -np.vstack([Hwp, Gp])
    lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A")
    x64 = lu.solve(b)
    x = x64.astype(np.longdouble)
    for _ in range(refine):
        r = b.astype(np.longdouble) - _matvec_ld(A, x)
        x = x + lu.solve(np.asarray(r, dtype=np.float64))
    res = np.asarray(b.astype(np.longdouble) - _matvec_ld(A, x), dtype=np.float64)
    xs = np.asarray(x, dtype=np.float64)
    anorm = abs(A).sum(axis=1).max()
    backward = (np.abs(res).max(axis=0) / (anorm * np.abs(xs).max(axis=0) + np.abs(b).max(axis=0) + 1e-300)).max()

    def unpack(sol):
        dX = np.zeros((N + 1, 8, 10))
        dX[0, :, :8] = np.eye(8)
        dX[1:] = sol[:8 * N].reshape(N, 8, 10)
        dU = sol[16 * N:18 * N].reshape(N, 2, 10)
        return dX, dU

    dX, dU = unpack(xs)
    dX64, dU64 = unpack(x64)
    gap = max((np.abs(dX64 - dX) / np.maximum(1.0, np.abs(dX))).max(), (np.abs(dU64 - dU) / np.maximum(1.0, np.abs(dU))).max())
    # inertia: reduced Hessian on the null space of Jg_w, parametrised by the controls (w = (y, u), y = (x_1..x_N, c))
    Gy, Gu = Gw[:, :16 * N].tocsc(), Gw[:, 16 * N:].toarray()
    Z = np.vstack([-spla.splu(Gy, permc_spec="MMD_AT_PLUS_A").solve(Gu), np.eye(2 * N)])
    Q = np.linalg.qr(Z)[0]
    Rh = Q.T @ (Hww @ Q)
    ev = sla.eigvalsh(0.5 * (Rh + Rh.T))
    cons = np.ones_like(T[:, :nb + 3], dtype=bool)
    cons[N - 1, nb:] = False
    margin = np.maximum(T[:, :nb + 3], NU[:, :nb + 3])[cons].min()
    return dict(dX=dX, dU=dU, du0=dU[0], ok_expected=bool(ev[0] > 0.0), lam_min=float(ev[0]), lam_scale=float(np.abs(ev).max()),
                backward=float(backward), gap=float(gap), margin=float(margin), n_w=nw, n_lambda=nl, kkt=A, rhs=b)
