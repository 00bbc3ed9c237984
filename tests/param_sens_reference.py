"""Reference for the parameter sensitivities (ltompc_get_param_sensitivities) without truncation error: the
implicit-function system of sens_reference.py (same KKT matrix, same solver) with the right-hand side of the 16 vehicle and
cost parameters theta.

    [[H_ww + Jh' Sigma Jh, Jg_w'], [Jg_w, 0]] [dw; dlambda] = -[d(grad_w L)/dtheta; dG/dtheta]

(the inequalities do not involve theta: the geometry is not in theta).  F_theta comes from autograd through the torch
restatement (nlp_reference.py): its module dict P holds exactly these parameters, so they are replaced by per-stage tensor
copies for one batched pass and restored afterwards (other tests share P).  The x0 / u_prev columns are solved together with
the theta columns and must reproduce sens_reference.sensitivities."""
from __future__ import annotations

import numpy as np
import scipy.sparse.linalg as spla
import torch

import nlp_reference as R
import sens_reference as SR

NAMES = ("mass", "inertia_z", "B_f", "C_f", "D_f", "B_r", "C_r", "D_r", "C_m", "Cr_0", "Cr_2", "q_n", "q_mu", "q_B", "r_du[0]",
         "r_du[1]")
P_KEYS = ("m", "Iz", "Bf", "Cf", "Df", "Br", "Cr", "Dr", "Cm", "Cr0", "Cr2", "q_n", "q_mu", "q_B")  # then r = (r_du[0], r_du[1])
NT = len(NAMES)


def theta_values(params=None):
    """theta of a Params struct (default: nlp_reference's P, which check_params pins to the default vehicle)."""
    if params is None:
        return np.array([R.P[k] for k in P_KEYS] + list(R.P["r"]), dtype=float)
    return np.array([getattr(params, n) for n in NAMES[:-2]] + [params.r_du[0], params.r_du[1]], dtype=float)


def set_theta(params, j, value):
    """params with theta_j = value (in place)."""
    if j < NT - 2:
        setattr(params, NAMES[j], value)
    else:
        params.r_du[j - (NT - 2)] = value
    return params


def _rows_theta(F, Th):
    """d F[:, i] / d theta for every i, per stage: (S, F.shape[1], 16).  Stage s depends on row s of Th only."""
    out = torch.zeros(F.shape[0], F.shape[1], Th.shape[1], dtype=F.dtype)
    for i in range(F.shape[1]):
        gi = torch.autograd.grad(F[:, i].sum(), Th, retain_graph=True, allow_unused=True)[0]
        if gi is not None:
            out[:, i] = gi
    return out


def theta_blocks(it, x0, uprev, tab, eps, params, h=0.1):
    """Per stage of M instances: d(grad_V L)/dtheta (M,N,28,16) and d(G1, G2)/dtheta (M,N,16,16), V the stage variables of
    sens_reference (x_k, c_k, u_k, x_{k+1}, u_{k-1})."""
    SR.check_params(params)
    X = torch.tensor(np.asarray(it["X"], float)).clone()
    M, N = X.shape[0], X.shape[1] - 1
    X[:, 0] = torch.as_tensor(np.asarray(x0, float).reshape(M, 8))
    C, U = torch.tensor(np.asarray(it["C"], float)), torch.tensor(np.asarray(it["U"], float))
    Um = torch.cat([torch.as_tensor(np.asarray(uprev, float)).reshape(M, 1, 2), U[:, :-1]], dim=1)
    V = torch.cat([X[:, :-1], C, U, X[:, 1:], Um], dim=2).reshape(M * N, SR.NV).requires_grad_(True)
    nb = len(SR.bound_rows(params))
    NUnl = torch.tensor(np.asarray(it["NU"], float)[:, :, nb:nb + 3]).reshape(M * N, 3)
    last = torch.zeros(M, N)
    last[:, N - 1] = 1.0
    last = last.reshape(M * N)
    L1, L2 = (torch.tensor(np.asarray(it[k], float)).reshape(M * N, 8) for k in ("L1", "L2"))
    Th = torch.tensor(theta_values()).repeat(M * N, 1).requires_grad_(True)
    saved = dict(R.P)
    try:
        for i, key in enumerate(P_KEYS):
            R.P[key] = Th[:, i]
        R.P["r"] = Th[:, NT - 2:]
        L, G, _ = SR._stage_functions(V, L1, L2, NUnl, last, 1.0 - last, tab, eps, h)
        gL = torch.autograd.grad(L.sum(), V, create_graph=True)[0]
        FT, GT = _rows_theta(gL, Th), _rows_theta(G, Th)
    finally:
        R.P.clear()
        R.P.update(saved)
    return FT.detach().numpy().reshape(M, N, SR.NV, NT), GT.detach().numpy().reshape(M, N, 16, NT)


def param_sensitivities_batch(it, x0, uprev, tab, eps, params, refine=3, h=0.1):
    """For each of M instances a dict with dX (N+1,8,16), dU (N,2,16), du0 (2,16) w.r.t. theta (NAMES order), the same for
    p = (x0, u_prev) from the combined solve (dX_p, dU_p: (.., 10)), and sens_reference's diagnostics (ok_expected, margin,
    backward, gap: here over the theta columns, scaled by |theta_j|)."""
    base = SR.sensitivities_batch(it, x0, uprev, tab, eps, params, refine, h)
    FT, GT = theta_blocks(it, x0, uprev, tab, eps, params, h)
    th = np.abs(theta_values())
    out = []
    for m, q in enumerate(base):
        N = FT.shape[1]
        idx, nz = SR._index(N)
        Fz = np.zeros((nz, NT))
        np.add.at(Fz, idx.ravel(), FT[m].reshape(N * SR.NV, NT))
        wi = np.arange(8, nz - 2)
        A = q["kkt"]
        b = np.hstack([q["rhs"], -np.vstack([Fz[wi], GT[m].reshape(16 * N, NT)])])
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A")
        x64 = lu.solve(b)
        x = x64.astype(np.longdouble)
        for _ in range(refine):
            r = b.astype(np.longdouble) - SR._matvec_ld(A, x)
            x = x + lu.solve(np.asarray(r, dtype=np.float64))
        res = np.asarray(b.astype(np.longdouble) - SR._matvec_ld(A, x), dtype=np.float64)
        xs = np.asarray(x, dtype=np.float64)
        anorm = abs(A).sum(axis=1).max()
        backward = (np.abs(res).max(axis=0) / (anorm * np.abs(xs).max(axis=0) + np.abs(b).max(axis=0) + 1e-300)).max()

        def unpack(sol):
            dX = np.zeros((N + 1, 8, 10 + NT))
            dX[0, :, :8] = np.eye(8)
            dX[1:] = sol[:8 * N].reshape(N, 8, 10 + NT)
            return dX, sol[16 * N:18 * N].reshape(N, 2, 10 + NT)

        dX, dU = unpack(xs)
        dX64, dU64 = unpack(x64)
        sc = np.r_[np.ones(10), th]
        gap = max((np.abs(dX64 - dX) * sc / np.maximum(1.0, np.abs(dX) * sc)).max(),
                  (np.abs(dU64 - dU) * sc / np.maximum(1.0, np.abs(dU) * sc)).max())
        out.append(dict(dX=dX[..., 10:], dU=dU[..., 10:], du0=dU[0, :, 10:], dX_p=dX[..., :10], dU_p=dU[..., :10],
                        ok_expected=q["ok_expected"], margin=q["margin"], backward=float(backward), gap=float(gap),
                        base=q))
    return out


def scaled_error(G, D, theta=None):
    """§9's error measure per entry after scaling each theta column by |theta_j|: |G - D| |theta| / max(1, |D| |theta|)."""
    th = np.abs(theta_values() if theta is None else theta)
    return np.abs(G - D) * th / np.maximum(1.0, np.abs(D) * th)
