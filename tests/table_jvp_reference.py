"""Reference for the directional sensitivities along a direction in the track tables (ltompc_get_jvp_tables)
without any kernel: sens_reference's KKT matrix at a given primal-dual iterate, F_y dy - the derivative of the condensed KKT
residual w.r.t. the table values (the F_y of table_sens_reference.py) applied to the direction - and ONE dense solve,

    A z = -F_y dy  (+ the right-hand side of (x0, u_prev) times dp),      (tX, tU) = the (x, u) entries of z.

F_y dy comes from torch by double-backward through the torch restatement of the NLP (nlp_reference.py): with the stage pieces
F(y) = (grad_V L, G, g) and a dummy cotangent u, F_y' u is one reverse pass to the four value rows, linear in u, and the
derivative of <F_y' u, dy> w.r.t. u is F_y dy.  The chain to the knots is autograd's, through the rounding patch too: the numpy
`lut_basis` is not used for the result.  The per-slot form (dslot, the tangents of the ten look-up results of every slot in
table_sens_reference.SLOT_NAMES order) applies the Jacobian w.r.t. value and slope offsets of every look-up instead.

The stage pieces go to the global right-hand side by the transpose of what table_sens_reference contracts with: the stage
variables' 28 entries (with Jh' Sigma dh/dy folded in for the track rows) are added at their global indices, the collocation
rows' 16 entries follow.

`scale` is the sum of the absolute terms of the contraction J_slot . dslot (+ J_p . dp): the Jacobian of (X, U) w.r.t. the ten
scalars of every slot, column by column on the same LU (unrefined: it is a magnitude), times the slot tangents - those given,
plus those of dtables gathered with the numpy `lut_basis` (used for the scale only)."""
from __future__ import annotations

import contextlib
from types import SimpleNamespace

import numpy as np
import scipy.sparse.linalg as spla
import torch

import nlp_reference as R
import sens_reference as SR
import table_sens_reference as TR

NS = TR.NS


def slot_tangents(dtables, S_c, S_x, tab, eps, period=0.0):
    """The ten tangents (N,10) of one instance's slots for a direction dtables (4,n): value and slope of the look-ups at
    s(c_k) = S_c[k], s(x_{k+1}) = S_x[k] through the numpy lut_basis (all ten for every slot; the last six of slot N - 1 do
    not enter the problem)."""
    N = len(S_c)
    out = np.zeros((N, NS))
    for k in range(N):
        for row, col, grid, s in ((0, 0, tab.s_kappa, S_c[k]), (0, 2, tab.s_kappa, S_x[k]), (1, 4, tab.s_arc, S_x[k]),
                                  (2, 6, tab.s_arc, S_x[k]), (3, 8, tab.s_arc, S_x[k])):
            idx, wv, ws = TR.lut_basis(grid, s, eps, period)
            out[k, col], out[k, col + 1] = wv @ dtables[row][idx], ws @ dtables[row][idx]
    return out


def _to_stage(d):
    """slot order -> sens_reference's stage order: the stage cost of node k + 1 (v_ref, columns 8, 9) is stage k + 1's"""
    z = np.array(d, float)
    z[..., 1:, 8:] = d[..., :-1, 8:]
    z[..., 0, 8:] = 0.0
    return z


@contextlib.contextmanager
def wrapped_lut(period):
    """nlp_reference.lut with the wrap of periodic tables (model.h: s - period floor((s - g0) / period); the floor has no
    derivative, as in the kernels) for the body; nothing when period is 0."""
    plain = R.lut
    if period > 0:
        R.lut = lambda grid, y, s, e: plain(grid, y, s - period * torch.floor((s.detach() - float(grid[0])) / period), e)
    try:
        yield
    finally:
        R.lut = plain


def table_jvp_batch(it, x0, uprev, tab, eps, params, dtables=None, dslot=None, dp=None, refine=3, h=0.1, base=None, period=0.0, scale=True, fine=False):
    """table_jvp_batch_ with the look-ups wrapped by `period` (0: tables that are not periodic)."""
    with wrapped_lut(period):
        return table_jvp_batch_(it, x0, uprev, tab, eps, params, dtables, dslot, dp, refine, h, base, period, scale, fine)


def table_jvp_batch_(it, x0, uprev, tab, eps, params, dtables=None, dslot=None, dp=None, refine=3, h=0.1, base=None, period=0.0, scale=True, fine=False):
    """For M instances (it, x0, uprev as in sens_reference.sensitivities_batch) and the direction dtables (4,n; shared),
    dslot (M,N,10), dp (M,10), any of them None: a dict with tX (M,N+1,8), tU (M,N,2), scale_X, scale_U (the same shapes; scale_X_tab, scale_U_tab: without the dp terms),
    ok_expected (M,) and base (sens_reference's per-instance results, which may be passed in).  scale=False leaves the scales 0
    (they cost N more solves per instance).  fine=True adds fine_X, fine_U (fine_X_tab, fine_U_tab: without the dp terms): the
    absolute terms of the solve itself, |A^-1| |right-hand side| entry by entry - the magnitude of what cancels inside the pass,
    which at an active track constraint (Sigma = nu / t of 1e8 and more in the right-hand side) is far above the scale."""
    if base is None:
        base = SR.sensitivities_batch(it, x0, uprev, tab, eps, params, refine, h)
    X = torch.tensor(np.asarray(it["X"], float)).clone()
    M, N = X.shape[0], X.shape[1] - 1
    X[:, 0] = torch.as_tensor(np.asarray(x0, float).reshape(M, 8))
    C, U = torch.tensor(np.asarray(it["C"], float)), torch.tensor(np.asarray(it["U"], float))
    Um = torch.cat([torch.as_tensor(np.asarray(uprev, float)).reshape(M, 1, 2), U[:, :-1]], dim=1)
    V = torch.cat([X[:, :-1], C, U, X[:, 1:], Um], dim=2).reshape(M * N, SR.NV).requires_grad_(True)
    nb = len(SR.bound_rows(params))
    NUnl = torch.tensor(np.asarray(it["NU"], float)[:, :, nb:nb + 3]).reshape(M * N, 3)
    Sig = NUnl / torch.tensor(np.asarray(it["T"], float)[:, :, nb:nb + 3]).reshape(M * N, 3)
    last = torch.zeros(M, N)
    last[:, N - 1] = 1.0
    last = last.reshape(M * N)
    nlmask = 1.0 - last
    L1, L2 = (torch.tensor(np.asarray(it[k], float)).reshape(M * N, 8) for k in ("L1", "L2"))

    def residual(tabs):
        L, G, g = SR._stage_functions(V, L1, L2, NUnl, last, nlmask, tabs, eps, h)
        return torch.cat([torch.autograd.grad(L.sum(), V, create_graph=True)[0], G, g], dim=1)   # (MN,47)

    FdY = torch.zeros(M * N, SR.NV + 16 + 3)
    # ---- the tables form: F_y dy by double-backward through lut
    if dtables is not None:
        dy = np.asarray(dtables, float)
        assert dy.shape == (4, len(tab.kappa)), dy.shape
        rows = {r: torch.tensor(np.asarray(getattr(tab, r), float)).requires_grad_(True) for r in TR.ROWS}
        F = residual(SimpleNamespace(s_kappa=tab.s_kappa, s_arc=tab.s_arc, **rows))
        u = torch.ones_like(F).requires_grad_(True)
        gr = torch.autograd.grad((F * u).sum(), [rows[r] for r in TR.ROWS], create_graph=True, allow_unused=True)
        lin = sum((g * torch.tensor(dy[i])).sum() for i, g in enumerate(gr) if g is not None)
        FdY = FdY + torch.autograd.grad(lin, u)[0]
    # ---- the Jacobian w.r.t. value and slope offsets of every look-up, call by call (stage order)
    Z = torch.zeros(M * N, NS, requires_grad=True)
    plain, calls = R.lut, []

    def lut_with_offsets(grid, y, s, e):
        c = len(calls)
        calls.append(c)
        return plain(grid, y, s, e) + Z[:, 2 * c] + Z[:, 2 * c + 1] * (s - s.detach())

    R.lut = lut_with_offsets
    try:
        F = residual(tab)
    finally:
        R.lut = plain
    assert len(calls) == NS // 2, calls
    JZ = torch.zeros(M * N, F.shape[1], NS)
    for i in range(F.shape[1]):
        gi = torch.autograd.grad(F[:, i].sum(), Z, retain_graph=True, allow_unused=True)[0]
        if gi is not None:
            JZ[:, i] = gi
    JZ = JZ.detach()
    if dslot is not None:
        zs = torch.tensor(_to_stage(np.asarray(dslot, float).reshape(M, N, NS))).reshape(M * N, NS)
        FdY = FdY + torch.einsum("siq,sq->si", JZ, zs)
    # ---- stage pieces -> the global right-hand side, per instance; the solve
    g_rows = residual(tab)[:, SR.NV + 16:]
    Jg = SR._rows(g_rows, V).detach()                                       # (MN,3,28)
    w = (Sig * nlmask[:, None])

    def assemble(Fs):
        """(MN,47,...) stage pieces -> (M, N, 28, ...) V part with Jh' Sigma dh folded in and (M, N, 16, ...) G part"""
        FV, FG, Fg = Fs[:, :SR.NV], Fs[:, SR.NV:SR.NV + 16], Fs[:, SR.NV + 16:]
        if Fs.dim() == 2:
            FV = FV + torch.einsum("sqa,sq->sa", Jg, w * Fg)
        else:
            FV = FV + torch.einsum("sqa,sqc->sac", Jg, w[:, :, None] * Fg)
        return FV.detach().numpy().reshape(M, N, SR.NV, -1), FG.detach().numpy().reshape(M, N, 16, -1)

    rV, rG = assemble(FdY)
    cV, cG = assemble(JZ)
    idx, nz = SR._index(N)
    nw = 18 * N
    tX, tU = np.zeros((M, N + 1, 8)), np.zeros((M, N, 2))
    sX, sU = np.zeros((M, N + 1, 8)), np.zeros((M, N, 2))
    yX, yU = np.zeros((M, N + 1, 8)), np.zeros((M, N, 2))      # ... the table part of the scale alone
    fX, fU, fyX, fyU = (np.zeros(s_) for s_ in ((M, N + 1, 8), (M, N, 2)) * 2)
    Xn, Cn = np.asarray(it["X"], float), np.asarray(it["C"], float)
    for m, q in enumerate(base):
        A = q["kkt"]

        def glob(v, g):
            """stage pieces (N,28,c), (N,16,c) -> (n_A, c)"""
            full = np.zeros((nz, v.shape[2]))
            np.add.at(full, idx, v)
            return np.vstack([full[8:nz - 2], g.reshape(16 * N, -1)])

        rhs = -glob(rV[m], rG[m])[:, 0]
        if dp is not None:
            rhs = rhs + q["rhs"] @ np.asarray(dp, float)[m]
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A")
        z = lu.solve(rhs).astype(np.longdouble)
        for _ in range(refine):
            r = rhs.astype(np.longdouble) - SR._matvec_ld(A, z[:, None])[:, 0]
            z = z + lu.solve(np.asarray(r, dtype=np.float64))
        z = np.asarray(z, dtype=np.float64)
        tX[m, 1:], tU[m] = z[:8 * N].reshape(N, 8), z[16 * N:nw].reshape(N, 2)
        if dp is not None:
            tX[m, 0] = np.asarray(dp, float)[m, :8]
        if fine:   # the absolute terms of the solve itself, |A^-1| |right-hand side|, entry by entry
            Ai = np.abs(np.linalg.inv(A.toarray()))
            cy = np.abs(glob(rV[m], rG[m])[:, 0])
            for (fx, fu), c in (((fyX, fyU), cy), ((fX, fU), cy + (np.abs(q["rhs"]) @ np.abs(np.asarray(dp, float)[m]) if dp is not None else 0.0))):
                t = Ai @ c
                fx[m, 1:], fu[m] = t[:8 * N].reshape(N, 8), t[16 * N:nw].reshape(N, 2)
        if not scale:
            continue
        # the scale: |J_slot| |slot tangents| (+ |J_p| |dp|)
        zdir = np.zeros((N, NS))
        if dslot is not None:
            zdir += np.asarray(dslot, float).reshape(M, N, NS)[m]
        if dtables is not None:
            zdir += slot_tangents(np.asarray(dtables, float), Cn[m][:, 0], Xn[m][1:, 0], tab, eps, period)
        # one solve per stage: the columns of the stages apart, not their sum
        sc = np.zeros(A.shape[0])
        zst = _to_stage(zdir)
        for k in range(N):
            vk, gk = np.zeros((N, SR.NV, NS)), np.zeros((N, 16, NS))
            vk[k], gk[k] = cV[m].reshape(N, SR.NV, NS)[k], cG[m].reshape(N, 16, NS)[k]
            Jk = lu.solve(-glob(vk, gk))
            sc += np.abs(Jk * zst[k][None, :]).sum(axis=1)
        yX[m, 1:], yU[m] = sc[:8 * N].reshape(N, 8), sc[16 * N:nw].reshape(N, 2)
        if dp is not None:
            sc += np.abs(lu.solve(q["rhs"]) * np.asarray(dp, float)[m][None, :]).sum(axis=1)
        sX[m, 1:], sU[m] = sc[:8 * N].reshape(N, 8), sc[16 * N:nw].reshape(N, 2)
        if dp is not None:
            sX[m, 0] = np.abs(np.asarray(dp, float)[m, :8])
    return dict(tX=tX, tU=tU, scale_X=sX, scale_U=sU, scale_X_tab=yX, scale_U_tab=yU, fine_X=fX, fine_U=fU, fine_X_tab=fyX, fine_U_tab=fyU, ok_expected=np.array([q["ok_expected"] for q in base]), base=base)
