"""Reference for the adjoint gradients w.r.t. the track tables (ltompc_get_adjoint_tables) without truncation
error: sens_reference's KKT matrix at a given primal-dual iterate, ONE dense solve with the cotangent (gX, gU) on the
right-hand side (the matrix is symmetric), and the contraction of that adjoint vector with F_y, the derivative of the condensed
KKT residual w.r.t. the table values y,

    F_y = [ d(grad_w L)/dy + Jh' Sigma dh/dy ;  dG/dy ],      grad_y <(gX, gU), (X, U)> = -z' F_y,   A z = (gX, gU; 0)

(the second term of the first block: the track rows h = gL, gR+, gR- depend on n_left and n_right; Sigma = NU / T).  The
contraction is one torch.autograd.grad through the torch restatement of the NLP (nlp_reference.py) with the four value rows as
tensors that require grad: nlp_reference.lut takes them through torch.as_tensor, so the chain rule to the knots is autograd's,
through the rounding patch too.

The per-slot form differentiates w.r.t. per-stage copies of what the look-ups returned instead: every look-up gets a value
offset and a slope offset (y(s) + dv + ds (s - s_0), s_0 the look-up point), ten scalars per slot in SLOT_NAMES order.  Slot k
owns kappa at c_k and at x_{k+1} and n_left, n_right, v_ref at x_{k+1} (the stage cost of node k + 1 is stage k + 1's in
sens_reference's stage functions: it is moved to slot k here).  `lut_basis` is the numpy statement of the knot weights of a
look-up; `scatter` chains the per-slot form to the knots with it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import scipy.sparse.linalg as spla
import torch

import nlp_reference as R
import sens_reference as SR

ROWS = ("kappa", "n_left", "n_right", "v_ref")
SLOT_NAMES = ("kappa_c", "kappa_c'", "kappa_x", "kappa_x'", "n_left", "n_left'", "n_right", "n_right'", "v_ref", "v_ref'")
NS = len(SLOT_NAMES)
_CALLS = ("kappa_c", "kappa_x", "n_left", "n_right", "v_ref")   # the look-ups of sens_reference._stage_functions, in its order


def lut_basis(grid, s, eps, period=0.0):
    """Knot indices (4,), value weights (4,) and slope weights (4,) of one look-up at s on `grid` with rounding length eps:
    value = sum w_val y[idx], slope = sum w_slope y[idx] for every row y on that grid (model.h: lut_eval).  The knots are
    i-1 .. i+2 around the interval i of s, clamped to the grid (a clamped knot has weight 0)."""
    g = np.asarray(grid, float)
    n = g.size
    if period > 0:
        s = s - period * np.floor((s - g[0]) / period)
    i = int(np.clip(np.searchsorted(g, s, side="right") - 1, 0, n - 2))
    idx = np.array([max(i - 1, 0), i, i + 1, min(i + 2, n - 1)])
    d = g[i + 1] - g[i]
    wv, ws = np.zeros(4), np.zeros(4)
    t = (s - g[i]) / d
    wv[1] += 1.0 - t
    wv[2] += t
    ws[1] -= 1.0 / d
    ws[2] += 1.0 / d
    if eps > 0:
        kn, z, W, sg = -1, 0.0, 0.0, 0.0
        if i > 0:
            Wk, zz = 0.5 * min(g[i] - g[i - 1], d), s - g[i]
            if 0.0 <= zz < Wk:
                kn, z, W, sg = i, zz, Wk, 1.0
        if kn < 0 and i + 1 < n - 1:
            Wk, zz = 0.5 * min(d, g[i + 2] - g[i + 1]), s - g[i + 1]
            if zz < 0.0 and -zz < Wk:
                kn, z, W, sg = i + 1, zz, Wk, -1.0
        if kn > 0:
            o = 0 if kn == i else 1                      # knots kn-1, kn, kn+1 are idx[o], idx[o+1], idx[o+2]
            ga, gb, gc = g[kn - 1], g[kn], g[kn + 1]
            # the patch coefficients of nlp_reference.lut with the differences of nearly equal numbers written out
            # (R - |z| = eps^2 / (R + |z|), W - RW = -eps^2 / (RW + W), 1 - W / RW = eps^2 / (RW (RW + W))): eps << W
            Rz, RW, e2 = np.sqrt(z * z + eps * eps), np.sqrt(W * W + eps * eps), eps * eps
            a = e2 / (RW * (RW + W)) / (2.0 * W)
            b = -e2 / (RW + W) - a * W * W
            cv, cs = 0.5 * (e2 / (Rz + abs(z)) + a * z * z + b), 0.5 * (2.0 * a * z - sg * e2 / (Rz * (Rz + abs(z))))
            # J = (yc - yb) / (gc - gb) - (yb - ya) / (gb - ga)
            J = np.array([1.0 / (gb - ga), -1.0 / (gc - gb) - 1.0 / (gb - ga), 1.0 / (gc - gb)])
            wv[o:o + 3] += cv * J
            ws[o:o + 3] += cs * J
    return idx, wv, ws


def scatter(slot_grad, S_c, S_x, tab, eps, period=0.0):
    """grad_tables (4, n) from per-slot gradients (N, 10) of one instance: S_c (N,), S_x (N,) the look-up points s(c_k),
    s(x_{k+1}).  Also returns the sum of the absolute terms per knot."""
    n = len(tab.kappa)
    out, mag = np.zeros((4, n)), np.zeros((4, n))
    for k in range(slot_grad.shape[0]):
        for row, col, grid, s in ((0, 0, tab.s_kappa, S_c[k]), (0, 2, tab.s_kappa, S_x[k]), (1, 4, tab.s_arc, S_x[k]),
                                  (2, 6, tab.s_arc, S_x[k]), (3, 8, tab.s_arc, S_x[k])):
            idx, wv, ws = lut_basis(grid, s, eps, period)
            t = slot_grad[k, col] * wv + slot_grad[k, col + 1] * ws
            np.add.at(out[row], idx, t)
            np.add.at(mag[row], idx, np.abs(slot_grad[k, col] * wv) + np.abs(slot_grad[k, col + 1] * ws))
    return out, mag


def _adjoint_vectors(base, gX, gU, refine):
    """z = A^-1 (gX, gU; 0) per instance, scattered to sens_reference's stage variables: aV (M,N,28), aG (M,N,16)."""
    out = []
    for m, q in enumerate(base):
        A = q["kkt"]
        N = gU.shape[1]
        nw = 18 * N
        c = np.zeros(A.shape[0])
        c[:8 * N] = gX[m, 1:].ravel()
        c[16 * N:18 * N] = gU[m].ravel()
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A")
        z = lu.solve(c).astype(np.longdouble)
        for _ in range(refine):
            r = c.astype(np.longdouble) - SR._matvec_ld(A, z[:, None])[:, 0]
            z = z + lu.solve(np.asarray(r, dtype=np.float64))
        z = np.asarray(z, dtype=np.float64)
        idx, nz = SR._index(N)
        full = np.zeros(nz)                       # x_0 and u_prev are parameters: their adjoint entries are 0
        full[8:nz - 2] = z[:nw]
        out.append((full[idx], z[nw:].reshape(N, 16)))
    return np.stack([a for a, _ in out]), np.stack([g for _, g in out])


def table_gradients_batch(it, x0, uprev, tab, eps, params, gX, gU, refine=3, h=0.1, slots=True):
    """For M instances (it, x0, uprev as in sens_reference.sensitivities_batch; cotangents gX (M,N+1,8), gU (M,N,2)):
    a dict with
      grad_tables (M,4,n)   per instance, rows in ROWS order (the kernel's grad_tables is their sum over the ok instances)
      slot_grad   (M,N,10)  SLOT_NAMES order, and slot_scale (M,N,10): the sum of the absolute terms of each contraction
      ok_expected (M,) and base (sens_reference's per-instance results)
    gX[:, 0] does not enter (block 0 of dX/dy is 0: x0 is data)."""
    gX, gU = np.asarray(gX, float), np.asarray(gU, float)
    base = SR.sensitivities_batch(it, x0, uprev, tab, eps, params, refine, h)
    aV, aG = _adjoint_vectors(base, gX, gU, refine)
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
    tV, tG = torch.tensor(aV).reshape(M * N, SR.NV), torch.tensor(aG).reshape(M * N, 16)

    def residual(tabs):
        """the stage pieces of F(y): grad_V L (MN,28), G (MN,16) and the track rows g (MN,3)"""
        L, G, g = SR._stage_functions(V, L1, L2, NUnl, last, nlmask, tabs, eps, h)
        return torch.autograd.grad(L.sum(), V, create_graph=True)[0], G, g

    # ---- the tables form: one reverse pass through lut to the knots, per instance (instance m's stages only)
    rows = {r: torch.tensor(np.asarray(getattr(tab, r), float)).requires_grad_(True) for r in ROWS}
    tabs = SimpleNamespace(s_kappa=tab.s_kappa, s_arc=tab.s_arc, **rows)
    gL, G, g = residual(tabs)
    Jg = SR._rows(g, V).detach()                                           # (MN,3,28)
    coef_g = torch.einsum("sqa,sa->sq", Jg, tV) * Sig * nlmask[:, None]    # (Jh a) Sigma per track row
    per_stage = (tV * gL).sum(-1) + (tG * G).sum(-1) + (coef_g * g).sum(-1)
    grad_tables = np.zeros((M, 4, len(tab.kappa)))
    for m in range(M):
        gr = torch.autograd.grad(per_stage[m * N:(m + 1) * N].sum(), [rows[r] for r in ROWS], retain_graph=True)
        grad_tables[m] = -np.stack([t.numpy() for t in gr])
    out = dict(grad_tables=grad_tables, ok_expected=np.array([q["ok_expected"] for q in base]), base=base)
    if not slots:
        return out
    # ---- the per-slot form: offsets of the value and the slope of every look-up, call by call
    Z = torch.zeros(M * N, NS, requires_grad=True)
    plain, calls = R.lut, []

    def lut_with_offsets(grid, y, s, e):
        c = len(calls)
        calls.append(c)
        return plain(grid, y, s, e) + Z[:, 2 * c] + Z[:, 2 * c + 1] * (s - s.detach())

    R.lut = lut_with_offsets
    try:
        gL, G, g = residual(tab)
    finally:
        R.lut = plain
    assert len(calls) == len(_CALLS), calls
    F = torch.cat([gL, G, g], dim=1)                                      # (MN,47)
    coef = torch.cat([tV, tG, coef_g], dim=1)
    JZ = torch.zeros(M * N, F.shape[1], NS)
    for i in range(F.shape[1]):
        gi = torch.autograd.grad(F[:, i].sum(), Z, retain_graph=True, allow_unused=True)[0]
        if gi is not None:
            JZ[:, i] = gi
    terms = (-coef[:, :, None] * JZ).reshape(M, N, F.shape[1], NS).numpy()
    sg, sc = terms.sum(axis=2), np.abs(terms).sum(axis=2)
    for a in (sg, sc):                                                    # the stage cost of node k + 1: from stage k + 1 to slot k
        a[:, :-1, 8:] = a[:, 1:, 8:]
        a[:, -1, 8:] = 0.0
    out.update(slot_grad=sg, slot_scale=sc)
    return out
