"""The dense reference for the gradients w.r.t. the track tables (table_sens_reference.py) pinned without a
GPU: against central differences of oracle re-solves with single knot values perturbed (rows v_ref, n_left with an active left
boundary, kappa), its per-slot form against its tables form through the numpy `lut_basis`, and `lut_basis` against the torch
look-up."""
import numpy as np
import pytest
import torch

import nlp_reference as R
import synthetic_tracks as ST
import table_sens_reference as TR
from test_sens_reference import KEYS

N = 10
BATCHES = ((8, 23), (6, 21))   # (instances, seed): three instances pass every criterion, one of them at the left edge
H_REL = 1e-6   # step of a knot value: H_REL x the largest magnitude of its row (a single knot of kappa may be 0)


def _left_edge_batch(pkg, tables, n, seed):
    """Sampled states; every second one next to the left-hand edge of the band (an active left boundary)."""
    x = pkg.sample_x0(tables, n, seed=seed)
    s = x[::2, 0]
    nl, nr = np.interp(s, tables.s_arc, tables.n_left), np.interp(s, tables.s_arc, tables.n_right)
    mid, w = 0.5 * (nl - nr), 0.5 * (nl + nr - 2.3)
    x[::2, 1] = mid + 0.97 * w
    return x


def _with_knot(pkg, tables, row, j, value):
    rows = {r: np.array(getattr(tables, r)) for r in TR.ROWS}
    rows[row][j] = value
    return pkg.TrackTables(s_kappa=tables.s_kappa, s_arc=tables.s_arc, **rows)


def test_lut_basis_reproduces_the_lookup(tables):
    """sum w_val y and sum w_slope y against nlp_reference.lut and its autograd slope, on the shipped grid and on a jittered
    40-knot grid at its look-up edges (knots +- 1e-9, window borders, both ends and beyond), eps = 1e-4 and 0."""
    rng = np.random.default_rng(2)
    for track, pts in ((tables, rng.uniform(-3.0, tables.s_arc[-1] + 3.0, 200)), (ST.get("chicane40_jit20"), ST.edges("chicane40_jit20"))):
        for grid, y in ((track.s_kappa, track.kappa), (track.s_arc, track.v_ref)):
            for eps in (1e-4, 0.0):
                s = torch.tensor(np.asarray(pts, float), requires_grad=True)
                v = R.lut(grid, y, s, eps)
                sl = torch.autograd.grad(v.sum(), s)[0].numpy()
                scale = np.abs(y).max()
                for q, sq in enumerate(pts):
                    idx, wv, ws = TR.lut_basis(grid, sq, eps)
                    assert abs(wv @ y[idx] - v[q].item()) <= 1e-13 * scale, (sq, eps)
                    d = np.diff(grid).min()
                    assert abs(ws @ y[idx] - sl[q]) <= 1e-12 * scale / d, (sq, eps)
                    assert abs(wv.sum() - 1.0) <= 1e-13 and abs(ws.sum()) <= 1e-12 / d   # constants are reproduced, with slope 0


def test_table_gradients_match_central_differences(pkg, tables, orc, oracle):
    """At oracle solutions (N = 10), <(gX, gU), d(X, U)/dy_j> for single knots j of v_ref, n_left and kappa against central
    differences of warm-started re-solves with that knot moved by h and by 10 h.  §9.1's criteria: instances whose solves all
    ended SOLVED with margin >= 1e-3, differences that agree between h and 10 h to 1e-5 and show no kink; §9.1's measure with
    the row's magnitude in the place of |theta_j|, |G - D| s / max(1, |D| s); §9.1's bound 1e-4 + mu / margin^2.  Two knots per
    row and instance: the knot nearest to a look-up of the horizon's second node and the one nearest to its seventh (inside
    their rounding windows, asserted for one of them).  Knots far from the prediction: exactly 0.  The per-slot form, chained
    to the knots by the numpy lut_basis, reproduces the tables form."""
    x = np.vstack([_left_edge_batch(pkg, tables, n, seed) for n, seed in BATCHES])
    B = x.shape[0]
    r = oracle.solve(x, N)
    eps = oracle.o.smooth_eps_min
    params = pkg.default_params()
    rng = np.random.default_rng(4)
    gX, gU = rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))
    up = np.zeros((B, 2))
    ref = TR.table_gradients_batch({k: r[k] for k in KEYS}, x, up, tables, eps, params, gX, gU)
    nb = r["NU"].shape[2] - 3
    assert (r["NU"][::2, :N - 1, nb] > 1e-2).any(), "no active left boundary in the batch"
    warm = {k: r[k] for k in ("X", "C", "U", "L1", "L2")}
    used, checked, worst, in_window, left_active = 0, {row: 0 for row in TR.ROWS}, 0.0, 0, 0
    for b in range(B):
        q = ref["base"][b]
        X = r["X"][b].copy()
        X[0] = x[b]
        # per-slot form -> knots, against the tables form (the same adjoint vector, two routes through the look-ups)
        got, mag = TR.scatter(ref["slot_grad"][b], r["C"][b][:, 0], X[1:, 0], tables, eps)
        assert np.abs(got - ref["grad_tables"][b]).max() <= 1e-11 * max(1.0, mag.max()), b
        # far from the prediction: exactly 0
        lo, hi = min(X[:, 0].min(), r["C"][b][:, 0].min()), max(X[:, 0].max(), r["C"][b][:, 0].max())
        for row, grid in (("kappa", tables.s_kappa), ("n_left", tables.s_arc), ("n_right", tables.s_arc), ("v_ref", tables.s_arc)):
            far = (grid < lo - 5.0) | (grid > hi + 5.0)
            G = ref["grad_tables"][b, TR.ROWS.index(row)]
            assert far.sum() > 800 and (G[far] == 0).all() and np.abs(G[~far]).max() > 0, (b, row)
        if r["status_solver"][b] != 0 or q["margin"] < 1e-3:
            continue
        tol = 1e-4 + max(r["mu"][b], 1e-9) / q["margin"] ** 2
        inst_used = False
        for row in ("v_ref", "n_left", "kappa"):
            grid = tables.s_kappa if row == "kappa" else tables.s_arc
            sc = np.abs(getattr(tables, row)).max()
            for node in (2, 7):
                j = int(np.argmin(np.abs(grid - X[node, 0])))
                in_window += abs(grid[j] - X[node, 0]) < ST.windows(grid)[j - 1]
                D = {}
                solved, kink = True, False
                for f in (1.0, 10.0):
                    h = f * H_REL * sc
                    res = []
                    for sgn in (1.0, -1.0):
                        t = _with_knot(pkg, tables, row, j, getattr(tables, row)[j] + sgn * h)
                        p = orc.Oracle(t.packed()).solve(x[b:b + 1], N, warm={k: v[b:b + 1] for k, v in warm.items()},
                                                         prev_status=r["status_solver"][b:b + 1])
                        solved = solved and p["status_solver"][0] == 0
                        res.append(p)
                    D[f] = sum((g * (res[0][k][0] - res[1][k][0])).sum() for g, k in ((gX[b], "X"), (gU[b], "U"))) / (2 * h)
                    if f == 1.0:   # X[0] is the measured state on both sides: block 0 drops out
                        one = sum((g * ((res[0][k][0] - r[k][b]) - (r[k][b] - res[1][k][0]))).sum() for g, k in ((gX[b], "X"), (gU[b], "U"))) / h
                        kink = abs(one) * sc / max(1.0, abs(D[1.0]) * sc) > 1e-2
                if not solved or kink or abs(D[1.0] - D[10.0]) * sc / max(1.0, abs(D[1.0]) * sc) > 1e-5:
                    continue
                G = ref["grad_tables"][b, TR.ROWS.index(row), j]
                e = abs(G - D[1.0]) * sc / max(1.0, abs(D[1.0]) * sc)
                assert e <= tol, (b, row, j, G, D[1.0], e, tol)
                worst = max(worst, e / tol)
                checked[row] += 1
                left_active += row == "n_left" and r["NU"][b, :N - 1, nb].max() > 1e-2
                inst_used = True
        used += inst_used
    print(f"{used} instances used, n_left knots checked with an active left boundary {left_active}, checked per row {checked}, look-ups inside a rounding window {in_window}, largest err / tol {worst:.3g}")
    assert used >= 3 and in_window >= 1 and left_active >= 1, (used, in_window, left_active)
    assert all(checked[row] >= 2 for row in ("v_ref", "n_left", "kappa")), checked
