"""The batched table look-up of the evaluation kernels (csrc/model.h: slot_luts_fetch / slot_luts_pin / slot_luts_finish, used by
k_eval, k_expand, k_linesearch and k_step1) against lut_eval, which the plant and the derivative passes still call look-up by
look-up.  The finish is lut_eval's text after its loads, so the two must give the same bits at every arc length, the ones where
the uniform-spacing estimate of the interval is wrong (search and refetch) among them.

test_batched_lookup_equals_lut_eval: ltompc_test_lut evaluates the five look-ups of a slot (kappa at s[t]; kappa, v_ref, n_left,
n_right at s[n - 1 - t]) both ways; the arc lengths are chosen on the CPU from the shipped tables (see _points).

test_line_search_of_narrow_and_wide_path_agrees: k_step1 holds the batch of knots apart from the slacks of the simple bounds (its
256 registers do not hold both), k_linesearch has them in one batch; same numbers.  N = 10 and N = 41, B = 5 with the states of
tests/test_gpu_pick_paths.py, three ticks, narrow path against wide path bit for bit."""
import numpy as np
import pytest

from test_gpu_pick_paths import WIDE, _states

pytestmark = pytest.mark.gpu
SMOOTH_EPS_MIN = 1e-4   # ltompc_default_options; tests/test_host_harness_lut.py runs the same points without the library


def _estimate_off(g, s):
    """True where int((s - g0) * inv), clamped to [0, n - 2], is not the interval searchsorted finds (lut_eval's fallback runs)."""
    n = len(g)
    inv = (n - 1) / (g[-1] - g[0])
    fi = (s - g[0]) * inv
    est = np.where(fi <= 0.0, 0, np.where(fi >= n - 2, n - 2, np.minimum(fi, n - 2).astype(np.int64)))
    true = np.clip(np.searchsorted(g, s, side="right") - 1, 0, n - 2)
    return est != true


def _points(tables):
    """Arc lengths on one lap: every knot of both grids, the first and the last interval, before the first and beyond the last knot,
    inside and outside the smoothing width W = half the shorter adjacent interval of every 25th knot, and points where the
    interval estimate is off on the (non-uniform) arc-length grid.  Returns the points and the mask of the last group."""
    out = []
    for g in (tables.s_kappa, tables.s_arc):
        out.append(g)
        out.append(g[0] + np.array([1e-9, 0.3, 0.999]) * (g[1] - g[0]))
        out.append(g[-1] - np.array([1e-9, 0.3, 0.999]) * (g[-1] - g[-2]))
        out.append(g[0] - np.array([1e-9, 1.7, 100.0]))
        out.append(g[-1] + np.array([1e-9, 2.3, 250.0]))
        j = np.arange(1, len(g) - 1, 25)
        W = 0.5 * np.minimum(g[j] - g[j - 1], g[j + 1] - g[j])
        for f in (0.25, 0.999, 1.001, 1.5):
            out += [g[j] - f * W, g[j] + f * W]
    g = tables.s_arc
    cand = np.concatenate([np.linspace(g[0], g[-1], 40001), np.nextafter(g, -np.inf), 0.5 * (g[1:] + g[:-1])])
    off = cand[_estimate_off(g, cand)]
    off = off[:: max(1, len(off) // 200)]   # (a couple of hundred are plenty)
    s = np.concatenate(out + [off])
    mask = np.zeros(len(s), bool)
    mask[-len(off):] = True
    return s, mask


def _pwl(g, y, s):
    """Piece-wise linear with linear extrapolation (lut_eval at eps = 0), in numpy."""
    i = np.clip(np.searchsorted(g, s, side="right") - 1, 0, len(g) - 2)
    return y[i] + (y[i + 1] - y[i]) / (g[i + 1] - g[i]) * (s - g[i])


@pytest.mark.parametrize("periodic", [0, 1])
def test_batched_lookup_equals_lut_eval(pkg, tables, gpu_lib, periodic):
    s, off = _points(tables)
    assert off.sum() >= 20 and _estimate_off(tables.s_arc, s[off]).all(), off.sum()
    o = pkg.default_options()
    o.periodic_tables = periodic
    assert o.smooth_eps_min == SMOOTH_EPS_MIN
    if periodic:   # the same points one and two laps on (and the extrapolated ones, which the wrap brings back onto the table)
        span = tables.s_arc[-1] - tables.s_arc[0]
        s = np.concatenate([s, s + span, s + 2.0 * span])
    m = pkg.BatchedMPC(tables, 4, 1, options=o)
    try:
        for eps in (0.0, o.smooth_eps_min):
            direct, batched = m.test_lut(s, eps)
            assert np.all(np.isfinite(direct))
            assert np.array_equal(direct.view(np.uint64), batched.view(np.uint64)), (periodic, eps, np.argwhere(direct != batched)[:5])
            if eps == 0.0 and not periodic:   # ... and the hook looks up what it says, where it says
                sx = s[::-1]
                ref = np.stack([_pwl(tables.s_kappa, tables.kappa, s), _pwl(tables.s_kappa, tables.kappa, sx), _pwl(tables.s_arc, tables.v_ref, sx),
                                _pwl(tables.s_arc, tables.n_left, sx), _pwl(tables.s_arc, tables.n_right, sx)], axis=1)
                assert np.abs(direct[:, :, 0] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
                assert np.all(direct[:, :, 2] == 0.0)
            else:
                assert np.any(direct[:, :, 2] != 0.0) or eps == 0.0   # smoothing: some points lie inside a knot's window
    finally:
        m.close()


def _closed_loop(pkg, tables, N, x0, ticks):
    m = pkg.BatchedMPC(tables, N, x0.shape[0])
    m.set_initial_guess(x0)
    x, out = x0.copy(), []
    for _ in range(ticks):
        u = m.make_step(x)
        st = m.stats()
        out.append(dict(u0=u.copy(), status=st["status"].copy(), iters=st["iters"].copy(), n_resto=st["n_resto"].copy(),
                        n_shift=st["n_shift"].copy(), it=m.iterate()))   # (the iterate: X, C, U, multipliers, slacks)
        x = m.plant_step(x, u, 100)
    m.close()
    return out


@pytest.mark.parametrize("N", [10, 41])
def test_line_search_of_narrow_and_wide_path_agrees(pkg, tables, gpu_lib, monkeypatch, N):
    x0 = _states(pkg, tables)[:5]
    ref = _closed_loop(pkg, tables, N, x0, 3)
    for k, v in WIDE.items():
        monkeypatch.setenv(k, v)
    got = _closed_loop(pkg, tables, N, x0, 3)
    for t, (a, b) in enumerate(zip(ref, got)):
        for key in ("u0", "status", "iters", "n_resto", "n_shift"):
            assert np.array_equal(a[key], b[key]), (N, t, key)
        for key in a["it"]:
            assert np.array_equal(a["it"][key], b["it"][key], equal_nan=True), (N, t, key)
