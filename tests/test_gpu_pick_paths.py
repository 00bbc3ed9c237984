"""d_pick (filter test, step length, recovery bookkeeping) and d_head8 (termination test, barrier update) keep the per-instance
state in registers: one batch of loads, the decisions, one group of stores.  Every kernel path calls the same two device functions
but schedules them differently - k_pick as two launches per iteration of 8 instances per wavefront with the list of rejected
full steps between them, k_step1 as one call per workgroup; the head in k_riccati8, k_riccati1 and k_riccati1q - so the paths
must agree bit for bit, and the wide path with the oracle, on states that reach the rare branches: a line search that fails,
the shifted restart / the restoration phase, a solve that does not end SOLVED.

The states (N = 10): pkg.sample_x0(tables, 72, seed=4) with the lateral position of the first four moved to 0.90, -0.95, 0.99 and
-1.02 of the half-width of the band the sampler uses (the last one is outside it).  Seeds 1..24 were tried with the oracle on
the CPU; seed 4 is the first whose three ticks hold a failed line search, a shifted restart or restoration phase and both a
STALLED and an INFEASIBLE solve, with at most one solve per tick that does not converge (the tolerances below allow two)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SEED = 10, 4
WIDE = {"LTOMPC_STEP1": "0", "LTOMPC_RIC1": "0"}  # k_riccati8 + k_linesearch / k_pick / k_update at every launch width


def _states(pkg, tables, B=72):
    x = pkg.sample_x0(tables, B, seed=SEED)
    s = x[:4, 0]
    nl, nr = np.interp(s, tables.s_arc, tables.n_left), np.interp(s, tables.s_arc, tables.n_right)
    mid, w = 0.5 * (nl - nr), 0.5 * (nl + nr - 2.3)
    x[:4, 1] = mid + np.array([0.9, -0.95, 0.99, -1.02]) * w
    return x


def _closed_loop(pkg, tables, x0, ticks):
    m = pkg.BatchedMPC(tables, N, x0.shape[0])
    m.set_initial_guess(x0)
    x, out = x0.copy(), []
    for _ in range(ticks):
        u = m.make_step(x)
        st = m.stats()
        out.append(dict(u0=u.copy(), status=st["status"].copy(), iters=st["iters"].copy(), n_resto=st["n_resto"].copy(),
                        n_shift=st["n_shift"].copy(), it=m.iterate()))
        x = m.plant_step(x, u, 100)
    m.close()
    return out


def test_narrow_and_wide_paths_agree_bit_for_bit(pkg, tables, oracle, gpu_lib, monkeypatch):
    """B = 12 (the four states at the edge of the band among them), 6 closed-loop ticks: the default path of a batch this
    small (k_riccati1q + k_step1) against the wide kernels - controls, statuses, iteration counts, the recovery counters and
    the whole iterate."""
    x0 = _states(pkg, tables)[:12]
    # the oracle's own closed loop on these states first: it has to leave the common path (n_lsfail: searches in which every
    # candidate was rejected, the full step first - the oracle's only record of rejected full steps)
    x, up, o, n_rej, n_rec, n_bad = x0.copy(), np.zeros((12, 2)), None, 0, 0, 0
    for _ in range(6):
        o = oracle.solve(x, N, uprev=up, warm=o, nthreads=8, prev_status=None if o is None else o["status"])
        n_rej, n_rec, n_bad = n_rej + int((o["n_lsfail"] >= 1).sum()), n_rec + int(((o["n_resto"] + o["n_shift"]) >= 1).sum()), n_bad + int((o["status"] != 0).sum())
        x, up = oracle.plant_step(x, o["u0"], n_sub=100), o["u0"]
    assert n_rej >= 1 and n_rec >= 1 and n_bad >= 1, (n_rej, n_rec, n_bad)
    ref = _closed_loop(pkg, tables, x0, 6)
    for k, v in WIDE.items():
        monkeypatch.setenv(k, v)
    got = _closed_loop(pkg, tables, x0, 6)
    # (... and so does the GPU's run)
    assert sum(int((r["status"] != 0).sum()) for r in ref) >= 1
    assert sum(int(((r["n_resto"] + r["n_shift"]) >= 1).sum()) for r in ref) >= 1
    for t, (a, b) in enumerate(zip(ref, got)):
        for key in ("u0", "status", "iters", "n_resto", "n_shift"):
            assert np.array_equal(a[key], b[key]), (t, key)
        for key in a["it"]:
            assert np.array_equal(a["it"][key], b["it"][key], equal_nan=True), (t, key)


def test_wide_path_with_rejected_steps_matches_oracle(pkg, tables, oracle, gpu_lib, monkeypatch):
    """B = 72 on the wide kernels (a last wavefront of 8 instances in the thread-per-slot kernels, lists of rejected full steps
    of a few instances), cold start and two warm ticks on the oracle's states, with the tolerances of
    test_gpu_parity.test_config_c3_batch_1024."""
    x0 = _states(pkg, tables)
    B = x0.shape[0]
    # the oracle's own run first: it has to contain what this test is about (n_lsfail: searches in which every candidate was
    # rejected, the full step first - the oracle's only record of rejected full steps)
    refs, x, up, ref = [], x0.copy(), np.zeros((B, 2)), None
    for _ in range(3):
        ref = oracle.solve(x, N, uprev=up, warm=ref, nthreads=8, prev_status=None if ref is None else ref["status"])
        refs.append((x, ref))
        x, up = oracle.plant_step(x, ref["u0"]), ref["u0"]
    assert sum(int((r["n_lsfail"] >= 1).sum()) for _, r in refs) >= 1
    assert sum(int(((r["n_resto"] + r["n_shift"]) >= 1).sum()) for _, r in refs) >= 1
    assert sum(int((r["status"] != 0).sum()) for _, r in refs) >= 1
    for k, v in WIDE.items():
        monkeypatch.setenv(k, v)
    m = pkg.BatchedMPC(tables, N, B)
    m.set_initial_guess(x0)
    try:
        for tick, (x, ref) in enumerate(refs):
            u0 = m.make_step(x)
            st = m.stats()
            both = (st["status"] == 0) & (ref["status"] == 0)
            print("tick", tick, "both", both.mean(), "status equal", (st["status"] == ref["status"]).mean(),
                  "max |u0 - oracle|", np.abs(u0 - ref["u0"])[both].max(), "iters within 2", (np.abs(st["iters"] - ref["iters"])[both] <= 2).mean())
            assert both.mean() >= 0.97, (tick, both.mean())
            assert (st["status"] == ref["status"]).mean() >= 0.98, tick
            assert np.abs(u0 - ref["u0"])[both].max() < 1e-5, tick
            assert (np.abs(st["iters"] - ref["iters"])[both] <= 2).mean() >= 0.95, tick
        assert max(h[2] for h in m.history()) == B
    finally:
        m.close()
