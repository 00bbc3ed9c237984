"""The narrow-launch kernels (k_riccati1q, k_riccati1, k_step1 and their _pi forms) at the horizons where their loops change
shape.  A batch of 12 (<= 16) runs k_riccati1q and k_step1 from the first iteration; the rest of the suite solves at N = 10, 20,
40 and 60, where none of the remainder branches below runs:
  N = 3    d_riccati1q's staging loop (`k0 += 8`) makes one round, and that round is a clamped remainder;
  N = 11   a full round, then a remainder of 3;
  N = 41   N * n_linesearch = 328 > 320: the first horizon at which k_step1's `idx += 320` loop makes a second, partial pass;
  N = 79   the largest horizon whose stage blocks k_riccati1 / k_riccati1q still stage in LDS (ric1q_lds_bytes(79) = 152 776 of
           the 153 600 bytes of the cap).  The formula's constants are not visible from Python, so instead of deriving 79 the
           tests assert that the default run launches class `riccati1` at N = 79 and that N = 80 does not.
Inputs: x0 = sample_x0(tables, 12, seed=83); a cold tick, then a warm tick from the state the oracle's control leads to, the
previous input of both sides being the oracle's control (the two sides then solve the same NLP).  On these inputs the oracle
solves 12 of 12 at N = 3 and 11 and 11 of 12 at N = 41 and 79 on both ticks: instance 5 ends INFEASIBLE after some hundred
iterations, so the restoration phase and the in-launch sweep retries run through the narrow kernels as well.
Every run creates its own handle and closes it; the oracle's results and the default run are made once per horizon and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 12
HORIZONS = (3, 11, 41, 79)


@pytest.fixture(scope="module")
def x_cold(pkg, tables):
    return pkg.sample_x0(tables, B, seed=83)


@pytest.fixture(scope="module")
def reference(oracle, x_cold):
    """Per horizon, made once: the oracle's cold and warm results and the two ticks' states."""
    cache = {}

    def get(N):
        if N not in cache:
            cold = oracle.solve(x_cold, N, nthreads=8)
            x_warm = oracle.plant_step(x_cold, cold["u0"], n_sub=100)
            warm = oracle.solve(x_warm, N, uprev=cold["u0"], warm=cold, nthreads=8, prev_status=cold["status"])
            cache[N] = dict(x=(x_cold, x_warm), ref=(cold, warm))
        return cache[N]
    return get


def _solve(pkg, tables, N, ref, rows=False, profile=False):
    """A cold and a warm tick on a fresh handle: per tick u0, status, iterations and kkt; with profile=True also the cold tick's
    iterate and the launch counts by kernel class."""
    m = pkg.BatchedMPC(tables, N, B)
    try:
        if rows:
            m.set_theta(np.tile(m.theta(), (B, 1)))
        if profile:
            m.set_profiling(True)
        m.set_initial_guess(ref["x"][0])
        out = dict(ticks=[])
        for t, x in enumerate(ref["x"]):
            if t:
                m.set_u_prev(ref["ref"][0]["u0"])
            u0 = m.make_step(x)
            s = m.stats()
            out["ticks"].append(dict(u0=u0.copy(), status=s["status"].copy(), iters=s["iters"].copy(), kkt=s["kkt"].copy()))
            if t == 0 and profile:
                out["iterate"], out["smooth_eps_min"] = m.iterate(), m.options.smooth_eps_min
        if profile:
            out["launches"] = m.timing()["launches_by_kernel"]
        return out
    finally:
        m.close()


@pytest.fixture(scope="module")
def default_run(pkg, tables, gpu_lib, reference):
    cache = {}

    def get(N):
        if N not in cache:
            cache[N] = _solve(pkg, tables, N, reference(N), profile=True)
        return cache[N]
    return get


def _assert_same_bits(a, b, label):
    """The rule of test_compaction_and_serial_riccati_do_not_change_results: u0 and status on every instance, iterations and kkt
    where solved."""
    for t, (p, q) in enumerate(zip(a["ticks"], b["ticks"])):
        assert np.array_equal(p["u0"], q["u0"]) and np.array_equal(p["status"], q["status"]), (label, t)
        solved = q["status"] == 0
        assert np.array_equal(p["iters"][solved], q["iters"][solved]) and np.array_equal(p["kkt"][solved], q["kkt"][solved]), (label, t)
    assert len(a["ticks"]) == len(b["ticks"]) == 2


@pytest.mark.parametrize("N", HORIZONS)
def test_edge_horizons_match_the_oracle_on_the_narrow_kernels(default_run, reference, N):
    """The default handle against the oracle on both ticks: statuses equal on all 12 instances, u0 within 1e-5 where both solved
    (the batch rule of test_batch_cold_and_warm_ticks), at least 11 of 12 solved by both; and the launches were those of
    k_riccati1q / k_riccati1 (class riccati1) and k_step1, never k_riccati8 - also at N = 79, which could otherwise fall back
    silently and prove nothing."""
    run, ref = default_run(N), reference(N)["ref"]
    ln = run["launches"]
    print(f"N={N}: launches {ln}")
    assert ln["riccati1"] > 0 and ln["step1"] > 0 and ln["riccati"] == 0, ln
    assert ln["linesearch"] == 0 and ln["pick"] == 0 and ln["update"] == 0, ln
    for t, (g, r) in enumerate(zip(run["ticks"], ref)):
        both = (g["status"] == 0) & (r["status"] == 0)
        err = np.abs(g["u0"] - r["u0"])[both].max()
        print(f"N={N} tick {t}: status gpu {g['status'].tolist()} oracle {r['status'].tolist()}, iterations gpu {g['iters'].tolist()} "
              f"oracle {r['iters'].tolist()}, max |u0 - oracle| where both solved {err:.3e}")
        assert np.array_equal(g["status"], r["status"]), (t, g["status"], r["status"])
        assert both.sum() >= 11, (t, both.sum())
        assert err < 1e-5, (t, err)


@pytest.mark.parametrize("N", HORIZONS)
def test_edge_horizon_solutions_satisfy_the_kkt_conditions(default_run, reference, tables, N):
    """Independent of the algorithm: two solved instances of the cold tick through nlp_reference.kkt_residuals, with the
    thresholds of test_kkt_conditions_of_gpu_solution."""
    import nlp_reference as R
    run, x = default_run(N), reference(N)["x"][0]
    solved = np.flatnonzero(run["ticks"][0]["status"] == 0)[:2]
    assert len(solved) == 2
    for b in solved:
        k = R.kkt_residuals(run["iterate"], x[b], np.zeros(2), tables, run["smooth_eps_min"], int(b))
        print(f"N={N} instance {b}: {k}")
        assert k["stationarity"] < 1e-6 and k["equality"] < 1e-7, (b, k)
        assert k["ineq_violation"] < 1e-7 and k["complementarity"] < 1e-7 and k["min_multiplier"] >= 0.0, (b, k)


@pytest.mark.parametrize("N", HORIZONS)
def test_edge_horizon_kernel_paths_agree_bit_for_bit(pkg, tables, default_run, reference, monkeypatch, N):
    """The default path (k_riccati1q, k_step1) against k_riccati1 (LTOMPC_RIC1Q=0) and against k_riccati8 with the separate
    line-search / pick / update launches (LTOMPC_RIC1=0, LTOMPC_STEP1=0)."""
    run, ref = default_run(N), reference(N)
    monkeypatch.setenv("LTOMPC_RIC1Q", "0")
    one_wave = _solve(pkg, tables, N, ref, profile=True)
    assert one_wave["launches"]["riccati1"] > 0 and one_wave["launches"]["riccati"] == 0, one_wave["launches"]
    _assert_same_bits(one_wave, run, "k_riccati1")
    monkeypatch.delenv("LTOMPC_RIC1Q")
    monkeypatch.setenv("LTOMPC_RIC1", "0")
    monkeypatch.setenv("LTOMPC_STEP1", "0")
    wide = _solve(pkg, tables, N, ref, profile=True)
    ln = wide["launches"]
    assert ln["riccati1"] == 0 and ln["step1"] == 0 and ln["riccati"] > 0 and ln["linesearch"] > 0 and ln["update"] > 0, ln
    _assert_same_bits(wide, run, "k_riccati8 and separate launches")


@pytest.mark.parametrize("N", (11, 79))
def test_edge_horizon_rows_equal_to_the_params_give_the_same_bits(pkg, tables, default_run, reference, N):
    """Per-instance rows equal to the handle's own parameters: k_riccati1q_pi and k_step1_pi, bit-identical to the uniform handle
    (test_rows_equal_to_the_params_give_the_same_bits at the remainder horizons)."""
    rows = _solve(pkg, tables, N, reference(N), rows=True, profile=True)
    ln = rows["launches"]
    assert ln["riccati1"] > 0 and ln["step1"] > 0 and ln["riccati"] == 0, ln
    _assert_same_bits(rows, default_run(N), "rows")
    for k in rows["iterate"]:
        assert np.array_equal(rows["iterate"][k], default_run(N)["iterate"][k]), k


def test_one_stage_past_the_lds_cap_falls_back(pkg, tables, gpu_lib, x_cold):
    """N = 80 does not stage in LDS: no launch of class riccati1, k_riccati8 instead (with N = 79 above: 79 is the largest
    horizon that does).  A budget of 5 iterations: which kernels run does not depend on how far the solve gets."""
    o = pkg.default_options()
    o.max_iter = 5
    m = pkg.BatchedMPC(tables, 80, B, options=o)
    try:
        m.set_profiling(True)
        m.set_initial_guess(x_cold)
        m.make_step(x_cold)
        ln = m.timing()["launches_by_kernel"]
    finally:
        m.close()
    assert ln["riccati1"] == 0 and ln["riccati"] > 0 and ln["step1"] > 0, ln
