"""Directional sensitivities (ltompc_get_jvp) and ltompc_set_u_prev on the GPU: against the contraction of the
handle's own forward trajectories (every instance), the dot-product identity with the adjoint, the structure of the result,
re-packed, with per-instance rows, u_prev as an input (twin, oracle, exact solves), the contract of the entry points (host /
device forms, SplitMPC, usage errors) and the absence of side effects."""
import os

import numpy as np
import pytest

import param_sens_reference as PR
from test_gpu_adjoint import _cotangent, _opts, _repacked, _warm, _record
from test_gpu_sensitivity_dense import _x0_batch

pytestmark = pytest.mark.gpu

# Test 1's measure, per instance and element e of (tX, tU): |jvp_e - ref_e| / sum_j |D_ej| |v_j| (denominator 1 where it is 0), jvp
# the directional pass and ref the float64 contraction of sensitivities(trajectory=True) / param_sensitivities(trajectory=True)
# of the same solve with the same direction.  Both run on one factorisation: rounding, amplified by the conditioning of the
# horizon.  Measured on MI355X over every instance (profiles/jvp/README.md; both modes, a cold solve and two closed-loop ticks;
# directions with dp and dtheta, dp alone, dtheta alone), max and the range of the medians:
#   N = 2  (B = 61)  max 4.07e-9   medians 2.5e-16 .. 4.2e-16
#   N = 10 (B = 13)  max 3.32e-8   medians 2.7e-15 .. 1.3e-10
#   N = 40 (B = 29)  max 4.39e-7   medians 5.6e-10 .. 2.5e-9
#   re-packed (B = 1024, N = 10, every 23rd instance)  max 3.77e-7, median 1.2e-10
#   dp alone after a rollout (B = 128, N = 10)         max 5.77e-8, median 8.6e-13
# (per ELEMENT of the trajectory, each against its own denominator: an element that hardly depends on the direction inherits
# the rounding of its neighbours through A_k, which the adjoint's per-column sums average out.)  The tU[0] rows against the du0
# outputs of the two forward passes, the same measure: at most 9.67e-9 (N = 40).  Each case is held to 10 x its OWN measured
# maximum (the solves and directions are seeded and the kernels have no atomics: the figures repeat from run to run).
JVP_MEASURED = {"N2": 4.07e-9, "N10": 3.32e-8, "N40": 4.39e-7, "repacked": 3.77e-7, "rollout_dp": 5.77e-8}
# Test 2's measure, per instance: |<gX, tX> + <gU, tU> - <grad_p, dp> - <grad_theta, dtheta>| / sum_e |g_e| sum_j |D_ej| |v_j|,
# over the same solves, max per horizon (medians 3.7e-17 .. 1.6e-13); again 10 x each.
DOT_MEASURED = {"N2": 3.59e-16, "N10": 2.75e-13, "N40": 7.32e-11}


def _bound(table, label):
    return 10.0 * table[label.split("_")[0] if label.startswith("N") else label]


def _log(name, text):
    print(name, text)
    f = os.environ.get("LTOMPC_TEST_RATES")
    if f:
        with open(f, "a") as fh:
            fh.write(f"{name} {text}\n")


def _direction(pkg, B, seed):
    """dp (B,10) of unit scale, dtheta (B,16) a seeded relative change of up to 5 % of every parameter."""
    rng = np.random.default_rng(seed)
    th = PR.theta_values(pkg.default_params())
    return rng.standard_normal((B, 10)), rng.uniform(-0.05, 0.05, (B, 16)) * th


def _contract(S, P, dp, dth):
    """float64 contraction of the forward Jacobians with the direction: (tX, tU) and the measure's denominators."""
    z = np.zeros_like
    tX = (np.einsum("bkij,bj->bki", S["dX"], dp) if dp is not None else z(S["dX"][..., 0])) + \
         (np.einsum("bkij,bj->bki", P["dX"], dth) if dth is not None else 0.0)
    tU = (np.einsum("bkij,bj->bki", S["dU"], dp) if dp is not None else z(S["dU"][..., 0])) + \
         (np.einsum("bkij,bj->bki", P["dU"], dth) if dth is not None else 0.0)
    dX = (np.einsum("bkij,bj->bki", np.abs(S["dX"]), np.abs(dp)) if dp is not None else z(S["dX"][..., 0])) + \
         (np.einsum("bkij,bj->bki", np.abs(P["dX"]), np.abs(dth)) if dth is not None else 0.0)
    dU = (np.einsum("bkij,bj->bki", np.abs(S["dU"]), np.abs(dp)) if dp is not None else z(S["dU"][..., 0])) + \
         (np.einsum("bkij,bj->bki", np.abs(P["dU"]), np.abs(dth)) if dth is not None else 0.0)
    return tX, tU, dX, dU


def check_against_forward(mpc, J, dp, dth, label, S, P, rows=None):
    """Tests 1 and 3 on the last solve of mpc: J = mpc.jvp(dp, dth) against the handle's own forward mode, every instance (or
    `rows`).  Returns the largest error."""
    ok = S["ok"]
    assert np.array_equal(J["ok"], ok), label  # bit for bit the forward pass's ok
    assert (J["tX"][~ok] == 0).all() and (J["tU"][~ok] == 0).all(), label
    want0 = (dp[:, :8] if dp is not None else np.zeros((mpc.B, 8))) * ok[:, None]
    assert np.array_equal(J["tX"][:, 0], want0), label  # block 0 is dp[0..7] as it is
    tX, tU, dX, dU = _contract(S, P, dp, dth)
    err = np.concatenate([(np.abs(J["tX"] - tX) / np.where(dX > 0, dX, 1.0)).reshape(mpc.B, -1),
                          (np.abs(J["tU"] - tU) / np.where(dU > 0, dU, 1.0)).reshape(mpc.B, -1)], axis=1)
    # the tU[0] rows reproduce du0_dp dp + du0_dth dtheta (the du0 outputs of the two passes)
    u0 = np.zeros((mpc.B, 2))
    if dp is not None:
        u0 += np.einsum("bij,bj->bi", S["du0_dx0"], dp[:, :8]) + np.einsum("bij,bj->bi", S["du0_duprev"], dp[:, 8:])
    if dth is not None:
        u0 += np.einsum("bij,bj->bi", P["du0_dtheta"], dth)
    e0 = np.abs(J["tU"][:, 0] - u0) / np.where(dU[:, 0] > 0, dU[:, 0], 1.0)
    if rows is not None:
        err, e0 = err[rows], e0[rows]
    e = err.max(axis=1)
    _log(f"jvp_fwd_{label}", f"instances {e.size} ok {int(ok.sum())} err max {e.max():.3e} median {np.median(e):.3e} u0 rows max {e0.max():.3e}")
    assert np.isfinite(J["tX"]).all() and np.isfinite(J["tU"]).all(), label
    assert e.max() <= _bound(JVP_MEASURED, label), (label, e.max(), int(np.argmax(e)))
    assert e0.max() <= _bound(JVP_MEASURED, label), (label, e0.max())
    return e.max()


def check_dot_product(mpc, J, dp, dth, label, S, P, seed):
    """Test 2: <(gX, gU), J v> = <J^T (gX, gU), v> with the adjoint pass of the same solve."""
    gX, gU = _cotangent(mpc.B, mpc.N, seed)
    A = mpc.adjoint(gX, gU)
    lhs = np.einsum("bki,bki->b", gX, J["tX"]) + np.einsum("bkc,bkc->b", gU, J["tU"])
    rhs = np.einsum("bj,bj->b", np.concatenate([A["grad_x0"], A["grad_uprev"]], axis=1), dp) + np.einsum("bj,bj->b", A["grad_theta"], dth)
    _, _, dX, dU = _contract(S, P, dp, dth)
    den = np.einsum("bki,bki->b", np.abs(gX), dX) + np.einsum("bkc,bkc->b", np.abs(gU), dU)
    e = np.abs(lhs - rhs) / np.where(den > 0, den, 1.0)
    _log(f"jvp_dot_{label}", f"instances {e.size} err max {e.max():.3e} median {np.median(e):.3e}")
    assert e.max() <= _bound(DOT_MEASURED, label), (label, e.max(), int(np.argmax(e)))


@pytest.mark.parametrize("N,B", [(2, 61), (10, 13), (40, 29)])
@pytest.mark.parametrize("mode", [1, 2])
def test_jvp_matches_forward_mode_and_the_adjoint(pkg, tables, gpu_lib, N, B, mode):
    """Tests 1, 2 and 3 on the same solves: a cold solve and two closed-loop ticks, both latency modes, B not a multiple of 8
    (padding lanes); N = 2: terminal and first stage only."""
    x = _x0_batch(pkg, tables, B, seed=90 + N)
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    mpc.set_initial_guess(x)
    for t in range(3):
        u = mpc.make_step(x)
        label = f"N{N}_mode{mode}_t{t}"
        dp, dth = _direction(pkg, B, seed=1000 * N + 10 * t + mode)
        J = mpc.jvp(dp, dth)  # (first: the pass makes the factorisation, ok and the right-hand sides itself)
        assert J["tX"].shape == (B, N + 1, 8) and J["tU"].shape == (B, N, 2) and J["ok"].shape == (B,)
        S, P = mpc.sensitivities(trajectory=True), mpc.param_sensitivities(trajectory=True)
        assert S["ok"].sum() >= 8, label
        check_against_forward(mpc, J, dp, dth, label, S, P)
        check_against_forward(mpc, mpc.jvp(dp, None), dp, None, label + "_dp", S, P)
        check_against_forward(mpc, mpc.jvp(None, dth), None, dth, label + "_dth", S, P)
        check_dot_product(mpc, J, dp, dth, label, S, P, seed=7 * N + t)
        x = mpc.plant_step(x, u, 50)
    mpc.close()


def test_exact_zeros_where_ok_is_zero(pkg, tables, gpu_lib):
    """Eight of 16 states outside the track (no feasible point): their ok is 0 and every output exactly 0; the others are not."""
    B, N = 16, 10
    x = pkg.sample_x0(tables, B, seed=23)
    x[1::2, 1] = np.interp(x[1::2, 0], tables.s_arc, tables.n_left) + 1.0
    mpc = pkg.BatchedMPC(tables, N, B)
    mpc.set_initial_guess(x)
    mpc.make_step(x)
    dp, dth = _direction(pkg, B, seed=2)
    J, ok = mpc.jvp(dp, dth), mpc.sensitivities()["ok"]
    assert np.array_equal(J["ok"], ok) and ok.any() and not ok[1::2].any()
    assert (J["tX"][~ok] == 0).all() and (J["tU"][~ok] == 0).all()
    assert np.array_equal(J["tX"][ok, 0], dp[ok, :8]) and (np.abs(J["tU"][ok]).max(axis=(1, 2)) > 0).all()
    mpc.close()


def _same(A, B_, rows=None):
    for k in ("tX", "tU", "ok"):
        a = A[k] if rows is None else A[k][rows]
        assert np.array_equal(a, B_[k]), k


def test_repacked_instances(pkg, tables, gpu_lib):
    """B = 1024 after warm ticks (instances re-packed, asserted): jvp(), iterate() (un-packs: factorisation and right-hand sides
    are no longer at the instances' slots), jvp() again: the same bits, and test 1."""
    mpc, _ = _warm(pkg, tables, 1024, 10, seed=95)
    assert _repacked(mpc), mpc.history()
    dp, dth = _direction(pkg, 1024, seed=3)
    J1 = mpc.jvp(dp, dth)
    mpc.iterate()
    J2 = mpc.jvp(dp, dth)
    _same(J1, J2)
    S, P = mpc.sensitivities(trajectory=True), mpc.param_sensitivities(trajectory=True)
    check_against_forward(mpc, J2, dp, dth, "repacked", S, P, rows=np.arange(0, 1024, 23))
    mpc.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_per_instance_rows(pkg, tables, gpu_lib, mode):
    """Four interleaved theta groups (B = 1024: re-packed, asserted): each group's result is the bits of a uniform handle
    created with that group's params; rows set after the solve do not change it."""
    from test_gpu_instance_params import GROUPS, _params, _row
    G, M, N = len(GROUPS), 256, 10
    B = G * M
    x0 = pkg.sample_x0(tables, B, seed=11)
    rows = np.array([_row(pkg, GROUPS[b % G]) for b in range(B)])
    dp, dth = _direction(pkg, B, seed=4)
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    mpc.set_theta(rows)
    mpc.set_initial_guess(x0)
    mpc.make_step(x0)
    assert _repacked(mpc), mpc.history()
    J, Jp = mpc.jvp(dp, dth), mpc.jvp(dp, None)
    assert J["ok"].mean() > 0.5 and np.array_equal(J["ok"], Jp["ok"])
    for g in range(G):
        u = pkg.BatchedMPC(tables, N, M, params=_params(pkg, rows[g]), options=_opts(pkg, mode))
        u.set_initial_guess(x0[g::G])
        u.make_step(x0[g::G])
        _same(J, u.jvp(dp[g::G], dth[g::G]), rows=slice(g, None, G))
        _same(Jp, u.jvp(dp[g::G], None), rows=slice(g, None, G))
        u.close()
    mpc.set_theta(np.roll(rows, 1, axis=0))  # R2 after the solve with R1: the result stays that of R1
    _same(J, mpc.jvp(dp, dth))
    mpc.close()


# ------------------------------------------------------------------------------------------------------ set_u_prev
def test_set_u_prev_twin_and_host_bookkeeping(pkg, tables, gpu_lib):
    """(a) A twin that sets, before tick 2, exactly the u0 that tick 1 returned gives tick 2's bits (B = 1024: packed instances
    go through orig, asserted); the device form the same; solved_parameters() reports what was set; the warm start, and the
    cached derivatives of the last solve, are untouched by a set."""
    import torch
    B, N = 1024, 10
    x = _x0_batch(pkg, tables, B, seed=96)
    a, b, c = (pkg.BatchedMPC(tables, N, B) for _ in range(3))
    for m in (a, b, c):
        m.set_initial_guess(x)
    u1 = a.make_step(x)
    assert np.array_equal(b.make_step(x), u1) and np.array_equal(c.make_step(x), u1)
    assert _repacked(b), b.history()
    S1 = b.sensitivities()
    dp, dth = _direction(pkg, B, seed=8)
    J1 = b.jvp(dp, dth)
    b.set_u_prev(u1)
    ud = torch.from_numpy(u1).cuda()
    c.set_u_prev_dev(ud.data_ptr())
    # ... the last solve's derivatives are still there, bit for bit (the r_du columns read that solve's u_prev)
    _same(J1, b.jvp(dp, dth))
    assert np.array_equal(S1["du0_duprev"], b.sensitivities()["du0_duprev"])
    x2 = a.plant_step(x, u1, 50)
    ua, ub, uc = a.make_step(x2), b.make_step(x2), c.make_step(x2)
    assert np.array_equal(ua, ub) and np.array_equal(ua, uc)
    for i, (p, q) in enumerate(zip(_record(a, ua), _record(b, ub))):
        assert np.array_equal(p, q), i
    assert np.array_equal(a.history(), b.history()) and np.array_equal(a.history(), c.history())
    assert np.array_equal(b.solved_parameters()[1], u1) and c.solved_parameters() is None
    # another value changes the solve, is reported, and holds for one solve only
    v = u1 + np.array([0.01, -0.02])
    a.set_u_prev(v)
    x3 = a.plant_step(x2, ua, 50)
    u3a, u3b = a.make_step(x3), b.make_step(x3)
    assert np.array_equal(a.solved_parameters()[1], v) and not np.array_equal(u3a, u3b)
    x4 = a.plant_step(x3, u3a, 50)
    a.make_step(x4)
    assert np.array_equal(a.solved_parameters()[1], u3a)
    for m in (a, b, c):
        m.close()


def test_set_u_prev_against_the_oracle(pkg, tables, oracle, gpu_lib):
    """(b) set_initial_guess, set_u_prev(v), make_step against Oracle.solve(x0, N, uprev=v): |u0| within 1e-5 over the
    instances both sides solve (the project's tolerance of the parity tests)."""
    B, N = 16, 20
    x0 = pkg.sample_x0(tables, B, seed=17)
    v = np.random.default_rng(3).uniform(-1.0, 1.0, (B, 2)) * np.array([0.1, 0.5])
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    mpc.set_initial_guess(x0)
    mpc.set_u_prev(v)
    u0 = mpc.make_step(x0)
    assert np.array_equal(mpc.solved_parameters()[1], v)
    ref = oracle.solve(x0, N, uprev=v, nthreads=8)
    both = (mpc.status == 0) & (ref["status"] == 0)
    assert both.mean() >= 0.75, both
    assert np.abs(u0 - ref["u0"])[both].max() < 1e-5
    # ... and it mattered: the cold solve without it differs
    mpc.set_initial_guess(x0)
    assert np.abs(mpc.make_step(x0) - u0)[both].max() > 1e-4
    # a set BEFORE the initial guess is discarded with the rest
    mpc.set_u_prev(v)
    mpc.set_initial_guess(x0)
    u00 = mpc.make_step(x0)
    assert np.array_equal(mpc.solved_parameters()[1], np.zeros((B, 2)))
    mpc.set_initial_guess(x0)
    assert np.array_equal(mpc.make_step(x0), u00)
    mpc.close()


# The step of the exact solves in u_prev = (steering rate, throttle rate).  Confirmed on the CPU first (the oracle's exact solves
# against the dense reference's du0_duprev, the same inputs, filters and criterion): 17 usable instances, 88.2 % of the ratios in
# [3, 5] (median 4.003), every error below 5 % of the move (median error 2.4e-6, median move 1.9e-2).  One combined direction: the
# solve is nearly linear in u_prev[0], so that with a step in the steering rate alone only 7 instances pass the filters at any
# h from 0.1 to 0.8 (their errors stay below 1e-7), one short of the criterion's eight; in the throttle rate alone, h = 0.05
# gives 12 usable, 83 % and 100 %.
UPREV_STEP = np.array([0.2, 0.05])


def test_du0_duprev_against_exact_solves_in_one_batch(pkg, tables, gpu_lib):
    """(c) Exact cold solves at u_prev + h e and u_prev + h/2 e (u_prev = 0, h e = UPREV_STEP) in ONE handle against
    u0 + du0_duprev h e and against u0 + tU[0] of jvp(dp = h e): halving h cuts the error about four-fold.  Inputs, filters and
    criterion of test_gpu_instance_params.test_predictor_against_exact_solves_in_one_batch.  Only u0 is asserted; the ratios of
    the whole trajectory are printed."""
    M, N = 128, 20
    x0 = pkg.sample_x0(tables, M, seed=23)
    base = pkg.BatchedMPC(tables, N, M, options=_opts(pkg, 2))
    base.set_initial_guess(x0)
    u0 = base.make_step(x0)
    Sp, pb = base.sensitivities(), base.params
    st0 = base.stats()["status_solver"]
    X0, U0 = base.prediction()
    v = np.vstack([np.tile(UPREV_STEP, (M, 1)), np.tile(0.5 * UPREV_STEP, (M, 1))])
    ex = pkg.BatchedMPC(tables, N, 2 * M, options=_opts(pkg, 2))
    x2 = np.vstack([x0, x0])
    ex.set_initial_guess(x2)
    ex.set_u_prev(v)
    ue = ex.make_step(x2)
    sts = ex.stats()["status_solver"]
    Xe, Ue = ex.prediction()
    ex.close()
    u1, uh = ue[:M], ue[M:]
    dp = np.zeros((M, 10))
    dp[:, 8:] = UPREV_STEP
    J = base.jvp(dp, None)
    base.close()
    lo, hi = np.array([pb.u_lb[0], pb.u_lb[1]]), np.array([pb.u_ub[0], pb.u_ub[1]])
    act = [(np.abs(w - lo) < 1e-6) | (np.abs(w - hi) < 1e-6) for w in (u0, u1, uh)]
    same = (act[0] == act[1]).all(axis=1) & (act[0] == act[2]).all(axis=1)
    conv = (st0 == 0) & (sts[:M] == 0) & (sts[M:] == 0)
    move = np.abs(u1 - u0).max(axis=1)
    lin = np.einsum("bij,j->bi", Sp["du0_duprev"], UPREV_STEP)
    for name, p1, ph in (("du0_duprev", u0 + lin, u0 + 0.5 * lin), ("jvp", u0 + J["tU"][:, 0], u0 + 0.5 * J["tU"][:, 0])):
        e1, eh = np.abs(u1 - p1).max(axis=1), np.abs(uh - ph).max(axis=1)
        use = Sp["ok"] & (Sp["margin"] >= 1e-3) & conv & same & (eh > 1e-7) & (e1 > 1e-7)
        ratio = e1[use] / eh[use]
        _log(f"uprev_exact_{name}", f"usable {use.sum()} ratio in [3,5] {np.mean((ratio >= 3) & (ratio <= 5)):.3f} "
             f"below 0.05 {np.mean(e1[use] / move[use] < 0.05):.3f} ratio median {np.median(ratio):.3f}")
        assert use.sum() >= 8, (name, use.sum())
        assert np.mean((ratio >= 3.0) & (ratio <= 5.0)) >= 0.75, (name, np.sort(ratio))
        assert np.mean(e1[use] / move[use] < 0.05) >= 0.75, (name, e1[use] / move[use])
    # the whole trajectory, recorded only
    for name, Ze, Z0, tZ in (("X", Xe, X0, J["tX"]), ("U", Ue, U0, J["tU"])):
        e1 = np.abs(Ze[:M] - Z0 - tZ).max(axis=(1, 2))
        eh = np.abs(Ze[M:] - Z0 - 0.5 * tZ).max(axis=(1, 2))
        use = Sp["ok"] & (Sp["margin"] >= 1e-3) & conv & same & (eh > 1e-7) & (e1 > 1e-7)
        ratio = e1[use] / eh[use]
        _log(f"uprev_exact_trajectory_{name}", f"usable {use.sum()} ratio median {np.median(ratio):.3f} in [3,5] {np.mean((ratio >= 3) & (ratio <= 5)):.3f}")


def test_set_u_prev_usage_errors(pkg, tables, gpu_lib):
    """(d) non-finite rows (named, nothing changed), null arguments, a wrong shape."""
    L = gpu_lib
    B, N = 16, 10
    x = pkg.sample_x0(tables, B, seed=5)
    a, b = pkg.BatchedMPC(tables, N, B), pkg.BatchedMPC(tables, N, B)
    for m in (a, b):
        m.set_initial_guess(x)
        m.make_step(x)
    bad = np.zeros((B, 2))
    bad[11, 1] = np.nan
    with pytest.raises(pkg.LtompcError, match="instance 11"):
        a.set_u_prev(bad)
    assert L.ltompc_set_u_prev(a._h, None) != 0 and b"null argument" in L.ltompc_last_error()
    assert L.ltompc_set_u_prev_dev(a._h, None) != 0 and b"null argument" in L.ltompc_last_error()
    with pytest.raises(ValueError):
        a.set_u_prev(np.zeros((B + 1, 2)))
    assert np.array_equal(a.make_step(x), b.make_step(x))  # (no trace of the refused calls)
    sp = pkg.SplitMPC(tables, N, B, n_parts=2)
    with pytest.raises(ValueError, match="instance 11"):
        sp.set_u_prev(bad)
    sp.close()
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------ contract
def test_contract(pkg, tables, gpu_lib):
    """Device forms equal the host forms bit for bit; SplitMPC equals one handle (jvp and set_u_prev); the usage errors."""
    import torch
    L = gpu_lib
    dev = torch.device("cuda", 0)
    B, N = 1024, 10
    x = _x0_batch(pkg, tables, B, seed=96)
    mpc = pkg.BatchedMPC(tables, N, B)
    dp, dth = _direction(pkg, B, seed=5)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        mpc.jvp(dp, dth)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        mpc.jvp(dp, None)
    assert L.ltompc_jvp_dev(mpc._h, None, None, None, None, None) != 0
    mpc.set_initial_guess(x)
    for _ in range(2):
        u = mpc.make_step(x)
        x = mpc.plant_step(x, u, 50)
    assert _repacked(mpc), mpc.history()
    J = mpc.jvp(dp, dth)
    dpd, dthd = torch.from_numpy(dp).to(dev), torch.from_numpy(dth).to(dev)
    tX = torch.full((B, N + 1, 8), np.nan, dtype=torch.float64, device=dev)
    tU = torch.full((B, N, 2), np.nan, dtype=torch.float64, device=dev)
    ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (torch's fills run on torch's stream, the handle on its own: order them)
    mpc.jvp_dev(dpd.data_ptr(), dthd.data_ptr(), tX.data_ptr(), tU.data_ptr(), ok.data_ptr())
    mpc.synchronize()
    assert np.array_equal(tX.cpu().numpy(), J["tX"]) and np.array_equal(tU.cpu().numpy(), J["tU"])
    assert np.array_equal(ok.cpu().numpy() != 0, J["ok"])
    # one of the directions absent = zeros
    _same(mpc.jvp(dp, None), mpc.jvp(dp, np.zeros_like(dth)))
    _same(mpc.jvp(None, dth), mpc.jvp(np.zeros_like(dp), dth))
    tU.fill_(np.nan)
    torch.cuda.synchronize()  # (torch's fills run on torch's stream, the handle on its own: order them)
    mpc.jvp_dev(0, dthd.data_ptr(), 0, tU.data_ptr())
    mpc.synchronize()
    assert np.array_equal(tU.cpu().numpy(), mpc.jvp(None, dth)["tU"])
    # usage errors: no direction, a non-finite direction (names the instance), a wrong shape, after an initial guess
    with pytest.raises(pkg.LtompcError, match="both NULL"):
        mpc.jvp(None, None)
    assert L.ltompc_jvp_dev(mpc._h, None, None, None, None, None) != 0 and b"both NULL" in L.ltompc_last_error()
    bad = dth.copy()
    bad[37, 3] = np.inf
    with pytest.raises(pkg.LtompcError, match="instance 37"):
        mpc.jvp(dp, bad)
    with pytest.raises(ValueError):
        mpc.jvp(dp[:, :8], None)
    _same(J, mpc.jvp(dp, dth))  # (no trace of the refused calls)
    mpc.set_initial_guess(x)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        mpc.jvp(dp, None)
    mpc.close()
    # handles whose problem theta does not cover: dtheta refused with the forward pass's wording, dp alone works
    for field, value in (("ell_penalty", 1e3), ("ptv", 10.0)):
        p = pkg.default_params()
        setattr(p, field, value)
        if field == "ell_penalty":
            p.ell_rho, p.ell_D_f, p.ell_D_r = 1.0, 5000.0, 5000.0
        m3 = pkg.BatchedMPC(tables, N, 8, params=p)
        m3.set_initial_guess(x[:8])
        m3.make_step(x[:8])
        with pytest.raises(pkg.LtompcError, match=field):
            m3.jvp(dp[:8], dth[:8])
        J3, S3 = m3.jvp(dp[:8], None), m3.sensitivities(trajectory=True)
        assert np.array_equal(J3["ok"], S3["ok"])
        m3.close()
    # after a rollout: dp alone works (test 1's measure), dtheta is refused
    M = 128
    m4 = pkg.BatchedMPC(tables, N, M)
    xs = torch.from_numpy(_x0_batch(pkg, tables, M, seed=44)).to(dev)
    m4.set_initial_guess_dev(xs.data_ptr())
    m4.rollout_dev(xs.data_ptr(), 2, 50)
    with pytest.raises(pkg.LtompcError, match="rollout"):
        m4.jvp(dp[:M], dth[:M])
    J4, S4 = m4.jvp(dp[:M], None), m4.sensitivities(trajectory=True)
    assert J4["ok"].mean() > 0.5
    check_against_forward(m4, J4, dp[:M], None, "rollout_dp", S4, dict(dX=None, dU=None))
    m4.close()
    # SplitMPC with 4 parts: the same bits as one handle (SplitMPC with 1 part); host and device entry points, set_u_prev
    Y = _x0_batch(pkg, tables, 512, seed=98)
    v = np.random.default_rng(9).uniform(-0.1, 0.1, (512, 2))
    out = []
    for parts in (1, 4):
        sp = pkg.SplitMPC(tables, N, 512, n_parts=parts)
        xa = torch.from_numpy(Y).to(dev)
        ua = torch.zeros(512, 2, dtype=torch.float64, device=dev)
        sp.set_initial_guess_dev(xa.data_ptr())
        sp.set_u_prev(v)
        sp.make_step_dev(xa.data_ptr(), ua.data_ptr())
        sp.synchronize()
        T = sp.jvp(dp[:512], dth[:512])
        a, b_ = torch.from_numpy(np.ascontiguousarray(dp[:512])).to(dev), torch.from_numpy(np.ascontiguousarray(dth[:512])).to(dev)
        tX = torch.zeros((512, N + 1, 8), dtype=torch.float64, device=dev)
        tU = torch.zeros((512, N, 2), dtype=torch.float64, device=dev)
        oks = torch.zeros((512,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # (torch's fills run on torch's stream, the handle on its own: order them)
        sp.jvp_dev(a.data_ptr(), b_.data_ptr(), tX.data_ptr(), tU.data_ptr(), oks.data_ptr())
        sp.synchronize()
        assert np.array_equal(tX.cpu().numpy(), T["tX"]) and np.array_equal(tU.cpu().numpy(), T["tU"])
        assert np.array_equal(oks.cpu().numpy() != 0, T["ok"])
        # the device form of the setter: the same solve again
        u_first = ua.cpu().numpy()
        vd = torch.from_numpy(v).to(dev)
        sp.set_initial_guess_dev(xa.data_ptr())
        sp.set_u_prev_dev(vd.data_ptr())
        sp.make_step_dev(xa.data_ptr(), ua.data_ptr())
        sp.synchronize()
        assert np.array_equal(ua.cpu().numpy(), u_first)
        out.append((T, u_first))
        sp.close()
    _same(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])
    # ... and u_prev mattered
    one = pkg.BatchedMPC(tables, N, 512)
    one.set_initial_guess(Y)
    assert not np.array_equal(one.make_step(Y), out[0][1])
    one.set_initial_guess(Y)
    one.set_u_prev(v)
    assert np.array_equal(one.make_step(Y), out[0][1])
    one.close()


def test_no_side_effects(pkg, tables, gpu_lib):
    """A handle that asks for the directional pass after every tick (before or after the other passes, host and device forms)
    gives the bits of a twin that never does: u0, statuses, iterations, prediction, the whole iterate, the poll history, both
    forward passes and the adjoint, over six closed-loop ticks and a rollout."""
    import torch
    dev = torch.device("cuda", 0)
    B, N = 600, 10
    x = _x0_batch(pkg, tables, B, seed=43)
    dp, dth = _direction(pkg, B, seed=6)
    gX, gU = _cotangent(B, N, seed=6)
    dpd, dthd = torch.from_numpy(dp).to(dev), torch.from_numpy(dth).to(dev)
    tX = torch.zeros(B, N + 1, 8, dtype=torch.float64, device=dev)
    tU = torch.zeros(B, N, 2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()  # (torch's fills run on torch's stream, the handle on its own: order them)
    a, b = pkg.BatchedMPC(tables, N, B), pkg.BatchedMPC(tables, N, B)
    a.set_initial_guess(x), b.set_initial_guess(x)
    xa, xb = x.copy(), x.copy()

    def ask():
        b.jvp_dev(dpd.data_ptr(), dthd.data_ptr(), tX.data_ptr(), tU.data_ptr())
        b.jvp(dp, dth)
        b.jvp(dp, None)

    for tick in range(6):
        ua, ub = a.make_step(xa), b.make_step(xb)
        if tick % 2:  # the directional pass first (it runs the factorisation, the ok pass and the right-hand sides) ...
            ask()
            Sb, Pb, Ab = b.sensitivities(trajectory=True), b.param_sensitivities(trajectory=True), b.adjoint(gX, gU)
        else:  # ... or after the other passes (it reuses them)
            Sb, Pb, Ab = b.sensitivities(trajectory=True), b.param_sensitivities(trajectory=True), b.adjoint(gX, gU)
            ask()
        b.synchronize()
        Sa, Pa, Aa = a.sensitivities(trajectory=True), a.param_sensitivities(trajectory=True), a.adjoint(gX, gU)
        for k in Sa:
            assert np.array_equal(Sa[k], Sb[k]), (tick, k)
        for k in Pa:
            assert np.array_equal(Pa[k], Pb[k]), (tick, k)
        for k in Aa:
            assert np.array_equal(Aa[k], Ab[k]), (tick, k)
        assert np.array_equal(a.history(), b.history()), tick
        for i, (p, q) in enumerate(zip(_record(a, ua), _record(b, ub))):
            assert np.array_equal(p, q), (tick, i)
        xa, xb = a.plant_step(xa, ua, 50), b.plant_step(xb, ub, 50)
    a.close(), b.close()
    M = 128
    x = _x0_batch(pkg, tables, M, seed=44)
    a, b = pkg.BatchedMPC(tables, N, M), pkg.BatchedMPC(tables, N, M)
    ta, tb = torch.from_numpy(x).to(dev), torch.from_numpy(x).to(dev)
    for m, t in ((a, ta), (b, tb)):
        m.set_initial_guess(x)
        m.rollout_dev(t.data_ptr(), 2, 50)
    b.jvp(dp[:M], None)
    Sa, Sb = a.sensitivities(trajectory=True), b.sensitivities(trajectory=True)
    for k in Sa:
        assert np.array_equal(Sa[k], Sb[k]), k
    for m, t in ((a, ta), (b, tb)):  # a rollout after it
        m.rollout_dev(t.data_ptr(), 2, 50)
    xs = ta.cpu().numpy()
    assert np.array_equal(xs, tb.cpu().numpy())
    ua, ub = a.make_step(xs), b.make_step(xs)
    for i, (p, q) in enumerate(zip(_record(a, ua), _record(b, ub))):
        assert np.array_equal(p, q), i
    a.close(), b.close()
