"""The feedback policy of a solve (ltompc_get_policy, ltompc_policy_step, ltompc_policy_run_dev) on the GPU: the
stage gains against the dense reference on the tail problems (policy_reference.py), the identities with sensitivities(), the
step against the formula in numpy, the run against the loop of step and plant step bit for bit, no side effects on the next
solve (also with re-packed instances), records, and SplitMPC with the multi-rate run_ticks."""
import numpy as np
import pytest

import policy_reference as PR
import sens_reference as SR
from test_gpu_sensitivity_dense import CAP, MEDIAN_CAP, SOLVED_OR_ACCEPTABLE, _eps, _x0_batch

pytestmark = pytest.mark.gpu

N = 10
# _x0_batch(seed=SEED): on the CPU oracle alone, at N = 10, the share of instances whose solver status is SOLVED or ACCEPTABLE is
# 0.90 / 0.90 / 0.93 for B = 29 and 0.91 / 0.93 / 0.93 for B = 70 in the cold solve and the two closed-loop ticks after it (plant
# steps of 50 sub-steps); at least 0.6 is required below.
SEED = 80
EPSM = 2.0 ** -52
KS = (0, 1, 5, 9)


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t if dtype is None else t.to(dtype)


def _sync():
    import torch
    torch.cuda.synchronize()  # (torch's copies run on torch's stream, the handle on its own: order them)


def _solved(pkg, tables, B, ticks=0, options=None, seed=SEED, prepare=None):
    """A handle after a cold make_step and `ticks` closed-loop ticks; returns it and the state of its last solve."""
    x = _x0_batch(pkg, tables, B, seed)
    mpc = pkg.BatchedMPC(tables, N, B, options=options)
    if prepare is not None:
        prepare(mpc)
    mpc.set_initial_guess(x)
    u = mpc.make_step(x)
    for _ in range(ticks):
        x = mpc.plant_step(x, u, 50)
        u = mpc.make_step(x)
    return mpc, x


@pytest.fixture(scope="module")
def solved13(pkg, tables, gpu_lib):
    """One handle of 13 instances after two closed-loop ticks (u_prev != 0), shared by the tests that only read it."""
    mpc, x = _solved(pkg, tables, 13, ticks=2)
    yield mpc, x
    mpc.close()


def _formula(P, X, U, up, k, x, v):
    """pi_k in numpy and the a-priori bound's magnitude |U_k| + |K||x - X_k| + |Kv||v - V_k|."""
    Vk = up if k == 0 else U[:, k - 1]
    dx, dv = x - X[:, k], v - Vk
    u = U[:, k] + np.einsum("bij,bj->bi", P["K"][:, k], dx) + np.einsum("bij,bj->bi", P["Kv"][:, k], dv)
    mag = np.abs(U[:, k]) + np.einsum("bij,bj->bi", np.abs(P["K"][:, k]), np.abs(dx)) + np.einsum("bij,bj->bi", np.abs(P["Kv"][:, k]), np.abs(dv))
    return u, mag


def _clip(p, t_step, x, u):
    u = u.copy()
    for i in range(2):
        if p.x_lb[6 + i] > -1e30:
            u[:, i] = np.maximum(u[:, i], (p.x_lb[6 + i] - x[:, 6 + i]) / t_step)
        if p.x_ub[6 + i] < 1e30:
            u[:, i] = np.minimum(u[:, i], (p.x_ub[6 + i] - x[:, 6 + i]) / t_step)
        if p.u_lb[i] > -1e30:
            u[:, i] = np.maximum(u[:, i], p.u_lb[i])
        if p.u_ub[i] < 1e30:
            u[:, i] = np.minimum(u[:, i], p.u_ub[i])
    return u


# ---- 1. the gains against the dense reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", [(1, 29), (2, 70)])
def test_gains_match_the_dense_reference_on_the_tail_problems(pkg, tables, gpu_lib, mode, B):
    """K_k, Kv_k at k in KS against sens_reference._solve on the stage slices [k:], cold and after two closed-loop ticks; the
    criteria of test_gpu_sensitivity_dense.py with the slice's gap and the instance's margin."""
    o = pkg.default_options()
    o.latency_mode = mode
    params = pkg.default_params()
    x = _x0_batch(pkg, tables, B, SEED)
    mpc = pkg.BatchedMPC(tables, N, B, options=o)
    mpc.set_initial_guess(x)
    for t in range(3):
        u = mpc.make_step(x)
        if t in (0, 2):
            if t:
                assert np.abs(mpc.solved_parameters()[1]).max() > 0  # (Kv at a real u_prev)
            P, S = mpc.policy(), mpc.sensitivities()
            st, it = mpc.stats(), mpc.iterate()
            x0, up, _ = mpc.solved_parameters()
            conv = np.isin(st["status_solver"], SOLVED_OR_ACCEPTABLE)
            assert conv.sum() >= 0.6 * B, (t, conv.sum())
            idx = np.flatnonzero(conv)[:12]
            eps = _eps(mpc, st, conv)
            R = PR.gains_batch({k: v[idx] for k, v in it.items()}, x0[idx], up[idx], tables, eps, params, KS)
            err, gaps, mg = [], [], []
            for b, r in zip(idx, R):
                for k in KS:
                    assert r[k]["backward"] < 1e-16, (t, b, k, r[k]["backward"])
                if not P["ok"][b]:
                    continue
                for k in KS:
                    G = np.concatenate([P["K"][b, k], P["Kv"][b, k]], axis=1)
                    D = r[k]["du0"]
                    err.append((np.abs(G - D) / np.maximum(1.0, np.abs(D))).max()), gaps.append(r[k]["gap"]), mg.append(S["margin"][b])
            err, gaps, mg = np.array(err), np.array(gaps), np.array(mg)
            print(f"mode {mode} B {B} tick {t}: converged {conv.sum()}/{B}, compared {err.size // len(KS)}/{idx.size}, err max {err.max():.3e} "
                  f"median {np.median(err):.3e}, gap max {gaps.max():.3e}")
            assert err.size >= 0.5 * idx.size * len(KS), (t, err.size, idx.size)
            hi = mg >= 1e-4
            assert (err[hi] <= np.maximum(CAP, gaps[hi])).all(), (t, err[hi].max())
            assert np.median(err[hi]) <= MEDIAN_CAP, (t, np.median(err[hi]))
            assert (err[~hi] <= np.maximum(CAP, 1e3 * gaps[~hi])).all(), (t, err[~hi], gaps[~hi])
        x = mpc.plant_step(x, u, 50)
    mpc.close()


# ---- 2. identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [29, 70])
def test_gains_are_the_words_the_forward_pass_propagates(pkg, tables, gpu_lib, B):
    mpc, _ = _solved(pkg, tables, B, ticks=1)
    P, S = mpc.policy(), mpc.sensitivities(trajectory=True)
    assert np.array_equal(P["K"][:, 0], S["du0_dx0"]) and np.array_equal(P["Kv"][:, 0], S["du0_duprev"]) and np.array_equal(P["ok"], S["ok"])
    assert P["ok"].sum() >= 0.6 * B
    assert (P["K"][~P["ok"]] == 0).all() and (P["Kv"][~P["ok"]] == 0).all()
    assert np.isfinite(P["K"]).all() and np.isfinite(P["Kv"]).all()
    dX, dU = S["dX"], S["dU"]
    dV = np.zeros_like(dU)  # dV_0 = [0 | I], dV_k = dU_{k-1}
    dV[:, 0, 0, 8] = dV[:, 0, 1, 9] = 1.0
    dV[~P["ok"], 0] = 0.0
    dV[:, 1:] = dU[:, :-1]
    rec = np.einsum("bkij,bkjc->bkic", P["K"], dX[:, :-1]) + np.einsum("bkij,bkjc->bkic", P["Kv"], dV)
    bound = 64 * EPSM * (np.einsum("bkij,bkjc->bkic", np.abs(P["K"]), np.abs(dX[:, :-1])) + np.einsum("bkij,bkjc->bkic", np.abs(P["Kv"]), np.abs(dV)))
    assert (np.abs(dU - rec) <= bound).all(), (np.abs(dU - rec) - bound).max()
    # the device form writes the same words
    import torch
    Kd, Kvd = torch.full((B, N, 2, 8), np.nan, dtype=torch.float64, device="cuda"), torch.full((B, N, 2, 2), np.nan, dtype=torch.float64, device="cuda")
    okd = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _sync()
    mpc.policy_dev(Kd.data_ptr(), Kvd.data_ptr(), okd.data_ptr())
    mpc.synchronize()
    assert np.array_equal(Kd.cpu().numpy(), P["K"]) and np.array_equal(Kvd.cpu().numpy(), P["Kv"]) and np.array_equal(okd.cpu().numpy() != 0, P["ok"])
    mpc.close()


# ---- 3. the step --------------------------------------------------------------------------------------------------------------
def test_policy_step_is_the_formula(pkg, solved13):
    mpc, _ = solved13
    B = mpc.B
    P = mpc.policy()
    X, U = mpc.prediction()
    x0, up, u0 = mpc.solved_parameters()
    assert P["ok"].sum() >= 0.6 * B
    rng = np.random.default_rng(5)
    for k in KS:
        Vk = up if k == 0 else U[:, k - 1]
        x, v = X[:, k] + 0.05 * rng.standard_normal((B, 8)), Vk + 0.1 * rng.standard_normal((B, 2))
        u = mpc.policy_step(k, x, v)
        ref, mag = _formula(P, X, U, up, k, x, v)
        assert (np.abs(u - ref) <= 32 * EPSM * mag).all(), (k, (np.abs(u - ref) / mag).max() / EPSM)
        assert (np.abs(u - U[:, k])[P["ok"]].max(axis=1) > 0).all()  # (the feedback terms are there)
        assert np.array_equal(u[~P["ok"]], U[~P["ok"], k])
        assert np.array_equal(mpc.policy_step(k, X[:, k], Vk), U[:, k])
        assert np.array_equal(mpc.policy_step(k, x), mpc.policy_step(k, x, Vk))
        # clip: rows next to the steering bound, rows with a feedback large enough to reach the input bounds
        xc = x.copy()
        xc[::3, 6] = mpc.params.x_ub[6] - 1e-3
        xc[1::3, 7] = mpc.params.x_lb[7] + 1e-3
        xc[2::3, :6] += 3.0 * rng.standard_normal((len(xc[2::3]), 6))
        raw, got = mpc.policy_step(k, xc, v), mpc.policy_step(k, xc, v, clip=True)
        want = _clip(mpc.params, mpc.options.t_step, xc, raw)
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), k
        assert (want != raw).any()
        if k == 0:
            fb = mpc.feedback(x, u_prev=v)
            assert (np.abs(u - fb) <= 32 * EPSM * mag).all(), (np.abs(u - fb) / mag).max() / EPSM
    # the device form: the same bits
    ud = _dev(np.full((B, 2), np.nan))
    xd, vd = _dev(x), _dev(v)
    _sync()
    mpc.policy_step_dev(KS[-1], xd.data_ptr(), vd.data_ptr(), ud.data_ptr())
    mpc.synchronize()
    assert np.array_equal(ud.cpu().numpy(), u)


def _next_step(mpc, x):
    u = mpc.make_step(x)
    it, st = mpc.iterate(), mpc.stats()
    return [u] + [it[k] for k in sorted(it)] + [st[k] for k in sorted(st)]


def test_usage_errors_leave_the_handle_unchanged(pkg, tables, gpu_lib):
    Err = pkg.LtompcError if hasattr(pkg, "LtompcError") else RuntimeError
    B = 13
    a, x = _solved(pkg, tables, B, ticks=1)
    twin, _ = _solved(pkg, tables, B, ticks=1)
    X, U = a.prediction()
    twin.prediction()
    xd, ud = _dev(x), _dev(np.zeros((B, 2)))
    _sync()
    bad_x, bad_v = x.copy(), np.zeros((B, 2))
    bad_x[3, 2], bad_v[5, 1] = np.nan, np.inf
    calls = [(lambda: a.policy_step(-1, x), "k must be"), (lambda: a.policy_step(N, x), "k must be"),
             (lambda: a.policy_step_dev(N, xd.data_ptr(), 0, ud.data_ptr()), "k must be"),
             (lambda: a.policy_run_dev(N, 1, xd.data_ptr()), "k0 must be"), (lambda: a.policy_run_dev(1, 0, xd.data_ptr()), "n must be"),
             (lambda: a.policy_run_dev(1, N, xd.data_ptr()), r"k0 \+ n"), (lambda: a.policy_run_dev(1, 2, xd.data_ptr(), n_sub=0), "n_sub"),
             (lambda: a.policy_step(1, bad_x), "instance 3"), (lambda: a.policy_step(1, x, bad_v), "instance 5")]
    for call, msg in calls:
        with pytest.raises(Err, match=msg):
            call()
    a.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)  # (no refused run touched the states)
    for p, q in zip(_next_step(a, x), _next_step(twin, x)):
        assert np.array_equal(p, q)
    # before any solve, and after an initial guess
    fresh = pkg.BatchedMPC(tables, N, B)
    for m in (fresh, a):
        m.set_initial_guess(x)
        for call in (m.policy, lambda: m.policy_step(0, x), lambda: m.policy_run_dev(0, 1, xd.data_ptr())):
            with pytest.raises(Err, match="no solve to differentiate"):
                call()
    # after a rollout (thread-per-slot handles only): the gains, but no law (V_0 is not kept)
    fresh.close()
    o = pkg.default_options()
    o.latency_mode = 2
    fresh = pkg.BatchedMPC(tables, N, B, options=o)
    fresh.set_initial_guess_dev(xd.data_ptr())
    fresh.rollout_dev(xd.data_ptr(), 1, 4)
    assert fresh.policy()["ok"].sum() >= 0.6 * B
    for call in (lambda: fresh.policy_step(0, x), lambda: fresh.policy_run_dev(0, 1, xd.data_ptr())):
        with pytest.raises(Err, match="after a rollout"):
            call()
    for m in (a, twin, fresh):
        m.close()


# ---- 4. the run ---------------------------------------------------------------------------------------------------------------
def _with_theta(mpc):
    rng = np.random.default_rng(11)
    mpc.set_theta(dict(mass=mpc.params.mass * (1.0 + 0.05 * rng.uniform(-1, 1, mpc.B)), C_m=mpc.params.C_m * (1.0 + 0.05 * rng.uniform(-1, 1, mpc.B))))


def _with_sets(mpc):
    v = mpc.table_values()
    other = v.copy()
    other[0] *= 1.05  # kappa
    mpc.set_table_sets(np.stack([v, other]), np.arange(mpc.B) % 2)


@pytest.mark.parametrize("B", [13, 70])
@pytest.mark.parametrize("kind", ["uniform", "theta", "sets"])
def test_policy_run_is_the_loop_of_step_and_plant_step(pkg, tables, gpu_lib, B, kind):
    import torch
    mpc, x = _solved(pkg, tables, B, ticks=1, prepare=dict(uniform=None, theta=_with_theta, sets=_with_sets)[kind])
    k0, n, n_sub = 1, 3, 4
    rng = np.random.default_rng(3)
    X, U = mpc.prediction()
    x1 = X[:, k0] + 0.05 * rng.standard_normal((B, 8))
    v1 = U[:, k0 - 1] + 0.05 * rng.standard_normal((B, 2))
    for clip, with_v in ((True, True), (False, False)):
        xr, vd = _dev(x1), _dev(v1)
        ul, xl = _dev(np.full((B, n, 2), np.nan)), _dev(np.full((B, n, 8), np.nan))
        xa, xb, ua, va = _dev(x1), _dev(np.zeros((B, 8))), _dev(np.zeros((B, 2))), _dev(v1)
        _sync()
        mpc.policy_run_dev(k0, n, xr.data_ptr(), vd.data_ptr() if with_v else 0, n_sub, clip, ul.data_ptr(), xl.data_ptr())
        mpc.synchronize()
        us, xs = [], []
        for j in range(n):
            mpc.policy_step_dev(k0 + j, xa.data_ptr(), va.data_ptr() if (with_v or j) else 0, ua.data_ptr(), clip)
            mpc.plant_step_dev(xa.data_ptr(), ua.data_ptr(), xb.data_ptr(), n_sub)
            mpc.synchronize()
            us.append(ua.cpu().numpy().copy()), xs.append(xb.cpu().numpy().copy())
            va, ua = ua, torch.zeros_like(ua)
            xa, xb = xb, xa
            _sync()
        assert np.array_equal(ul.cpu().numpy(), np.stack(us, axis=1)), (kind, clip)
        assert np.array_equal(xl.cpu().numpy(), np.stack(xs, axis=1)), (kind, clip)
        assert np.array_equal(xr.cpu().numpy(), xs[-1])
        assert np.isfinite(xs[-1]).all() and (np.abs(us[0] - U[:, k0]).max(axis=1)[mpc.policy()["ok"]] > 0).all()
        if kind == "uniform":  # the host convenience: the same loop on host arrays
            H = mpc.policy_run(k0, n, x1, v1 if with_v else None, n_sub, clip)
            assert np.array_equal(H["u"], np.stack(us, axis=1)) and np.array_equal(H["x"], np.stack(xs, axis=1))
    mpc.close()


# ---- 5. no side effects, packing ----------------------------------------------------------------------------------------------
def _every_policy_call(mpc, x):
    B = mpc.B
    P = mpc.policy()
    xd, ud = _dev(x), _dev(np.zeros((B, 2)))
    Kd = _dev(np.zeros((B, N, 2, 8)))
    ul = _dev(np.zeros((B, 3, 2)))
    _sync()
    mpc.policy_dev(Kd.data_ptr())
    mpc.policy_step_dev(2, xd.data_ptr(), 0, ud.data_ptr(), True)
    mpc.policy_run_dev(1, 3, xd.data_ptr(), ud.data_ptr(), 4, True, ul.data_ptr())
    mpc.policy_last_dev(3, ul.data_ptr(), ud.data_ptr())
    mpc.synchronize()
    assert np.array_equal(ud.cpu().numpy(), ul.cpu().numpy()[:, -1])
    u = mpc.policy_step(1, x)
    mpc.policy_run(0, 2, x, n_sub=4)
    return P, u


def test_policy_calls_do_not_change_the_next_solve(pkg, tables, gpu_lib):
    B = 70
    a, x = _solved(pkg, tables, B, ticks=1)
    twin, _ = _solved(pkg, tables, B, ticks=1)
    _every_policy_call(a, x)
    xn = a.plant_step(x, a.solved_parameters()[2], 50)
    for p, q in zip(_next_step(a, xn), _next_step(twin, xn)):
        assert np.array_equal(p, q)
    a.close(), twin.close()


def test_policy_on_repacked_instances(pkg, tables, gpu_lib):
    """The set-up of test_repacked_instances_match_the_dense_reference (B = 1024, warm ticks: the instances are re-packed during
    the solve): the policy calls before and after the accessors restore the caller's order give the same bits, and leave the next
    solve as the twin's."""
    B = 1024
    x = _x0_batch(pkg, tables, B, seed=85)
    a, twin = pkg.BatchedMPC(tables, N, B), pkg.BatchedMPC(tables, N, B)
    for m in (a, twin):
        xm = x
        m.set_initial_guess(xm)
        for _ in range(3):
            u = m.make_step(xm)
            xm = m.plant_step(xm, u, 50)
        m.make_step(xm)
    P1, u1 = _every_policy_call(a, xm)  # (packed as the solve left them)
    a.iterate()  # (un-packs)
    P2, u2 = _every_policy_call(a, xm)
    for k in P1:
        assert np.array_equal(P1[k], P2[k]), k
    assert np.array_equal(u1, u2)
    S = a.sensitivities()
    assert np.array_equal(P1["K"][:, 0], S["du0_dx0"]) and np.array_equal(P1["ok"], S["ok"]) and P1["ok"].sum() >= 0.6 * B
    X, U = a.prediction()
    ref, mag = _formula(P1, X, U, a.solved_parameters()[1], 1, xm, U[:, 0])
    assert (np.abs(u1 - ref) <= 32 * EPSM * mag).all()
    twin.iterate()
    xn = a.plant_step(xm, a.solved_parameters()[2], 50)
    for p, q in zip(_next_step(a, xn), _next_step(twin, xn)):
        assert np.array_equal(p, q)
    a.close(), twin.close()


# ---- 6. records ---------------------------------------------------------------------------------------------------------------
def test_policy_of_a_record(pkg, tables, gpu_lib):
    B = 13
    mpc, x = _solved(pkg, tables, B, ticks=1)
    rng = np.random.default_rng(9)
    xs, vs = x + 0.05 * rng.standard_normal((B, 8)), 0.1 * rng.standard_normal((B, 2))
    P, u = mpc.policy(), [mpc.policy_step(k, xs, vs, clip=True) for k in (0, 4)]
    run = mpc.policy_run(1, 2, xs, vs, n_sub=4)
    rec = mpc.record()
    xn = mpc.plant_step(x, mpc.solved_parameters()[2], 50)
    mpc.make_step(xn)
    assert not np.array_equal(mpc.policy()["K"], P["K"])
    with mpc.differentiating(rec):
        Q = mpc.policy()
        for k in P:
            assert np.array_equal(P[k], Q[k]), k
        assert all(np.array_equal(a, mpc.policy_step(k, xs, vs, clip=True)) for a, k in zip(u, (0, 4)))
        again = mpc.policy_run(1, 2, xs, vs, n_sub=4)
        assert np.array_equal(run["u"], again["u"]) and np.array_equal(run["x"], again["x"])
    rec.release()
    mpc.close()


# ---- 7. SplitMPC --------------------------------------------------------------------------------------------------------------
def test_split_handle_equals_one_handle(pkg, tables, gpu_lib):
    B, n_sub = 13, 4
    x = _x0_batch(pkg, tables, B, SEED)
    one, sp = pkg.BatchedMPC(tables, N, B), pkg.SplitMPC(tables, N, B, n_parts=3)
    xd, ud = _dev(x), _dev(np.zeros((B, 2)))
    u1, u2 = _dev(np.zeros((B, 2))), _dev(np.zeros((B, 2)))
    _sync()
    for m, uo in ((one, u1), (sp, u2)):
        m.set_initial_guess_dev(xd.data_ptr())
        m.synchronize()
        m.make_step_dev(xd.data_ptr(), uo.data_ptr())
        m.synchronize()
    P, Q = one.policy(), sp.policy()
    for k in P:
        assert np.array_equal(P[k], Q[k]), k
    assert P["ok"].sum() >= 0.6 * B
    rng = np.random.default_rng(4)
    xs, vs = x + 0.05 * rng.standard_normal((B, 8)), 0.1 * rng.standard_normal((B, 2))
    assert np.array_equal(one.policy_step(3, xs, vs, True), sp.policy_step(3, xs, vs, True))
    r1, r2 = one.policy_run(1, 3, xs, vs, n_sub, True), sp.policy_run(1, 3, xs, vs, n_sub, True)
    assert np.array_equal(r1["u"], r2["u"]) and np.array_equal(r1["x"], r2["x"])
    outs = []
    for m in (one, sp):
        xr, vd, uo = _dev(xs), _dev(vs), _dev(np.full((B, 2), np.nan))
        ul, xl, Kd = _dev(np.full((B, 3, 2), np.nan)), _dev(np.full((B, 3, 8), np.nan)), _dev(np.full((B, N, 2, 8), np.nan))
        _sync()
        m.policy_dev(Kd.data_ptr())
        m.policy_step_dev(2, xr.data_ptr(), vd.data_ptr(), uo.data_ptr())
        m.policy_run_dev(1, 3, xr.data_ptr(), vd.data_ptr(), n_sub, True, ul.data_ptr(), xl.data_ptr())
        m.policy_last_dev(3, ul.data_ptr(), vd.data_ptr())
        m.synchronize()
        outs.append([t.cpu().numpy() for t in (Kd, uo, ul, xl, xr, vd)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.array_equal(outs[0][2], r1["u"]) and np.array_equal(outs[0][5], r1["u"][:, -1])
    one.close(), sp.close()


def test_run_ticks_with_solve_every(pkg, tables, gpu_lib):
    """run_ticks(n_ticks=4, solve_every=2) against the same loop written out on one BatchedMPC; solve_every=1 against a call
    without the keyword."""
    B, n_sub = 13, 4
    x = _x0_batch(pkg, tables, B, SEED)

    def split(**kw):
        sp = pkg.SplitMPC(tables, N, B, n_parts=3)
        xa, xb, u = _dev(x), _dev(np.zeros((B, 8))), _dev(np.zeros((B, 2)))
        _sync()
        sp.set_initial_guess_dev(xa.data_ptr())
        sp.run_ticks(xa.data_ptr(), u.data_ptr(), xb.data_ptr(), 4, n_sub, **kw)
        sp.synchronize()
        out = xa.cpu().numpy(), xb.cpu().numpy(), u.cpu().numpy(), sp.stats()["iters"]
        sp.close()
        return out

    base, every1, every2 = split(), split(solve_every=1), split(solve_every=2)
    for a, b in zip(base, every1):
        assert np.array_equal(a, b)
    one = pkg.BatchedMPC(tables, N, B)
    a, b, u = _dev(x), _dev(np.zeros((B, 8))), _dev(np.zeros((B, 2)))
    _sync()
    one.set_initial_guess_dev(a.data_ptr())
    for _ in range(2):
        one.make_step_dev(a.data_ptr(), u.data_ptr())
        one.plant_step_dev(a.data_ptr(), u.data_ptr(), b.data_ptr(), n_sub)
        a, b = b, a
        one.policy_run_dev(1, 1, a.data_ptr(), u.data_ptr(), n_sub, True, u_log_ptr=u.data_ptr())  # (the log of one tick is the (B,2) array itself)
        one.set_u_prev_dev(u.data_ptr())
    one.synchronize()
    xa2, xb2, u2, it2 = every2
    assert np.array_equal(a.cpu().numpy(), xa2) and np.array_equal(b.cpu().numpy(), xb2) and np.array_equal(u.cpu().numpy(), u2)
    assert np.array_equal(one.stats()["iters"], it2)
    assert not np.array_equal(base[2], u2)  # (and it is another loop than solving every tick)
    one.close()
