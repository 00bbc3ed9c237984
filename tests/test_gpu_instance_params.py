"""Per-instance vehicle and cost parameters (ltompc_set_instance_params) on the GPU: rows equal to the handle's
params give the bits of no rows; four interleaved parameter groups in one handle give, group by group, the bits of uniform
handles created with that group's params (solves, plant steps, rollout logs, both kinds of sensitivity); the oracle agrees per
group; exact solves at theta0 +- h e_j in one handle against the tangential predictor; the contract of set / get / None / _dev."""
import ctypes as C

import numpy as np
import pytest

import param_sens_reference as PR

pytestmark = pytest.mark.gpu

# the four groups of the issue: grip x 0.9, grip x 1.1, mass x 1.2, q_n x 2 with r_du x 5
GROUPS = ({"D_f": 0.9, "D_r": 0.9}, {"D_f": 1.1, "D_r": 1.1}, {"mass": 1.2}, {"q_n": 2.0, "r_du[0]": 5.0, "r_du[1]": 5.0})


def _opts(pkg, mode):
    o = pkg.default_options()
    o.latency_mode = mode
    return o


def _row(pkg, scale):
    t = PR.theta_values(pkg.default_params())
    for name, f in scale.items():
        t[PR.NAMES.index(name)] *= f
    return t


def _params(pkg, row):
    p = pkg.default_params()
    for j, v in enumerate(row):
        PR.set_theta(p, j, v)
    return p


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _solve_state(mpc, u0):
    return dict(u0=u0, status=mpc.status.copy(), iters=mpc.iters.copy())


def _full_state(mpc):
    S, P = mpc.sensitivities(trajectory=True), mpc.param_sensitivities(trajectory=True)
    out = {"it_" + k: v for k, v in mpc.iterate().items()}
    X, U = mpc.prediction()
    out.update(X=X, U=U)
    out.update({"s_" + k: v for k, v in S.items()})
    out.update({"p_" + k: v for k, v in P.items() if k != "names"})
    return out


def _repacked(mpc):
    """The last make_step re-packed its instances: a poll with more than 512 instances in the launch and at most 6/8 of them
    unfinished (ltompc_make_step_dev: the condition of k_pack, with the default LTOMPC_PACK_NUM)."""
    return any(n_launch > 512 and 0 < n_active <= (6 * n_launch) // 8 for _, n_active, n_launch in mpc.history())


def _assert_same(a, b, rows=None, label=""):
    for k in a:
        va = a[k] if rows is None else a[k][rows]
        assert _same(va, b[k]), (label, k)


@pytest.mark.parametrize("mode", [1, 2])
def test_rows_equal_to_the_params_give_the_same_bits(pkg, tables, gpu_lib, mode):
    """Cold solve and 3 warm ticks, B = 1024 (re-packed, asserted): u0, statuses, iterations every tick; iterate, prediction
    and both kinds of sensitivity after the cold solve and after the last tick."""
    B, N = 1024, 10
    x0 = pkg.sample_x0(tables, B, seed=5)
    a = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    b = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    b.set_theta(np.tile(b.theta(), (B, 1)))
    assert _same(b.instance_theta(), np.tile(a.theta(), (B, 1)))
    for m in (a, b):
        m.set_initial_guess(x0)
    x = x0
    for tick in range(4):
        ua, ub = a.make_step(x), b.make_step(x)
        if tick == 0:
            assert _repacked(b), b.history()
        _assert_same(_solve_state(a, ua), _solve_state(b, ub), label=f"tick {tick}")
        if tick in (0, 3):
            _assert_same(_full_state(a), _full_state(b), label=f"tick {tick}")
        xa, xb = a.plant_step(x, ua, n_sub=50), b.plant_step(x, ub, n_sub=50)
        assert _same(xa, xb), tick
        x = xa
    a.close(), b.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_interleaved_groups_match_uniform_handles(pkg, tables, gpu_lib, mode):
    """Instance b in group b % 4: every group bit-identical to a uniform handle of that group's params solving the same x0
    (cold and one warm tick), plant steps, both kinds of sensitivity.  B = 1024: the instances are re-packed during the solves
    (asserted from the poll history), so slot b holds instance orig[b] of another group - the rows must follow the instance.
    The sensitivities are requested before anything un-packs the batch (they run at the packed slots)."""
    G, M, N = len(GROUPS), 256, 10
    B = G * M
    x0 = pkg.sample_x0(tables, B, seed=11)
    rows = np.array([_row(pkg, GROUPS[b % G]) for b in range(B)])
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    mpc.set_theta(rows)
    mpc.set_initial_guess(x0)
    uni = [pkg.BatchedMPC(tables, N, M, params=_params(pkg, rows[g]), options=_opts(pkg, mode)) for g in range(G)]
    for g, u in enumerate(uni):
        u.set_initial_guess(x0[g::G])
    x = x0
    for tick in range(2):
        u0 = mpc.make_step(x)
        if tick == 0:
            assert _repacked(mpc), mpc.history()
        st, full = _solve_state(mpc, u0), _full_state(mpc)
        xn = mpc.plant_step(x, u0, n_sub=50)
        for g, u in enumerate(uni):
            ug = u.make_step(x[g::G])
            _assert_same(st, _solve_state(u, ug), rows=slice(g, None, G), label=f"group {g} tick {tick}")
            _assert_same(full, _full_state(u), rows=slice(g, None, G), label=f"group {g} tick {tick}")
            assert _same(xn[g::G], u.plant_step(x[g::G], ug, n_sub=50)), (g, tick)
        x = xn
    mpc.close()
    for u in uni:
        u.close()


def test_interleaved_groups_rollout(pkg, tables, gpu_lib):
    """rollout_dev: the logs of every group bit-identical to a uniform handle's (slot mode; the rollout has no latency mode)."""
    import torch
    G, M, N, T = len(GROUPS), 64, 10, 3
    B = G * M
    x0 = pkg.sample_x0(tables, B, seed=13)
    rows = np.array([_row(pkg, GROUPS[b % G]) for b in range(B)])

    def run(mpc, x):
        xd = torch.tensor(x, dtype=torch.float64, device="cuda")
        ul = torch.zeros((x.shape[0], T, 2), dtype=torch.float64, device="cuda")
        sl = torch.zeros((x.shape[0], T), dtype=torch.int32, device="cuda")
        il = torch.zeros((x.shape[0], T), dtype=torch.int32, device="cuda")
        mpc.set_initial_guess(x)
        mpc.rollout_dev(xd.data_ptr(), T, 50, ul.data_ptr(), sl.data_ptr(), il.data_ptr())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (xd, ul, sl, il)]

    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    mpc.set_theta(rows)
    got = run(mpc, x0)
    mpc.close()
    for g in range(G):
        u = pkg.BatchedMPC(tables, N, M, params=_params(pkg, rows[g]), options=_opts(pkg, 2))
        ref = run(u, x0[g::G])
        u.close()
        for k, (a, b) in enumerate(zip(got, ref)):
            assert _same(a[g::G], b), (g, k)


def test_groups_against_the_oracle(pkg, tables, orc, gpu_lib):
    """8 instances per group against oracle.Oracle(params=p_g), the tolerances of test_gpu_parity's batch test (cold)."""
    G, M, N = len(GROUPS), 8, 20
    B = G * M
    x0 = pkg.sample_x0(tables, B, seed=17)
    rows = np.array([_row(pkg, GROUPS[b % G]) for b in range(B)])
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    mpc.set_theta(rows)
    mpc.set_initial_guess(x0)
    u0 = mpc.make_step(x0)
    for g in range(G):
        p = orc.default_params()
        for j, v in enumerate(rows[g]):
            PR.set_theta(p, j, v)
        ref = orc.Oracle(tables.packed(), params=p).solve(x0[g::G], N, nthreads=8)
        both = (mpc.status[g::G] == 0) & (ref["status"] == 0)
        assert both.mean() >= 0.75, (g, both)
        assert np.abs(u0[g::G] - ref["u0"])[both].max() < 1e-5, g
    mpc.close()


def test_predictor_against_exact_solves_in_one_batch(pkg, tables, gpu_lib):
    """Rows theta0 + h e_j and theta0 + h/2 e_j (j = D_f, mass) solved exactly in ONE handle against feedback(theta=...) of a
    uniform solve, with (B,) arrays: halving h cuts the error about four-fold (the criterion of
    test_predictor_is_second_order_in_grip_and_mass)."""
    M, N = 128, 20
    x0 = pkg.sample_x0(tables, M, seed=23)
    base = pkg.BatchedMPC(tables, N, M, options=_opts(pkg, 2))
    base.set_initial_guess(x0)
    u0 = base.make_step(x0)
    Sp, pb = base.sensitivities(), base.params
    st0 = base.stats()["status_solver"]
    th0 = base.theta()
    for name, d in (("D_f", -0.005), ("mass", 5.0)):
        j = PR.NAMES.index(name)
        rows = np.tile(th0, (2 * M, 1))
        rows[:M, j] += d
        rows[M:, j] += 0.5 * d
        ex = pkg.BatchedMPC(tables, N, 2 * M, options=_opts(pkg, 2))
        ex.set_theta(rows)
        x2 = np.vstack([x0, x0])
        ex.set_initial_guess(x2)
        ue = ex.make_step(x2)
        sts = ex.stats()["status_solver"]
        ex.close()
        u1, uh = ue[:M], ue[M:]
        p1 = base.feedback(x0, theta={name: np.full(M, th0[j] + d)})
        ph = base.feedback(x0, theta={name: np.full(M, th0[j] + 0.5 * d)})
        e1, eh = np.abs(u1 - p1).max(axis=1), np.abs(uh - ph).max(axis=1)
        move = np.abs(u1 - u0).max(axis=1)
        lo, hi = np.array([pb.u_lb[0], pb.u_lb[1]]), np.array([pb.u_ub[0], pb.u_ub[1]])
        act = [(np.abs(v - lo) < 1e-6) | (np.abs(v - hi) < 1e-6) for v in (u0, u1, uh)]
        same = (act[0] == act[1]).all(axis=1) & (act[0] == act[2]).all(axis=1)
        conv = (st0 == 0) & (sts[:M] == 0) & (sts[M:] == 0)
        use = Sp["ok"] & (Sp["margin"] >= 1e-3) & conv & same & (eh > 1e-7) & (e1 > 1e-7)
        ratio = e1[use] / eh[use]
        assert use.sum() >= 8, (name, use.sum())
        assert np.mean((ratio >= 3.0) & (ratio <= 5.0)) >= 0.75, (name, np.sort(ratio))
        assert np.mean(e1[use] / move[use] < 0.05) >= 0.75, (name, e1[use] / move[use])
    base.close()


def test_contract(pkg, tables, gpu_lib):
    """A set takes effect at the next solve and keeps the warm start; the sensitivities and feedback(theta=...) of a solve
    requested only after a later set are those of the solve's rows; None restores the uniform bits; set_theta_dev equals
    set_theta (feedback included); get returns what set gave; usage errors change nothing; SplitMPC.set_theta is one handle's
    rows, bit for bit."""
    import torch
    B, N = 64, 10
    x0 = pkg.sample_x0(tables, B, seed=29)
    r1 = np.array([_row(pkg, GROUPS[b % 4]) for b in range(B)])
    r2 = np.array([_row(pkg, GROUPS[(b + 1) % 4]) for b in range(B)])  # (every instance changes, r_du included)
    fb = {"D_f": np.linspace(0.95, 1.05, B), "mass": 1010.0}
    a = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    t = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))  # twin: solves with r1, never re-set before its requests
    for m in (a, t):
        m.set_theta(r1)
        m.set_initial_guess(x0)
    ua, ut = a.make_step(x0), t.make_step(x0)
    assert _same(ua, ut)
    a.set_theta(r2)  # before ANY sensitivity request of that solve
    assert _same(a.instance_theta(), r2) and _same(t.instance_theta(), r1)
    _assert_same(_full_state(t), _full_state(a), label="requested after a set")
    assert _same(a.feedback(x0, theta=fb), t.feedback(x0, theta=fb))
    # the next solve uses r2, warm-started from the r1 solve: the twin set to r2 now gives the same bits
    t.set_theta(r2)
    x1 = a.plant_step(x0, ua, n_sub=50)
    assert _same(x1, t.plant_step(x0, ut, n_sub=50))
    ua1, ut1 = a.make_step(x1), t.make_step(x1)
    assert _same(ua1, ut1)
    _assert_same(_full_state(t), _full_state(a), label="second solve")
    # from a cold start, rows r1 give other bits than the uniform params; None gives the uniform bits again
    u = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    u.set_initial_guess(x0)
    uu = u.make_step(x0)
    ref = _full_state(u)
    assert not _same(uu, ua)
    a.set_theta(None)
    assert _same(a.instance_theta(), np.tile(a.theta(), (B, 1)))
    a.set_initial_guess(x0)
    assert _same(a.make_step(x0), uu)
    _assert_same(ref, _full_state(a), label="None")
    # set_theta_dev = set_theta, feedback(theta=...) included
    c = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    td = torch.tensor(r1, dtype=torch.float64, device="cuda")
    c.set_theta_dev(td.data_ptr())
    assert _same(c.instance_theta(), r1)
    c.set_initial_guess(x0)
    assert _same(c.make_step(x0), ua)
    v = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))  # (t has moved on: a fresh twin solved with r1 set on the host)
    v.set_theta(r1)
    v.set_initial_guess(x0)
    v.make_step(x0)
    assert _same(c.feedback(x0, theta=fb), v.feedback(x0, theta=fb))
    # usage errors leave the handle unchanged
    for bad, what in ((r1[:-1], "shape"), ({"mass": -1.0}, "mass"), ({"D_f": np.inf}, "finite"), ({"grip": 1.0}, "name"),
                      ({"q_n": np.zeros(B + 1)}, "shape")):
        with pytest.raises(ValueError):
            c.set_theta(bad)
        assert _same(c.instance_theta(), r1), what
    r = r1.copy()
    r[7, 0] = 0.0
    assert gpu_lib.ltompc_set_instance_params(c._h, r.ctypes.data_as(C.POINTER(C.c_double))) < 0
    assert b"row 7, column 0 (mass)" in gpu_lib.ltompc_last_error()
    r[7, 0], r[3, 15] = 1000.0, np.nan
    assert gpu_lib.ltompc_set_instance_params(c._h, r.ctypes.data_as(C.POINTER(C.c_double))) < 0
    assert b"row 3, column 15" in gpu_lib.ltompc_last_error()
    assert _same(c.instance_theta(), r1)
    for field, val in (("ell_penalty", 10.0), ("ptv", 0.5)):
        p = pkg.default_params()
        setattr(p, field, val)
        if field == "ell_penalty":
            p.ell_D_f = p.ell_D_r = 5000.0
        d = pkg.BatchedMPC(tables, N, B, params=p, options=_opts(pkg, 2))
        with pytest.raises(pkg.LtompcError):
            d.set_theta(r1)
        assert _same(d.instance_theta(), np.tile(d.theta(), (B, 1)))
        d.close()
    # SplitMPC: the rows split across its parts, the bits of one handle
    sp = pkg.SplitMPC(tables, N, B, n_parts=2, options=_opts(pkg, 2))
    sp.set_theta(r1)
    assert _same(sp.instance_theta(), r1)
    xd = torch.tensor(x0, dtype=torch.float64, device="cuda")
    ud = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
    sp.set_initial_guess_dev(xd.data_ptr())
    sp.make_step_dev(xd.data_ptr(), ud.data_ptr())
    sp.synchronize()
    assert _same(ud.cpu().numpy(), ua)
    sp.close()
    for m in (a, t, u, c, v):
        m.close()
