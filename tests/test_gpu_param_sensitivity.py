"""Sensitivities w.r.t. the vehicle and cost parameters (ltompc_get_param_sensitivities) on the GPU: against
the dense reference (param_sens_reference.py) at the GPU's own final iterate, every SOLVED / ACCEPTABLE instance and every
stage, both evaluation paths, cold and after closed-loop ticks, re-packed; soft track constraints against oracle central
differences; the contract (ok, zeros, usage errors, caching, SplitMPC, feedback), the second order of the predictor in D_f
and the mass, and the absence of side effects."""
import os

import numpy as np
import pytest

import param_sens_reference as PR
from test_gpu_sensitivity_dense import SOLVED_OR_ACCEPTABLE, _eps, _x0_batch

pytestmark = pytest.mark.gpu

# |G - D| |theta_j| / max(1, |D| |theta_j|) per entry (each column scaled by |theta_j|), on instances with margin >= 1e-4 whose
# float64 LU is accurate to CAP (else to its gap, as for x0 / u_prev), and the median over the instances.  The bounds of the
# x0 / u_prev columns (tests/test_gpu_sensitivity_dense.py).  Measured on MI355X (both paths, cold and two ticks): max 7.5e-15 /
# 2.5e-6 / 5.9e-7 at N = 2 / 10 / 40, 4.1e-7 re-packed; medians 4e-16 .. 6e-16 (N = 2), 5e-15 .. 1e-13 (N = 10), 7e-9 .. 1.7e-8
# (N = 40).
CAP = 1e-5
MEDIAN_CAP = 1e-7


def _log(name, text):
    f = os.environ.get("LTOMPC_TEST_RATES")
    if f:
        with open(f, "a") as fh:
            fh.write(f"{name} {text}\n")


def check_against_reference(pkg, tables, mpc, S, label, params=None, subset=None):
    """Compare S = mpc.param_sensitivities(trajectory=True) of the last make_step with the dense reference at mpc's iterate."""
    params = params or pkg.default_params()
    st, it = mpc.stats(), mpc.iterate()
    x0, up, _ = mpc.solved_parameters()
    B, N = mpc.B, mpc.N
    Sp = mpc.sensitivities()
    ok = S["ok"]
    assert np.array_equal(ok, Sp["ok"]), label  # the same ok as the x0 / u_prev pass, bit for bit
    for k in ("du0_dtheta", "dX", "dU"):
        assert (S[k][~ok] == 0).all(), (label, k)
    assert (S["dX"][:, 0] == 0).all() and np.array_equal(S["dU"][:, 0], S["du0_dtheta"]), label
    conv = np.isin(st["status_solver"], SOLVED_OR_ACCEPTABLE)
    if subset is not None:
        conv &= np.isin(np.arange(B), subset)
    idx = np.flatnonzero(conv & ok)
    assert idx.size >= 0.5 * (B if subset is None else len(subset)), (label, idx.size)
    eps = _eps(mpc, st, conv)
    R = PR.param_sensitivities_batch({k: v[idx] for k, v in it.items()}, x0[idx], up[idx], tables, eps, params)
    th = PR.theta_values(params)
    err, mg, gaps = [], [], []
    for b, r in zip(idx, R):
        e = max(PR.scaled_error(S["dX"][b], r["dX"], th).max(), PR.scaled_error(S["dU"][b], r["dU"], th).max(),
                PR.scaled_error(S["du0_dtheta"][b], r["du0"], th).max())
        err.append(e), mg.append(Sp["margin"][b]), gaps.append(r["gap"])
    err, mg, gaps = np.array(err), np.array(mg), np.array(gaps)
    hi = mg >= 1e-4
    _log(f"psens_dense_{label}", f"conv {conv.sum()}/{B} compared {err.size} (margin >= 1e-4: {hi.sum()}) "
         f"err_pct50/90/100 {np.percentile(err[hi], [50, 90, 100]) if hi.any() else None} "
         f"low-margin err max {err[~hi].max() if (~hi).any() else None} gap max {gaps.max()}")
    assert hi.sum() >= 1, label
    assert (err[hi] <= np.maximum(CAP, gaps[hi])).all(), (label, err[hi].max(), gaps[hi][np.argmax(err[hi])])
    assert np.median(err[hi]) <= MEDIAN_CAP, (label, np.median(err[hi]))
    assert (err[~hi] <= np.maximum(CAP, 1e3 * gaps[~hi])).all(), (label, err[~hi].max())
    return err


def _ticks(pkg, tables, x, N, label, options=None, ticks=3):
    mpc = pkg.BatchedMPC(tables, N, x.shape[0], options=options)
    mpc.set_initial_guess(x)
    for t in range(ticks):
        u = mpc.make_step(x)
        S = mpc.param_sensitivities(trajectory=True)
        assert S["names"] == PR.NAMES and S["du0_dtheta"].shape == (x.shape[0], 2, 16)
        check_against_reference(pkg, tables, mpc, S, f"{label}_t{t}")
        x = mpc.plant_step(x, u, 50)
    mpc.close()


@pytest.mark.parametrize("N,B", [(2, 61), (10, 61), (40, 29)])
@pytest.mark.parametrize("mode", [1, 2])
def test_param_sensitivities_match_the_dense_reference(pkg, tables, gpu_lib, N, B, mode):
    """latency_mode 1 (8 lanes per slot in the solve and the factorisation) and 2 (thread per slot); a cold solve and two
    closed-loop ticks (u_prev != 0).  B not a multiple of 8: padding lanes."""
    o = pkg.default_options()
    o.latency_mode = mode
    _ticks(pkg, tables, _x0_batch(pkg, tables, B, seed=90 + N), N, f"N{N}_mode{mode}", options=o)


def test_repacked_instances_match_the_dense_reference(pkg, tables, gpu_lib):
    """B >= 1024 after warm ticks (instances re-packed): param_sensitivities(), iterate() (un-packs: the factorisation is
    no longer at the instances' slots), then param_sensitivities(True), which factorises again at the new slots."""
    x = _x0_batch(pkg, tables, 1024, seed=95)
    mpc = pkg.BatchedMPC(tables, 10, x.shape[0])
    mpc.set_initial_guess(x)
    for _ in range(3):
        u = mpc.make_step(x)
        x = mpc.plant_step(x, u, 50)
    mpc.make_step(x)
    S1 = mpc.param_sensitivities()
    mpc.iterate()
    S = mpc.param_sensitivities(trajectory=True)
    for k in ("du0_dtheta", "ok"):
        assert np.array_equal(S1[k], S[k]), k
    check_against_reference(pkg, tables, mpc, S, "repacked", subset=np.arange(0, 1024, 23))
    mpc.close()


def _theta_fd(orc, tables, x, N, options, cols, h_rel=1e-6):
    """du0 central differences w.r.t. theta_j (j in cols) at h and 10 h, cold oracle solves; and all solves SOLVED."""
    base = orc.Oracle(tables.packed(), options=options).solve(x, N)
    th = PR.theta_values(orc.default_params())
    solved, out = base["status_solver"] == 0, {}
    for f in (1.0, 10.0):
        D = np.zeros((x.shape[0], 2, PR.NT))
        for j in cols:
            h = f * h_rel * abs(th[j])
            u = []
            for sgn in (1.0, -1.0):
                p = PR.set_theta(orc.default_params(), j, th[j] + sgn * h)
                q = orc.Oracle(tables.packed(), params=p, options=options).solve(x, N)
                solved &= q["status_solver"] == 0
                u.append(q["u0"])
            D[:, :, j] = (u[0] - u[1]) / (2 * h)
        out[f] = D
    return out, base, solved


def test_soft_track_constraints_match_central_differences(pkg, tables, orc, gpu_lib):
    """soft_rho = 100 (elastic track constraints, the barrier weights of the elastic pairs): du0_dtheta against oracle central
    differences on the instances whose solves all ended SOLVED, with margin >= 1e-3 and differences that agree between h and
    10 h, to 1e-4 + mu_min / margin^2 as for x0 / u_prev."""
    o = pkg.default_options()
    o.soft_rho = 100.0
    oo = orc.default_options()
    oo.soft_rho = 100.0
    x = _x0_batch(pkg, tables, 12, seed=97)
    mpc = pkg.BatchedMPC(tables, 10, x.shape[0], options=o)
    mpc.set_initial_guess(x)
    u = mpc.make_step(x)
    S, Sp, st = mpc.param_sensitivities(), mpc.sensitivities(), mpc.stats()
    mpc.close()
    fd, base, solved = _theta_fd(orc, tables, x, 10, oo, range(PR.NT))
    th = PR.theta_values(orc.default_params())
    smooth = np.abs(fd[1.0] - fd[10.0]) * th / np.maximum(1.0, np.abs(fd[1.0]) * th) <= 1e-5
    use = S["ok"] & (Sp["margin"] >= 1e-3) & (st["status_solver"] == 0) & solved & (np.abs(u - base["u0"]).max(axis=1) < 1e-6)
    assert use.sum() >= 3, use
    e = PR.scaled_error(S["du0_dtheta"], fd[1.0], th)
    worst = []
    for b in np.flatnonzero(use):
        tol = 1e-4 + 1e-9 / Sp["margin"][b] ** 2
        assert smooth[b].sum() >= 0.5 * smooth[b].size, (b, smooth[b].sum())
        assert e[b][smooth[b]].max() <= tol, (b, e[b][smooth[b]].max(), tol)
        worst.append(e[b][smooth[b]].max())
    _log("psens_fd_soft", f"used {use.sum()} err {np.round(worst, 10).tolist()}")


def test_predictor_is_second_order_in_grip_and_mass(pkg, tables, gpu_lib):
    """u0(theta + d) - (u0 + du0_dtheta d) = O(d^2): halving d cuts the error about four-fold, on instances whose three
    solves converged with the same inputs at their bounds and margin >= 1e-3.  d = -0.5 % of D_f, +0.5 % of the mass.  As for
    x0 (test_gpu_sensitivity.py) a full step that crosses a kink of a track constraint is not seen by the input-bound filter:
    hence a rate of 0.75, not 1."""
    M, N = 128, 20
    x0 = pkg.sample_x0(tables, M, seed=23)
    for name, d in (("D_f", -0.005), ("mass", 5.0)):
        j = PR.NAMES.index(name)
        us, sts = [], []
        for f in (0.0, 1.0, 0.5):
            p = pkg.default_params()
            PR.set_theta(p, j, PR.theta_values(p)[j] + f * d)
            mpc = pkg.BatchedMPC(tables, N, M, params=p)
            mpc.set_initial_guess(x0)
            us.append(mpc.make_step(x0)), sts.append(mpc.stats()["status_solver"])
            if f == 0.0:
                S, Sp, pb = mpc.param_sensitivities(), mpc.sensitivities(), mpc.params
            mpc.close()
        u0, u1, uh = us
        g = S["du0_dtheta"][:, :, j]
        e1 = np.abs(u1 - (u0 + g * d)).max(axis=1)
        eh = np.abs(uh - (u0 + g * 0.5 * d)).max(axis=1)
        move = np.abs(u1 - u0).max(axis=1)
        lo, hi = np.array([pb.u_lb[0], pb.u_lb[1]]), np.array([pb.u_ub[0], pb.u_ub[1]])
        act = [(np.abs(v - lo) < 1e-6) | (np.abs(v - hi) < 1e-6) for v in us]
        same = (act[0] == act[1]).all(axis=1) & (act[0] == act[2]).all(axis=1)
        conv = (sts[0] == 0) & (sts[1] == 0) & (sts[2] == 0)
        use = S["ok"] & (Sp["margin"] >= 1e-3) & conv & same & (eh > 1e-7) & (e1 > 1e-7)
        ratio = e1[use] / eh[use]
        _log(f"psens_second_order_{name}", f"used {use.sum()} ratio {np.round(np.sort(ratio), 3).tolist()} "
             f"err/move {np.round(np.sort(e1[use] / move[use]), 4).tolist()}")
        assert use.sum() >= 8, (name, use.sum())
        assert np.mean((ratio >= 3.0) & (ratio <= 5.0)) >= 0.75, (name, np.sort(ratio))
        assert np.mean(e1[use] / move[use] < 0.05) >= 0.75, (name, e1[use] / move[use])


def test_contract(pkg, tables, gpu_lib):
    """Usage errors; host / device variants; ok = 0 rows (an instance far off the track) exactly 0 and its neighbours
    unaffected; SplitMPC bit-identical to one handle; feedback(theta=...) the tangential predictor."""
    import torch
    L = gpu_lib
    x = _x0_batch(pkg, tables, 16, seed=99)
    mpc = pkg.BatchedMPC(tables, 10, x.shape[0])
    with pytest.raises(pkg.LtompcError):
        mpc.param_sensitivities()
    assert L.ltompc_param_sensitivities_dev(mpc._h, None, None) != 0
    mpc.set_initial_guess(x)
    y = x.copy()
    y[4, 1] += 40.0
    u = mpc.make_step(y)
    S = mpc.param_sensitivities(trajectory=True)
    sst = mpc.stats()["status_solver"]
    assert sst[4] not in (0, 1) and not S["ok"][4]
    bad = ~S["ok"]
    for k in ("du0_dtheta", "dX", "dU"):
        assert (S[k][bad] == 0).all(), k
    assert S["ok"].mean() >= 0.75
    dev = torch.device("cuda", 0)
    g = torch.full((x.shape[0], 2, 16), np.nan, dtype=torch.float64, device=dev)
    ok = torch.full((x.shape[0],), -1, dtype=torch.int32, device=dev)
    mpc.param_sensitivities_dev(g.data_ptr(), ok.data_ptr())
    mpc.synchronize()
    assert np.array_equal(g.cpu().numpy(), S["du0_dtheta"]) and np.array_equal(ok.cpu().numpy() != 0, S["ok"])
    # feedback: theta=None is the x0 / u_prev predictor unchanged; theta adds du0_dtheta (theta - theta_solved)
    fb = mpc.feedback(y + 1e-3)
    assert np.array_equal(mpc.feedback(y + 1e-3, theta=None), fb)
    want = fb + S["du0_dtheta"][:, :, 4] * (0.95 - 1.0) + S["du0_dtheta"][:, :, 0] * 10.0
    assert np.allclose(mpc.feedback(y + 1e-3, theta={"D_f": 0.95, "mass": 1010.0}), want, rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        mpc.feedback(y, theta={"width": 2.0})
    # neighbours of the far-off instance: the same bits as in a solve without it
    m2 = pkg.BatchedMPC(tables, 10, x.shape[0])
    m2.set_initial_guess(x)
    m2.make_step(x)
    T = m2.param_sensitivities(trajectory=True)
    m2.close()
    others = np.setdiff1d(np.arange(x.shape[0]), [4])
    for k in ("du0_dtheta", "ok", "dX", "dU"):
        assert np.array_equal(S[k][others], T[k][others]), k
    mpc.set_initial_guess(x)
    with pytest.raises(pkg.LtompcError):
        mpc.param_sensitivities()
    mpc.close()
    # handles whose problem theta does not cover
    for field, value in (("ell_penalty", 1e3), ("ptv", 10.0)):
        p = pkg.default_params()
        setattr(p, field, value)
        if field == "ell_penalty":
            p.ell_rho, p.ell_D_f, p.ell_D_r = 1.0, 5000.0, 5000.0
        m3 = pkg.BatchedMPC(tables, 10, 8, params=p)
        m3.set_initial_guess(x[:8])
        m3.make_step(x[:8])
        m3.sensitivities()  # (the x0 / u_prev pass covers them)
        with pytest.raises(pkg.LtompcError, match=field):
            m3.param_sensitivities()
        assert L.ltompc_param_sensitivities_dev(m3._h, None, None) != 0
        m3.close()
    # SplitMPC with 4 parts: the same bits as one handle (SplitMPC with 1 part); host and device entry points
    Y = _x0_batch(pkg, tables, 512, seed=98)
    out = []
    for parts in (1, 4):
        sp = pkg.SplitMPC(tables, 10, Y.shape[0], n_parts=parts)
        xa = torch.from_numpy(Y).to(dev)
        ua = torch.zeros(Y.shape[0], 2, dtype=torch.float64, device=dev)
        sp.set_initial_guess_dev(xa.data_ptr())
        sp.make_step_dev(xa.data_ptr(), ua.data_ptr())
        sp.synchronize()
        T = sp.param_sensitivities(trajectory=True)
        assert T["names"] == PR.NAMES
        gs = torch.zeros((Y.shape[0], 2, 16), dtype=torch.float64, device=dev)
        oks = torch.zeros((Y.shape[0],), dtype=torch.int32, device=dev)
        sp.param_sensitivities_dev(gs.data_ptr(), oks.data_ptr())
        sp.synchronize()
        assert np.array_equal(gs.cpu().numpy(), T["du0_dtheta"]) and np.array_equal(oks.cpu().numpy() != 0, T["ok"])
        out.append((ua.cpu().numpy(), T))
        sp.close()
    assert np.array_equal(out[0][0], out[1][0])
    for k in ("du0_dtheta", "ok", "dX", "dU"):
        assert np.array_equal(out[0][1][k], out[1][1][k]), k


def _record(mpc, u, x):
    X, U = mpc.prediction()
    it = mpc.iterate()
    return [u, mpc.status.copy(), mpc.iters.copy(), X, U] + [it[k] for k in sorted(it)]


def test_no_side_effects(pkg, tables, gpu_lib):
    """A handle that asks for the parameter sensitivities after every tick (both orders against the x0 / u_prev pass) gives the
    bits of a twin that never does: u0, statuses, iterations, predictions, the whole iterate and get_sensitivities' outputs,
    over closed-loop ticks and after a rollout (where the request is a usage error)."""
    import torch
    x = _x0_batch(pkg, tables, 600, seed=43)
    a, b = pkg.BatchedMPC(tables, 10, x.shape[0]), pkg.BatchedMPC(tables, 10, x.shape[0])
    dev = torch.device("cuda", 0)
    g = torch.zeros(x.shape[0], 2, 16, dtype=torch.float64, device=dev)
    ok = torch.zeros(x.shape[0], dtype=torch.int32, device=dev)
    xa, xb = x.copy(), x.copy()
    a.set_initial_guess(xa), b.set_initial_guess(xb)
    for tick in range(6):
        ua, ub = a.make_step(xa), b.make_step(xb)
        if tick % 2:  # the parameter pass first (it runs the factorisation and the x0 / u_prev forward pass) ...
            b.param_sensitivities(trajectory=True)
            b.param_sensitivities_dev(g.data_ptr(), ok.data_ptr())
            Sb = b.sensitivities(trajectory=True)
        else:  # ... or second (it reuses them)
            Sb = b.sensitivities(trajectory=True)
            b.param_sensitivities_dev(g.data_ptr(), ok.data_ptr())
            b.param_sensitivities(trajectory=True)
        b.synchronize()
        Sa = a.sensitivities(trajectory=True)
        for k in Sa:
            assert np.array_equal(Sa[k], Sb[k]), (tick, k)
        ra, rb = _record(a, ua, xa), _record(b, ub, xb)
        for i, (p, q) in enumerate(zip(ra, rb)):
            assert np.array_equal(p, q), (tick, i)
        xa, xb = a.plant_step(xa, ua, 50), b.plant_step(xb, ub, 50)
    a.close(), b.close()
    x = _x0_batch(pkg, tables, 128, seed=44)
    a, b = pkg.BatchedMPC(tables, 10, x.shape[0]), pkg.BatchedMPC(tables, 10, x.shape[0])
    ta, tb = torch.from_numpy(x).to(dev), torch.from_numpy(x).to(dev)
    for m, t in ((a, ta), (b, tb)):
        m.set_initial_guess(x)
        m.rollout_dev(t.data_ptr(), 2, 50)
    # a rollout does not keep the u_prev of each instance's last solve (the r_du columns need it): a usage error, no side effect
    with pytest.raises(pkg.LtompcError, match="rollout"):
        b.param_sensitivities(trajectory=True)
    Sa, Sb = a.sensitivities(trajectory=True), b.sensitivities(trajectory=True)
    assert Sb["ok"].mean() > 0.5
    for k in Sa:
        assert np.array_equal(Sa[k], Sb[k]), k
    xs = ta.cpu().numpy()
    assert np.array_equal(xs, tb.cpu().numpy())
    ua, ub = a.make_step(xs), b.make_step(xs)
    for i, (p, q) in enumerate(zip(_record(a, ua, xs), _record(b, ub, xs))):
        assert np.array_equal(p, q), i
    a.close(), b.close()
