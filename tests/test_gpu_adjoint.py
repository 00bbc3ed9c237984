"""Adjoint sensitivities (ltompc_get_adjoint) on the GPU: against the contraction of the handle's own forward
Jacobians (every instance), against the dense reference through one-hot cotangents (independent of the forward kernels),
re-packed, with per-instance rows, the contract of the three entry points (host / device forms, prediction_dev, SplitMPC,
usage errors), and the absence of side effects."""
import os

import numpy as np
import pytest

import param_sens_reference as PR
from test_gpu_param_sensitivity import CAP, MEDIAN_CAP
from test_gpu_sensitivity_dense import SOLVED_OR_ACCEPTABLE, _eps, _x0_batch

pytestmark = pytest.mark.gpu

# Test 1's measure, per instance and column j: |adj_j - fwd_j| / sum_e |g_e| |D_e,j| (denominator 1 where it is 0), adj the
# adjoint pass and fwd the float64 contraction of sensitivities(trajectory=True) / param_sensitivities(trajectory=True) of the
# same solve with the same cotangent.  Both run on one factorisation: rounding, amplified by the conditioning of the horizon.
# Measured on MI355X over every instance (profiles/adj/README.md; both modes, a cold solve and two closed-loop ticks), max and
# the range of the medians:
#   N = 2  (B = 61)  max 2.9e-15   medians 3.1e-16 .. 4.4e-16
#   N = 10 (B = 61)  max 1.20e-8   medians 3.6e-16 .. 4.8e-16
#   N = 40 (B = 13)  max 2.6e-9    medians 2.9e-11 .. 1.1e-10
#   N = 80 (B = 29)  max 1.21e-8   medians 7.4e-11 .. 1.4e-10
#   re-packed (B = 1024, N = 10, every 23rd instance)  max 1.2e-9, median 7.7e-16
#   grad_p after a rollout (B = 128, N = 10)           max 2.6e-13, median 2.5e-16
# The bound is 10 x the largest of these (run-to-run variation of the chosen instances), 80 times tighter than CAP.
FWD_BOUND = 1.21e-7
assert FWD_BOUND <= CAP


def _log(name, text):
    f = os.environ.get("LTOMPC_TEST_RATES")
    if f:
        with open(f, "a") as fh:
            fh.write(f"{name} {text}\n")


def _opts(pkg, mode):
    o = pkg.default_options()
    o.latency_mode = mode
    return o


def _cotangent(B, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))


def _contract(S, P, gX, gU):
    """float64 contraction of the forward Jacobians with the cotangent: grad_p (B,10), grad_theta (B,16), and the measure's
    denominators sum_e |g_e| |D_e,j|."""
    gp = np.einsum("bki,bkij->bj", gX, S["dX"]) + np.einsum("bkc,bkcj->bj", gU, S["dU"])
    gt = np.einsum("bki,bkij->bj", gX, P["dX"]) + np.einsum("bkc,bkcj->bj", gU, P["dU"])
    dp = np.einsum("bki,bkij->bj", np.abs(gX), np.abs(S["dX"])) + np.einsum("bkc,bkcj->bj", np.abs(gU), np.abs(S["dU"]))
    dt = np.einsum("bki,bkij->bj", np.abs(gX), np.abs(P["dX"])) + np.einsum("bkc,bkcj->bj", np.abs(gU), np.abs(P["dU"]))
    return gp, gt, dp, dt


def check_against_forward(mpc, A, gX, gU, label, S=None, P=None, rows=None):
    """Test 1 on the last solve of mpc: A = mpc.adjoint(gX, gU) against the handle's own forward mode, every instance (or
    `rows`).  Returns the per-instance errors."""
    S = S or mpc.sensitivities(trajectory=True)
    P = P or mpc.param_sensitivities(trajectory=True)
    ok = S["ok"]
    assert np.array_equal(A["ok"], ok) and np.array_equal(P["ok"], ok), label  # bit for bit the forward passes' ok
    for k in ("grad_x0", "grad_uprev", "grad_theta"):
        assert (A[k][~ok] == 0).all(), (label, k)
    gp, gt, dp, dt = _contract(S, P, gX, gU)
    got = np.concatenate([A["grad_x0"], A["grad_uprev"], A["grad_theta"]], axis=1)
    want, den = np.concatenate([gp, gt], axis=1), np.concatenate([dp, dt], axis=1)
    err = np.abs(got - want) / np.where(den > 0, den, 1.0)
    if rows is not None:
        err = err[rows]
    e = err.max(axis=1)
    _log(f"adj_fwd_{label}", f"instances {e.size} ok {int(ok.sum())} err max {e.max():.3e} median {np.median(e):.3e} "
         f"worst column {int(np.argmax(err.max(axis=0)))}")
    assert np.isfinite(got).all(), label
    assert e.max() <= FWD_BOUND, (label, e.max(), int(np.argmax(e)))
    return e


def _one_hot(B, N, where):
    """Cotangents with one entry 1 per instance: where[b] = ("x", k, i) or ("u", k, c)."""
    gX, gU = np.zeros((B, N + 1, 8)), np.zeros((B, N, 2))
    for b, (kind, k, i) in enumerate(where):
        (gX if kind == "x" else gU)[b, k, i] = 1.0
    return gX, gU


def _places(B, N, seed):
    """Three one-hot placements per instance: a forced one (node N, node 1, u_0, u_{N-1} in turn), u_0 for every instance, and
    a seeded (k, i) anywhere on the horizon."""
    rng = np.random.default_rng(seed)
    forced, u0, rand = [], [], []
    for b in range(B):
        forced.append((("x", N, int(rng.integers(8))), ("x", 1, int(rng.integers(8))), ("u", 0, int(rng.integers(2))),
                       ("u", N - 1, int(rng.integers(2))))[b % 4])
        u0.append(("u", 0, b % 2))
        if rng.integers(5) == 0:
            rand.append(("u", int(rng.integers(N)), int(rng.integers(2))))
        else:
            rand.append(("x", int(rng.integers(1, N + 1)), int(rng.integers(8))))
    return forced, u0, rand


def check_against_dense(pkg, tables, mpc, label, seed, params=None):
    """Test 2 on the last make_step of mpc: one-hot cotangents return rows of the Jacobians; compared with the dense reference
    at the GPU's iterate with test_gpu_param_sensitivity.check_against_reference's measure and bounds."""
    params = params or pkg.default_params()
    st, it = mpc.stats(), mpc.iterate()
    x0, up, _ = mpc.solved_parameters()
    B, N = mpc.B, mpc.N
    Sp = mpc.sensitivities()
    ok = Sp["ok"]
    conv = np.isin(st["status_solver"], SOLVED_OR_ACCEPTABLE)
    idx = np.flatnonzero(conv & ok)
    assert idx.size >= 0.5 * B, (label, idx.size)
    eps = _eps(mpc, st, conv)
    R = PR.param_sensitivities_batch({k: v[idx] for k, v in it.items()}, x0[idx], up[idx], tables, eps, params)
    th = PR.theta_values(params)
    one = np.ones(10)
    errs = []
    for name, where in zip(("forced", "u0", "random"), _places(B, N, seed)):
        gX, gU = _one_hot(B, N, where)
        A = mpc.adjoint(gX, gU)
        assert np.array_equal(A["ok"], ok), (label, name)
        gp = np.concatenate([A["grad_x0"], A["grad_uprev"]], axis=1)
        if name == "u0":  # the u_0 rows are du0_dx0, du0_duprev, du0_dtheta
            Pd = mpc.param_sensitivities()
            for b in idx:
                c = where[b][2]
                want = np.concatenate([Sp["du0_dx0"][b, c], Sp["du0_duprev"][b, c]])
                assert PR.scaled_error(gp[b], want, one).max() <= CAP, (label, b)
                assert PR.scaled_error(A["grad_theta"][b], Pd["du0_dtheta"][b, c], th).max() <= CAP, (label, b)
        ep, et, mg, gaps_p, gaps_t = [], [], [], [], []
        for b, r in zip(idx, R):
            kind, k, i = where[b]
            Dp, Dt = (r["dX_p"][k, i], r["dX"][k, i]) if kind == "x" else (r["dU_p"][k, i], r["dU"][k, i])
            ep.append(PR.scaled_error(gp[b], Dp, one).max()), et.append(PR.scaled_error(A["grad_theta"][b], Dt, th).max())
            mg.append(Sp["margin"][b]), gaps_p.append(r["base"]["gap"]), gaps_t.append(r["gap"])
        ep, et, mg, gaps_p, gaps_t = (np.array(v) for v in (ep, et, mg, gaps_p, gaps_t))
        e, hi = np.maximum(ep, et), mg >= 1e-4
        _log(f"adj_dense_{label}_{name}", f"compared {e.size} (margin >= 1e-4: {hi.sum()}) err_pct50/90/100 "
             f"{np.percentile(e[hi], [50, 90, 100]) if hi.any() else None} low-margin max {e[~hi].max() if (~hi).any() else None} "
             f"gap max {max(gaps_p.max(), gaps_t.max())}")
        assert hi.sum() >= 1, label
        assert (ep[hi] <= np.maximum(CAP, gaps_p[hi])).all(), (label, name, ep[hi].max())
        assert (et[hi] <= np.maximum(CAP, gaps_t[hi])).all(), (label, name, et[hi].max())
        assert np.median(e[hi]) <= MEDIAN_CAP, (label, name, np.median(e[hi]))
        assert (ep[~hi] <= np.maximum(CAP, 1e3 * gaps_p[~hi])).all(), (label, name)
        assert (et[~hi] <= np.maximum(CAP, 1e3 * gaps_t[~hi])).all(), (label, name)
        errs.append(e)
    return errs


def _ticks(pkg, tables, x, N, label, mode, dense, ticks=3):
    B = x.shape[0]
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    mpc.set_initial_guess(x)
    for t in range(ticks):
        u = mpc.make_step(x)
        if t > 0:
            assert np.abs(mpc.solved_parameters()[1]).max() > 0  # u_prev != 0
        gX, gU = _cotangent(B, N, seed=1000 * N + 10 * t + mode)
        A = mpc.adjoint(gX, gU)
        assert A["names"] == PR.NAMES and A["grad_x0"].shape == (B, 8) and A["grad_uprev"].shape == (B, 2) and A["grad_theta"].shape == (B, 16)
        check_against_forward(mpc, A, gX, gU, f"{label}_t{t}")
        # block 0 alone comes back in grad_x0 (times ok), everything else is 0
        g0 = np.zeros_like(gX)
        g0[:, 0] = gX[:, 0]
        A0 = mpc.adjoint(g0, None)
        assert np.array_equal(A0["grad_x0"], gX[:, 0] * A0["ok"][:, None]), label
        assert (A0["grad_uprev"] == 0).all() and (A0["grad_theta"] == 0).all(), label
        if dense:
            check_against_dense(pkg, tables, mpc, f"{label}_t{t}", seed=7 * N + t)
        x = mpc.plant_step(x, u, 50)
    mpc.close()


@pytest.mark.parametrize("N,B", [(2, 61), (10, 61), (40, 13)])
@pytest.mark.parametrize("mode", [1, 2])
def test_adjoint_matches_forward_mode_and_the_dense_reference(pkg, tables, gpu_lib, N, B, mode):
    """Tests 1 and 2 on the same solves: a cold solve and two closed-loop ticks, both latency modes, B not a multiple of 8
    (padding lanes); N = 2: terminal and first stage only."""
    _ticks(pkg, tables, _x0_batch(pkg, tables, B, seed=90 + N), N, f"N{N}_mode{mode}", mode, dense=True)


@pytest.mark.parametrize("mode", [1, 2])
def test_adjoint_matches_forward_mode_beyond_the_documented_horizon(pkg, tables, gpu_lib, mode):
    """N = 80: the per-stage storage of the sweep (test 1 only)."""
    _ticks(pkg, tables, _x0_batch(pkg, tables, 29, seed=170), 80, f"N80_mode{mode}", mode, dense=False)


def _warm(pkg, tables, B, N, seed, ticks=3, **kw):
    x = _x0_batch(pkg, tables, B, seed=seed)
    mpc = pkg.BatchedMPC(tables, N, B, **kw)
    mpc.set_initial_guess(x)
    for _ in range(ticks):
        u = mpc.make_step(x)
        x = mpc.plant_step(x, u, 50)
    mpc.make_step(x)
    return mpc, x


def _repacked(mpc):
    return any(n_launch > 512 and 0 < n_active <= (6 * n_launch) // 8 for _, n_active, n_launch in mpc.history())


def _same(A, B_, rows=None):
    for k in ("grad_x0", "grad_uprev", "grad_theta", "ok"):
        if k in A or k in B_:
            a = A[k] if rows is None else A[k][rows]
            assert np.array_equal(a, B_[k]), k


def test_repacked_instances(pkg, tables, gpu_lib):
    """B = 1024 after warm ticks (instances re-packed): adjoint(), iterate() (un-packs: factorisation and right-hand sides are
    no longer at the instances' slots), adjoint() again: the same bits, and test 1."""
    mpc, _ = _warm(pkg, tables, 1024, 10, seed=95)
    gX, gU = _cotangent(1024, 10, seed=3)
    A1 = mpc.adjoint(gX, gU)
    mpc.iterate()
    A2 = mpc.adjoint(gX, gU)
    _same(A1, A2)
    check_against_forward(mpc, A2, gX, gU, "repacked", rows=np.arange(0, 1024, 23))
    mpc.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_per_instance_rows(pkg, tables, gpu_lib, mode):
    """Four interleaved theta groups (B = 1024: re-packed, asserted): each group's gradients are the bits of a uniform handle
    created with that group's params; rows set after the solve do not change them."""
    from test_gpu_instance_params import GROUPS, _params, _row
    G, M, N = len(GROUPS), 256, 10
    B = G * M
    x0 = pkg.sample_x0(tables, B, seed=11)
    rows = np.array([_row(pkg, GROUPS[b % G]) for b in range(B)])
    gX, gU = _cotangent(B, N, seed=4)
    mpc = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    mpc.set_theta(rows)
    mpc.set_initial_guess(x0)
    mpc.make_step(x0)
    assert _repacked(mpc), mpc.history()
    A = mpc.adjoint(gX, gU)
    Ap = mpc.adjoint(gX, gU, theta=False)
    assert "grad_theta" not in Ap
    _same(Ap, {k: A[k] for k in ("grad_x0", "grad_uprev", "ok")})
    assert A["ok"].mean() > 0.5
    for g in range(G):
        u = pkg.BatchedMPC(tables, N, M, params=_params(pkg, rows[g]), options=_opts(pkg, mode))
        u.set_initial_guess(x0[g::G])
        u.make_step(x0[g::G])
        _same(A, u.adjoint(gX[g::G], gU[g::G]), rows=slice(g, None, G))
        u.close()
    mpc.set_theta(np.roll(rows, 1, axis=0))  # R2 after the solve with R1: the gradients stay those of R1
    _same(A, mpc.adjoint(gX, gU))
    mpc.close()


def test_contract(pkg, tables, gpu_lib):
    """Device forms equal the host forms bit for bit; prediction_dev equals prediction() and leaves the packed order alone;
    SplitMPC equals one handle; the usage errors; grad_p after a rollout."""
    import torch
    L = gpu_lib
    dev = torch.device("cuda", 0)
    B, N = 1024, 10
    x = _x0_batch(pkg, tables, B, seed=96)
    mpc, twin, ref = (pkg.BatchedMPC(tables, N, B) for _ in range(3))
    gX, gU = _cotangent(B, N, seed=5)
    # usage errors before a solve
    with pytest.raises(pkg.LtompcError, match="no solve"):
        mpc.adjoint(gX, gU)
    assert L.ltompc_adjoint_dev(mpc._h, None, None, None, None, None) != 0
    for m in (mpc, twin, ref):
        m.set_initial_guess(x)
    for _ in range(2):
        u, ut, ur = mpc.make_step(x), twin.make_step(x), ref.make_step(x)
        x = mpc.plant_step(x, u, 50)
    assert _repacked(mpc), mpc.history()
    # prediction_dev on the packed instances, then the host form (which un-packs), then prediction_dev again
    Xd = torch.full((B, N + 1, 8), np.nan, dtype=torch.float64, device=dev)
    Ud = torch.full((B, N, 2), np.nan, dtype=torch.float64, device=dev)
    mpc.prediction_dev(Xd.data_ptr(), Ud.data_ptr())
    mpc.synchronize()
    Xr, Ur = ref.prediction()
    assert np.array_equal(Xd.cpu().numpy(), Xr) and np.array_equal(Ud.cpu().numpy(), Ur)
    ref.close()
    # ... it left the packed order alone: the next tick runs as the twin's, which never asked
    u, ut = mpc.make_step(x), twin.make_step(x)
    assert np.array_equal(u, ut) and np.array_equal(mpc.history(), twin.history())
    assert mpc.timing()["launches"] == twin.timing()["launches"]
    Xt, Ut = twin.prediction()
    mpc.prediction_dev(Xd.data_ptr(), Ud.data_ptr())
    mpc.synchronize()
    assert np.array_equal(Xd.cpu().numpy(), Xt) and np.array_equal(Ud.cpu().numpy(), Ut)
    Xh, Uh = mpc.prediction()  # (un-packs)
    assert np.array_equal(Xh, Xt) and np.array_equal(Uh, Ut)
    mpc.prediction_dev(Xd.data_ptr(), 0)
    mpc.synchronize()
    assert np.array_equal(Xd.cpu().numpy(), Xt)
    twin.close()
    # host and device forms of the adjoint
    A = mpc.adjoint(gX, gU)
    gXd, gUd = torch.from_numpy(gX).to(dev), torch.from_numpy(gU).to(dev)
    gp = torch.full((B, 10), np.nan, dtype=torch.float64, device=dev)
    gt = torch.full((B, 16), np.nan, dtype=torch.float64, device=dev)
    ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    mpc.adjoint_dev(gXd.data_ptr(), gUd.data_ptr(), gp.data_ptr(), gt.data_ptr(), ok.data_ptr())
    mpc.synchronize()
    assert np.array_equal(gp.cpu().numpy(), np.concatenate([A["grad_x0"], A["grad_uprev"]], axis=1))
    assert np.array_equal(gt.cpu().numpy(), A["grad_theta"]) and np.array_equal(ok.cpu().numpy() != 0, A["ok"])
    # one of the cotangents absent = zeros
    Ax, Az = mpc.adjoint(gX, None), mpc.adjoint(gX, np.zeros_like(gU))
    _same(Ax, Az)
    Au, Az = mpc.adjoint(None, gU), mpc.adjoint(np.zeros_like(gX), gU)
    _same(Au, Az)
    gp.fill_(np.nan)
    mpc.adjoint_dev(0, gUd.data_ptr(), gp.data_ptr())
    mpc.synchronize()
    assert np.array_equal(gp.cpu().numpy(), np.concatenate([Au["grad_x0"], Au["grad_uprev"]], axis=1))
    # usage errors: no cotangent, a non-finite cotangent (names the instance), after an initial guess
    with pytest.raises(pkg.LtompcError, match="both NULL"):
        mpc.adjoint(None, None)
    assert L.ltompc_adjoint_dev(mpc._h, None, None, None, None, None) != 0
    bad = gU.copy()
    bad[37, 3, 1] = np.inf
    with pytest.raises(pkg.LtompcError, match="instance 37"):
        mpc.adjoint(gX, bad)
    _same(A, mpc.adjoint(gX, gU))  # (no trace of the refused calls)
    mpc.set_initial_guess(x)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        mpc.adjoint(gX, gU)
    mpc.close()
    # handles whose problem theta does not cover: grad_theta refused with the forward pass's wording, grad_p works
    for field, value in (("ell_penalty", 1e3), ("ptv", 10.0)):
        p = pkg.default_params()
        setattr(p, field, value)
        if field == "ell_penalty":
            p.ell_rho, p.ell_D_f, p.ell_D_r = 1.0, 5000.0, 5000.0
        m3 = pkg.BatchedMPC(tables, N, 8, params=p)
        m3.set_initial_guess(x[:8])
        m3.make_step(x[:8])
        with pytest.raises(pkg.LtompcError, match=field):
            m3.adjoint(gX[:8], gU[:8])
        A3, S3 = m3.adjoint(gX[:8], gU[:8], theta=False), m3.sensitivities(trajectory=True)
        assert np.array_equal(A3["ok"], S3["ok"])
        m3.close()
    # after a rollout: grad_p works (test 1's measure on the (x0, u_prev) columns), grad_theta is refused
    M = 128
    m4 = pkg.BatchedMPC(tables, N, M)
    xs = torch.from_numpy(_x0_batch(pkg, tables, M, seed=44)).to(dev)
    m4.set_initial_guess_dev(xs.data_ptr())
    m4.rollout_dev(xs.data_ptr(), 2, 50)
    with pytest.raises(pkg.LtompcError, match="rollout"):
        m4.adjoint(gX[:M], gU[:M])
    A4, S4 = m4.adjoint(gX[:M], gU[:M], theta=False), m4.sensitivities(trajectory=True)
    assert np.array_equal(A4["ok"], S4["ok"]) and A4["ok"].mean() > 0.5
    want = np.einsum("bki,bkij->bj", gX[:M], S4["dX"]) + np.einsum("bkc,bkcj->bj", gU[:M], S4["dU"])
    den = np.einsum("bki,bkij->bj", np.abs(gX[:M]), np.abs(S4["dX"])) + np.einsum("bkc,bkcj->bj", np.abs(gU[:M]), np.abs(S4["dU"]))
    err = (np.abs(np.concatenate([A4["grad_x0"], A4["grad_uprev"]], axis=1) - want) / np.where(den > 0, den, 1.0)).max(axis=1)
    _log("adj_fwd_rollout_grad_p", f"instances {err.size} ok {int(A4['ok'].sum())} err max {err.max():.3e} median {np.median(err):.3e}")
    assert err.max() <= FWD_BOUND, err.max()
    m4.close()
    # SplitMPC with 4 parts: the same bits as one handle (SplitMPC with 1 part); host and device entry points
    Y = _x0_batch(pkg, tables, 512, seed=98)
    hX, hU = gX[:512], gU[:512]
    out = []
    for parts in (1, 4):
        sp = pkg.SplitMPC(tables, N, Y.shape[0], n_parts=parts)
        xa = torch.from_numpy(Y).to(dev)
        ua = torch.zeros(Y.shape[0], 2, dtype=torch.float64, device=dev)
        sp.set_initial_guess_dev(xa.data_ptr())
        sp.make_step_dev(xa.data_ptr(), ua.data_ptr())
        sp.synchronize()
        T = sp.adjoint(hX, hU)
        a, b_ = torch.from_numpy(np.ascontiguousarray(hX)).to(dev), torch.from_numpy(np.ascontiguousarray(hU)).to(dev)
        gp = torch.zeros((512, 10), dtype=torch.float64, device=dev)
        gt = torch.zeros((512, 16), dtype=torch.float64, device=dev)
        oks = torch.zeros((512,), dtype=torch.int32, device=dev)
        Xs = torch.zeros((512, N + 1, 8), dtype=torch.float64, device=dev)
        Us = torch.zeros((512, N, 2), dtype=torch.float64, device=dev)
        sp.adjoint_dev(a.data_ptr(), b_.data_ptr(), gp.data_ptr(), gt.data_ptr(), oks.data_ptr())
        sp.prediction_dev(Xs.data_ptr(), Us.data_ptr())
        sp.synchronize()
        assert np.array_equal(gp.cpu().numpy(), np.concatenate([T["grad_x0"], T["grad_uprev"]], axis=1))
        assert np.array_equal(gt.cpu().numpy(), T["grad_theta"]) and np.array_equal(oks.cpu().numpy() != 0, T["ok"])
        it = sp.iterate()
        assert np.array_equal(Xs.cpu().numpy(), it["X"]) and np.array_equal(Us.cpu().numpy(), it["U"])
        out.append(T)
        sp.close()
    _same(out[0], out[1])


def _record(mpc, u):
    X, U = mpc.prediction()
    it = mpc.iterate()
    return [u, mpc.status.copy(), mpc.iters.copy(), X, U] + [it[k] for k in sorted(it)]


def test_no_side_effects(pkg, tables, gpu_lib):
    """A handle that asks for the adjoint after every tick (before or after the forward passes, host and device forms, with
    prediction_dev) gives the bits of a twin that never does: u0, statuses, iterations, prediction, the whole iterate and both
    forward sensitivities, over six closed-loop ticks and a rollout."""
    import torch
    dev = torch.device("cuda", 0)
    B, N = 600, 10
    x = _x0_batch(pkg, tables, B, seed=43)
    gX, gU = _cotangent(B, N, seed=6)
    gXd, gUd = torch.from_numpy(gX).to(dev), torch.from_numpy(gU).to(dev)
    gp = torch.zeros(B, 10, dtype=torch.float64, device=dev)
    gt = torch.zeros(B, 16, dtype=torch.float64, device=dev)
    Xd = torch.zeros(B, N + 1, 8, dtype=torch.float64, device=dev)
    a, b = pkg.BatchedMPC(tables, N, B), pkg.BatchedMPC(tables, N, B)
    a.set_initial_guess(x), b.set_initial_guess(x)
    xa, xb = x.copy(), x.copy()

    def ask():
        b.prediction_dev(Xd.data_ptr(), 0)
        b.adjoint_dev(gXd.data_ptr(), gUd.data_ptr(), gp.data_ptr(), gt.data_ptr())
        b.adjoint(gX, gU)
        b.adjoint(gX, None, theta=False)

    for tick in range(6):
        ua, ub = a.make_step(xa), b.make_step(xb)
        if tick % 2:  # the adjoint first (it runs the factorisation, the ok pass and the right-hand sides) ...
            ask()
            Sb, Pb = b.sensitivities(trajectory=True), b.param_sensitivities(trajectory=True)
        else:  # ... or after the forward passes (it reuses them)
            Sb, Pb = b.sensitivities(trajectory=True), b.param_sensitivities(trajectory=True)
            ask()
        b.synchronize()
        Sa, Pa = a.sensitivities(trajectory=True), a.param_sensitivities(trajectory=True)
        for k in Sa:
            assert np.array_equal(Sa[k], Sb[k]), (tick, k)
        for k in Pa:
            assert np.array_equal(Pa[k], Pb[k]), (tick, k)
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
    b.adjoint(gX[:M], gU[:M], theta=False)
    with pytest.raises(pkg.LtompcError, match="rollout"):
        b.adjoint(gX[:M], gU[:M])
    Sa, Sb = a.sensitivities(trajectory=True), b.sensitivities(trajectory=True)
    for k in Sa:
        assert np.array_equal(Sa[k], Sb[k]), k
    xs = ta.cpu().numpy()
    assert np.array_equal(xs, tb.cpu().numpy())
    ua, ub = a.make_step(xs), b.make_step(xs)
    for i, (p, q) in enumerate(zip(_record(a, ua), _record(b, ub))):
        assert np.array_equal(p, q), i
    a.close(), b.close()
