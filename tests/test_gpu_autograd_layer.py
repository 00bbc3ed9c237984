"""The autograd layer (lap-time-optimization_amd/autograd.py) on the GPU: mpc_solve's forward is make_step_dev +
prediction_dev, its backward the adjoint pass and its forward mode the directional pass, bit for bit; plant_step's backward is
the contraction of plant_sensitivities(); a three-tick closed loop differentiated end to end against loop_sensitivities()."""
import importlib

import numpy as np
import pytest

import param_sens_reference as PR
from test_gpu_sensitivity_dense import _x0_batch

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# plant_step's backward: a float64 dot product of n <= 16 terms in another order of summation than the host's: n eps sum |terms|
PLANT_TOL = 16 * EPS
# The three-tick loop, per instance and column j of q = (x_init, theta): |grad_j - (S^T x_3)_j| / sum_i |S_ij| |x_3,i| with S =
# loop_sensitivities()["dx"].  Reverse mode through the adjoint pass against the forward accumulation through the two forward
# passes, on the same factorisations.  Measured on MI355X (profiles/jvp/README.md): 58 of 61 instances alive after the three
# ticks, max 5.35e-9 (column q_B), median of the per-instance maxima 1.3e-15.  The bound is 10 x that.
LOOP_MEASURED = 5.35e-9
LOOP_TOL = 10.0 * LOOP_MEASURED


@pytest.fixture(scope="module")
def layer():
    return importlib.import_module("lap-time-optimization_amd.autograd")


def _t(a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda").requires_grad_(grad)


def _rows(pkg, B, seed):
    """per-instance rows: the default theta with a seeded change of up to 3 % in every column"""
    th = PR.theta_values(pkg.default_params())
    return th * (1.0 + np.random.default_rng(seed).uniform(-0.03, 0.03, (B, 16)))


def test_mpc_solve_is_the_solve_the_adjoint_and_the_jvp_bit_for_bit(pkg, tables, gpu_lib, layer):
    import torch
    import torch.autograd.forward_ad as fwAD
    B, N = 61, 10
    x = _x0_batch(pkg, tables, B, seed=31)
    rows = _rows(pkg, B, seed=1)
    a, b = pkg.BatchedMPC(tables, N, B), pkg.BatchedMPC(tables, N, B)
    for m in (a, b):
        m.set_initial_guess(x)
        m.set_theta(rows)
    u1 = a.make_step(x)
    assert np.array_equal(b.make_step(x), u1)
    x1 = a.plant_step(x, u1, 50)
    v = u1 + np.random.default_rng(2).uniform(-0.01, 0.01, (B, 2))
    # the twin: the same solve through the plain device-pointer calls
    xd, vd, thd = _t(x1), _t(v), _t(rows)
    u0r, Xr, Ur = (torch.full(s, np.nan, dtype=torch.float64, device="cuda") for s in ((B, 2), (B, N + 1, 8), (B, N, 2)))
    torch.cuda.synchronize()  # (torch's fills run on torch's stream, the handle on its own: order them)
    b.set_theta_dev(thd.data_ptr())
    b.set_u_prev_dev(vd.data_ptr())
    b.make_step_dev(xd.data_ptr(), u0r.data_ptr())
    b.prediction_dev(Xr.data_ptr(), Ur.data_ptr())
    b.synchronize()
    # the layer
    x0, up, th = _t(x1, True), _t(v, True), _t(rows, True)
    u0, X, U, ok = layer.mpc_solve(a, x0, up, th)
    assert torch.equal(u0, u0r) and torch.equal(X, Xr) and torch.equal(U, Ur)
    S = b.sensitivities()
    assert np.array_equal(ok.cpu().numpy() != 0, S["ok"]) and S["ok"].sum() >= 8 and not ok.requires_grad
    # a seeded quadratic loss of (u0, X, U): its cotangents by hand, through adjoint()
    g = torch.Generator(device="cpu").manual_seed(3)
    wu, wX, wU = (torch.randn(s, dtype=torch.float64, generator=g).cuda() for s in ((B, 2), (B, N + 1, 8), (B, N, 2)))
    loss = 0.5 * ((wu * u0 * u0).sum() + (wX * X * X).sum() + (wU * U * U).sum())
    loss.backward()
    gX, gU = (wX * X).detach(), (wU * U).detach().clone()
    gU[:, 0] += (wu * u0).detach()
    A = b.adjoint(gX.cpu().numpy(), gU.cpu().numpy())
    assert np.array_equal(x0.grad.cpu().numpy(), A["grad_x0"])
    assert np.array_equal(up.grad.cpu().numpy(), A["grad_uprev"])
    assert np.array_equal(th.grad.cpu().numpy(), A["grad_theta"])
    assert (x0.grad[~(ok != 0)] == 0).all()
    # forward mode
    rng = np.random.default_rng(4)
    dp, dth = rng.standard_normal((B, 10)), rows * rng.uniform(-0.05, 0.05, (B, 16))
    a.set_initial_guess(x)  # (a fresh solve on the same handle: the same ticks again)
    a.make_step(x)
    with fwAD.dual_level():
        du0, dX, dU, dok = layer.mpc_solve(a, fwAD.make_dual(_t(x1), _t(dp[:, :8])), fwAD.make_dual(_t(v), _t(dp[:, 8:])),
                                           fwAD.make_dual(_t(rows), _t(dth)))
        tu0, tX, tU = (fwAD.unpack_dual(q).tangent for q in (du0, dX, dU))
        assert fwAD.unpack_dual(dok).tangent is None
        assert torch.equal(fwAD.unpack_dual(dX).primal, Xr)
    J = b.jvp(dp, dth)
    assert np.array_equal(tX.cpu().numpy(), J["tX"]) and np.array_equal(tU.cpu().numpy(), J["tU"])
    assert np.array_equal(tu0.cpu().numpy(), J["tU"][:, 0])
    # stale: another solve on the handle, then backward of the earlier one
    u0, *_ = layer.mpc_solve(a, x0, up, th)
    a.make_step(x1)
    with pytest.raises(RuntimeError, match="another solve"):
        u0.sum().backward()
    a.close(), b.close()


def test_plant_step_backward_is_the_contraction_of_plant_sensitivities(pkg, tables, gpu_lib, layer):
    import torch
    B, n_sub = 61, 40
    x = _x0_batch(pkg, tables, B, seed=33)
    u = np.random.default_rng(5).uniform(-1.0, 1.0, (B, 2)) * np.array([0.3, 1.0])
    rows = _rows(pkg, B, seed=6)
    mpc = pkg.BatchedMPC(tables, 10, B)
    xt, ut, tht = _t(x, True), _t(u, True), _t(rows, True)
    xn = layer.plant_step(mpc, xt, ut, tht, n_sub=n_sub)
    mpc.set_theta(rows)
    R = mpc.plant_sensitivities(x, u, n_sub=n_sub)
    assert np.array_equal(xn.detach().cpu().numpy(), R["x_next"])
    assert np.array_equal(xn.detach().cpu().numpy(), mpc.plant_step(x, u, n_sub=n_sub))  # k_plant's bits
    g = np.random.default_rng(7).standard_normal((B, 8))
    xn.backward(_t(g))
    worst = 0.0
    for got, D in ((xt.grad, R["dx"]), (ut.grad, R["du"]), (tht.grad, R["dtheta"])):
        want, den = np.einsum("bi,bij->bj", g, D), np.einsum("bi,bij->bj", np.abs(g), np.abs(D))
        err = np.abs(got.cpu().numpy() - want) / np.where(den > 0, den, 1.0)
        worst = max(worst, err.max())
        assert err.max() <= PLANT_TOL, err.max()
    print(f"plant_step backward: max error / sum |terms| = {worst:.3e}")
    # theta without a gradient: its columns are not computed, the others are the same bits
    x2, u2 = _t(x, True), _t(u, True)
    layer.plant_step(mpc, x2, u2, _t(rows), n_sub=n_sub).backward(_t(g))
    assert torch.equal(x2.grad, xt.grad) and torch.equal(u2.grad, ut.grad)
    mpc.close()


def test_three_tick_loop_against_loop_sensitivities(pkg, tables, gpu_lib, layer):
    """x_{t+1} = plant(x_t, solve(x_t, u0_{t-1}, theta), theta) for three ticks (N = 10, B = 61, n_sub = 40): the gradient of
    |x_3|^2 / 2 w.r.t. x_init and theta against S^T x_3 from loop_sensitivities() (mode 3) of a handle that runs the same loop.
    The handle is stateful and a solve's derivatives go with the next solve, so tick t is differentiated on a handle of its own
    that ran the ticks before it plainly (the same warm starts, hence the same iterates as the one-handle loop, asserted)."""
    import torch
    B, N, T, n_sub = 61, 10, 3, 40
    xi = pkg.sample_x0(tables, B, seed=23)
    rows = _rows(pkg, B, seed=8)
    ref = pkg.BatchedMPC(tables, N, B)
    hs = [pkg.BatchedMPC(tables, N, B) for _ in range(T)]
    for m in [ref] + hs:
        m.set_theta(rows)
        m.set_initial_guess(xi)
    ref.loop_begin(3)
    x_init, th = _t(xi, True), _t(rows, True)
    x, up = x_init, None
    xr = xi
    scratch = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for t in range(T):
        ur = ref.make_step(xr)
        xd = x.detach().contiguous()
        for k in range(t + 1, T):  # the handles of the later ticks follow plainly
            hs[k].make_step_dev(xd.data_ptr(), scratch.data_ptr())
            hs[k].synchronize()
        u0, X, U, ok = layer.mpc_solve(hs[t], x, up, th)
        assert np.array_equal(u0.detach().cpu().numpy(), ur), t
        x = layer.plant_step(hs[t], x, u0, th, n_sub=n_sub)
        xr = ref.loop_tick(xr, ur, n_sub=n_sub)
        assert np.array_equal(x.detach().cpu().numpy(), xr), t
        up = u0
    (0.5 * (x * x).sum()).backward()
    L = ref.loop_sensitivities()
    alive = L["ok"]
    assert alive.sum() >= 0.75 * B, alive.sum()
    want = np.einsum("biq,bi->bq", L["dx"], xr)
    den = np.einsum("biq,bi->bq", np.abs(L["dx"]), np.abs(xr))
    got = np.concatenate([x_init.grad.cpu().numpy(), th.grad.cpu().numpy()], axis=1)
    err = (np.abs(got - want) / np.where(den > 0, den, 1.0))[alive]
    print(f"three-tick loop: alive {alive.sum()}/{B} err max {err.max():.3e} median {np.median(err.max(axis=1)):.3e} "
          f"worst column {int(np.argmax(err.max(axis=0)))}")
    assert np.isfinite(got).all()
    assert err.max() <= LOOP_TOL, err.max()
    for m in [ref] + hs:
        m.close()
