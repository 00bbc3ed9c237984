"""mpc_solve(..., keep=True) on the GPU (lap-time-optimization_amd/autograd.py): a closed loop backpropagated on ONE
handle, every tick differentiated from its solve record after the handle has solved the later ticks."""
import numpy as np
import pytest

from test_gpu_autograd_layer import LOOP_TOL, _rows, _t, layer  # noqa: F401
from test_gpu_records import TAB_TOL

pytestmark = pytest.mark.gpu


def _t_handle_loop(pkg, tables, layer, xi, rows, T, n_sub):  # noqa: F811
    """test_three_tick_loop_against_loop_sensitivities' construction: tick t differentiated on a handle of its own that ran the
    ticks before it plainly.  Returns (u0 per tick, x per tick, grad x_init, grad theta)."""
    import torch
    B, N = xi.shape[0], 10
    hs = [pkg.BatchedMPC(tables, N, B) for _ in range(T)]
    for m in hs:
        m.set_theta(rows)
        m.set_initial_guess(xi)
    x_init, th = _t(xi, True), _t(rows, True)
    x, up = x_init, None
    scratch = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    us, xs = [], []
    for t in range(T):
        xd = x.detach().contiguous()
        for k in range(t + 1, T):
            hs[k].make_step_dev(xd.data_ptr(), scratch.data_ptr())
            hs[k].synchronize()
        u0, X, U, ok = layer.mpc_solve(hs[t], x, up, th)
        x = layer.plant_step(hs[t], x, u0, th, n_sub=n_sub)
        us.append(u0.detach().cpu().numpy()), xs.append(x.detach().cpu().numpy())
        up = u0
    (0.5 * (x * x).sum()).backward()
    out = us, xs, x_init.grad.cpu().numpy(), th.grad.cpu().numpy()
    for m in hs:
        m.close()
    return out


def test_three_tick_loop_on_one_handle(pkg, tables, gpu_lib, layer):  # noqa: F811
    """The loop of test_three_tick_loop_against_loop_sensitivities (B = 61, N = 10, T = 3, n_sub = 40) with keep=True on one
    handle: u0 and x of every tick are the reference loop's bits, the gradient of |x_3|^2 / 2 w.r.t. x_init and theta agrees with
    S^T x_3 from loop_sensitivities() within that test's LOOP_TOL, and (printed; 0 expected) with the T-handle construction."""
    B, N, T, n_sub = 61, 10, 3, 40
    xi = pkg.sample_x0(tables, B, seed=23)
    rows = _rows(pkg, B, seed=8)
    ref, h = pkg.BatchedMPC(tables, N, B), pkg.BatchedMPC(tables, N, B)
    for m in (ref, h):
        m.set_theta(rows)
        m.set_initial_guess(xi)
    ref.loop_begin(3)
    x_init, th = _t(xi, True), _t(rows, True)
    x, up, xr = x_init, None, xi
    for t in range(T):
        ur = ref.make_step(xr)
        u0, X, U, ok = layer.mpc_solve(h, x, up, th, keep=True)
        assert np.array_equal(u0.detach().cpu().numpy(), ur), t
        x = layer.plant_step(h, x, u0, th, n_sub=n_sub)
        xr = ref.loop_tick(xr, ur, n_sub=n_sub)
        assert np.array_equal(x.detach().cpu().numpy(), xr), t
        up = u0
    assert h.record_stats() == (T, 0)
    (0.5 * (x * x).sum()).backward()
    L = ref.loop_sensitivities()
    alive = L["ok"]
    assert alive.sum() >= 0.75 * B, alive.sum()
    want = np.einsum("biq,bi->bq", L["dx"], xr)
    den = np.einsum("biq,bi->bq", np.abs(L["dx"]), np.abs(xr))
    got = np.concatenate([x_init.grad.cpu().numpy(), th.grad.cpu().numpy()], axis=1)
    err = (np.abs(got - want) / np.where(den > 0, den, 1.0))[alive]
    us, xs, gx, gth = _t_handle_loop(pkg, tables, layer, xi, rows, T, n_sub)
    assert np.array_equal(xs[-1], xr)
    diff = np.abs(got - np.concatenate([gx, gth], axis=1)).max()
    print(f"three-tick loop on one handle: alive {alive.sum()}/{B} err max {err.max():.3e} median {np.median(err.max(axis=1)):.3e}; "
          f"max |grad - grad of the T-handle construction| = {diff:.3e}")
    assert np.isfinite(got).all()
    assert err.max() <= LOOP_TOL, err.max()
    del x, u0, X, U, ok, up  # (the graph goes, and the records go back to the free list)
    import gc
    gc.collect()
    assert h.record_stats() == (0, T)
    ref.close(), h.close()


def test_tables_through_two_ticks(pkg, tables, gpu_lib, layer):  # noqa: F811
    """B = 13, N = 10, two ticks with tables= and keep=True on one handle: tables.grad is the sum of the two per-tick table
    gradients of the two-handle construction (to the order of the atomic adds)."""
    import torch
    B, N, n_sub = 13, 10, 40
    xi = pkg.sample_x0(tables, B, seed=21)
    h, h0, h1 = (pkg.BatchedMPC(tables, N, B) for _ in range(3))
    for m in (h, h0, h1):
        m.set_initial_guess(xi)
    tv = h.table_values()

    def loss(Xa, Xb):
        return 0.5 * ((Xa[:, 1:] - 1.0) ** 2).sum() + 0.5 * (Xb * Xb).sum()

    # one handle, records
    tab = _t(tv, True)
    x = _t(xi)
    u0, Xa, _, _ = layer.mpc_solve(h, x, None, None, tab, keep=True)
    x1 = layer.plant_step(h, x, u0, n_sub=n_sub)
    u1, Xb, _, okb = layer.mpc_solve(h, x1, u0, None, tab, keep=True)
    loss(Xa, Xb).backward()
    assert int(okb.sum()) >= B // 2
    # two handles: tick 0 on h0, tick 1 on h1 after it ran tick 0 plainly
    tab2 = _t(tv, True)
    scratch = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h1.make_step_dev(x.data_ptr(), scratch.data_ptr())
    h1.synchronize()
    v0, Ya, _, _ = layer.mpc_solve(h0, x, None, None, tab2)
    y1 = layer.plant_step(h0, x, v0, n_sub=n_sub)
    v1, Yb, _, _ = layer.mpc_solve(h1, y1, v0, None, tab2)
    assert torch.equal(v0, u0) and torch.equal(y1, x1) and torch.equal(v1, u1) and torch.equal(Yb, Xb)
    loss(Ya, Yb).backward()
    got, want = tab.grad.cpu().numpy(), tab2.grad.cpu().numpy()
    sc = np.abs(want).max(axis=1, keepdims=True)
    print(f"tables through two ticks: max |diff| / row scale = {(np.abs(got - want) / sc).max():.3e}")
    assert (sc > 0).all() and (np.abs(got - want) <= TAB_TOL * sc).all()
    for m in (h, h0, h1):
        m.close()


def test_keep_false_is_unchanged(pkg, tables, gpu_lib, layer):  # noqa: F811
    B, N = 13, 10
    xi = pkg.sample_x0(tables, B, seed=21)
    h = pkg.BatchedMPC(tables, N, B)
    h.set_initial_guess(xi)
    x = _t(xi, True)
    u0, *_ = layer.mpc_solve(h, x)
    assert h.record_stats() == (0, 0)
    h.make_step(xi)
    with pytest.raises(RuntimeError, match="another solve"):
        u0.sum().backward()
    h.close()
