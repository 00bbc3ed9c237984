"""Per-instance control of the warm start on the GPU (ltompc_reset_instances, ltompc_set_guess, ltompc_export_state /
ltompc_import_state).

"Bits" below: u0, status, iters, iterate(), prediction() and stats() (which holds the counters, restoration and recovery
outputs), compared with array_equal.  Handles of different batch sizes are compared under one explicit options.latency_mode.
Shapes: N = 10 with B = 13 (mode 1, one part-filled wavefront) and B = 77 (mode 2, two wavefronts and padding); B = 1024 where
the packed order is needed; B = 32, N = 20, seed 21 which has an INFEASIBLE instance."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_instance_params import _repacked

pytestmark = pytest.mark.gpu

SHAPES = [(1, 13), (2, 77)]  # (latency_mode, batch)


def _opts(pkg, mode, **kw):
    o = pkg.default_options()
    o.latency_mode = mode
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _theta_rows(pkg, mpc, B):
    """per-instance rows: grip and mass scaled by up to 10 % per instance (the _pi kernels)"""
    rows = np.tile(mpc.theta(), (B, 1))
    rng = np.random.default_rng(3)
    for name in ("mass", "D_f", "D_r"):
        rows[:, pkg.THETA_NAMES.index(name)] *= 1.0 + 0.1 * rng.uniform(-1, 1, B)
    return rows


def _bits(mpc, u0):
    out = dict(u0=np.array(u0), status=mpc.status.copy(), iters=mpc.iters.copy())
    out.update({"it_" + k: v for k, v in mpc.iterate().items()})
    X, U = mpc.prediction()
    out.update(X=X, U=U)
    out.update({"st_" + k: v for k, v in mpc.stats().items()})
    return out


def _accessor_bits(mpc):
    """the bits without a host make_step (after make_step_dev)"""
    out = {"it_" + k: v for k, v in mpc.iterate().items()}
    X, U = mpc.prediction()
    out.update(X=X, U=U)
    out.update({"st_" + k: v for k, v in mpc.stats().items()})
    return out


def _same_rows(a, b, ra, rb=None, label=""):
    rb = ra if rb is None else rb
    for k in a:
        assert np.array_equal(a[k][ra], b[k][rb], equal_nan=True), (label, k)


def _subset(B):
    M = np.zeros(B, dtype=bool)
    M[[0, B // 3, B // 2, B // 2 + 1, B - 1]] = True
    return M


def _two_ticks(pkg, tables, handles, x0):
    """set_initial_guess and two ticks on every handle (the same bits on all: asserted on u0); returns the state after them"""
    for m in handles:
        m.set_initial_guess(x0)
    x = x0
    for _ in range(2):
        us = [m.make_step(x) for m in handles]
        assert all(np.array_equal(us[0], u) for u in us[1:])
        x = handles[0].plant_step(x, us[0])
    return x


# ---- 1, 12: masked reset ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("theta", [False, True])
@pytest.mark.parametrize("mode,B", SHAPES)
def test_masked_reset(pkg, tables, gpu_lib, monkeypatch, mode, B, theta, poison):
    """Rows outside the mask keep the twin's bits over two further ticks; rows inside it have the bits of a fresh handle's
    first two solves (u_prev, previous status, counters).  Also with per-instance theta rows, and with LTOMPC_POISON=1."""
    if poison:
        monkeypatch.setenv("LTOMPC_POISON", "1")
    N = 10
    A, T, F = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode)) for _ in range(3))
    if theta:
        rows = _theta_rows(pkg, A, B)
        for m in (A, T, F):
            m.set_theta(rows)
    x = _two_ticks(pkg, tables, (A, T), pkg.sample_x0(tables, B, seed=21))
    M = _subset(B)
    xn = np.where(M[:, None], pkg.sample_x0(tables, B, seed=77), x)
    count = A.solve_count
    A.reset(M, xn)
    assert A.solve_count == count + 1 and A.solved_parameters() is None
    it = A.iterate()
    assert np.array_equal(it["X"][M], np.repeat(xn[M][:, None], N + 1, 1)) and np.array_equal(it["C"][M], np.repeat(xn[M][:, None], N, 1))
    assert not it["U"][M].any() and not it["L1"][M].any() and not it["L2"][M].any()
    F.set_initial_guess(xn)
    xa, xt, xf = xn, x, xn
    for tick in range(2):
        ua, ut, uf = A.make_step(xa), T.make_step(xt), F.make_step(xf)
        ba, bt, bf = _bits(A, ua), _bits(T, ut), _bits(F, uf)
        _same_rows(ba, bt, ~M, label=f"kept {tick}")
        _same_rows(ba, bf, M, label=f"reset {tick}")
        if tick == 0:
            assert np.array_equal(A.solved_parameters()[1][M], np.zeros((M.sum(), 2)))
            assert np.array_equal(A.solved_parameters()[1][~M], T.solved_parameters()[1][~M])
        xa, xt, xf = A.plant_step(xa, ua), T.plant_step(xt, ut), F.plant_step(xf, uf)
    for m in (A, T, F):
        m.close()


# ---- 2: on a packed handle ------------------------------------------------------------------------------------------------------
def test_masked_reset_on_a_packed_handle(pkg, tables, gpu_lib):
    """B = 1024, solved through make_step_dev so that no accessor runs between the solves and the reset: the handle is in packed
    order when ~100 scattered instances are reset (the masks and rows go through `orig`)."""
    import torch
    dev = torch.device("cuda", 0)
    N, B, mode = 10, 1024, 2
    A, T, F = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode)) for _ in range(3))
    x0 = pkg.sample_x0(tables, B, seed=21)
    xa, xt = (torch.from_numpy(x0).to(dev) for _ in range(2))
    ua, ut = (torch.zeros(B, 2, dtype=torch.float64, device=dev) for _ in range(2))
    xna, xnt = torch.empty_like(xa), torch.empty_like(xt)
    torch.cuda.synchronize(dev)
    packed = False
    for m, x, u, xn in ((A, xa, ua, xna), (T, xt, ut, xnt)):
        m.set_initial_guess_dev(x.data_ptr())
        for _ in range(2):
            m.make_step_dev(x.data_ptr(), u.data_ptr())
            packed = packed or _repacked(m)   # (host-side history: no accessor)
            m.plant_step_dev(x.data_ptr(), u.data_ptr(), xn.data_ptr(), 100)
            m.synchronize()
            x.copy_(xn)
        torch.cuda.synchronize(dev)
    assert packed and torch.equal(xa, xt)
    M = np.zeros(B, dtype=bool)
    M[np.random.default_rng(5).choice(B, 100, replace=False)] = True
    xnew = np.where(M[:, None], pkg.sample_x0(tables, B, seed=78), xa.cpu().numpy())
    A.reset(M, xnew)
    xa.copy_(torch.from_numpy(xnew).to(dev))
    torch.cuda.synchronize(dev)
    F.set_initial_guess(xnew)
    xf = xnew
    for tick in range(2):
        A.make_step_dev(xa.data_ptr(), ua.data_ptr()), T.make_step_dev(xt.data_ptr(), ut.data_ptr())
        A.synchronize(), T.synchronize()
        uf = F.make_step(xf)
        a, t = ua.cpu().numpy(), ut.cpu().numpy()
        assert np.array_equal(a[~M], t[~M]) and np.array_equal(a[M], uf[M]), tick
        if tick == 1:
            ba, bt, bf = _accessor_bits(A), _accessor_bits(T), _accessor_bits(F)
            _same_rows(ba, bt, ~M, label="kept")
            _same_rows(ba, bf, M, label="reset")
        else:
            for m, x, u, xn in ((A, xa, ua, xna), (T, xt, ut, xnt)):
                m.plant_step_dev(x.data_ptr(), u.data_ptr(), xn.data_ptr(), 100)
                m.synchronize()
                x.copy_(xn)
            torch.cuda.synchronize(dev)
            xf = F.plant_step(xf, uf, 100)
            assert np.array_equal(xa.cpu().numpy()[M], xf[M])
    for m in (A, T, F):
        m.close()


# ---- 3: edge masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", SHAPES)
def test_edge_masks(pkg, tables, gpu_lib, mode, B):
    N = 10
    A, G, Z, T = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode)) for _ in range(4))
    x = _two_ticks(pkg, tables, (A, G, Z, T), pkg.sample_x0(tables, B, seed=21))
    xn = pkg.sample_x0(tables, B, seed=77)
    A.reset(np.ones(B, dtype=bool), xn)
    G.set_initial_guess(xn)
    ia, ig = A.iterate(), G.iterate()
    assert all(np.array_equal(ia[k], ig[k], equal_nan=True) for k in ia)
    _same_rows(_bits(A, A.make_step(xn)), _bits(G, G.make_step(xn)), slice(None), label="all ones")
    Z.reset(np.zeros(B, dtype=bool), xn)
    _same_rows(_bits(Z, Z.make_step(x)), _bits(T, T.make_step(x)), slice(None), label="all zeros")
    for m in (A, G, Z, T):
        m.close()


# ---- 4: reset, then rollout -----------------------------------------------------------------------------------------------------
def test_reset_then_rollout(pkg, tables, gpu_lib):
    """The rollout's first pass honours the flag per instance: its logs are those of reset + a make_step / plant_step loop."""
    import torch
    dev = torch.device("cuda", 0)
    N, B, K, n_sub = 10, 77, 3, 50
    A, T = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2)) for _ in range(2))
    x = _two_ticks(pkg, tables, (A, T), pkg.sample_x0(tables, B, seed=21))
    M = _subset(B)
    xn = np.where(M[:, None], pkg.sample_x0(tables, B, seed=77), x)
    A.reset(M, xn), T.reset(M, xn)
    U, S, I = [], [], []
    xs = xn
    for _ in range(K):
        u = T.make_step(xs)
        U.append(u.copy()), S.append(T.status.copy()), I.append(T.iters.copy())
        xs = T.plant_step(xs, u, n_sub)
    xr = torch.from_numpy(xn).to(dev)
    ul = torch.zeros(B, K, 2, dtype=torch.float64, device=dev)
    sl, il = (torch.full((B, K), -1, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize(dev)
    A.rollout_dev(xr.data_ptr(), K, n_sub, ul.data_ptr(), sl.data_ptr(), il.data_ptr())
    torch.cuda.synchronize(dev)
    assert np.array_equal(ul.cpu().numpy(), np.stack(U, 1)) and np.array_equal(sl.cpu().numpy(), np.stack(S, 1))
    assert np.array_equal(il.cpu().numpy(), np.stack(I, 1)) and np.array_equal(xr.cpu().numpy(), xs)
    A.close(), T.close()


# ---- 5: order of reset and set_u_prev -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", SHAPES)
def test_order_of_reset_and_set_u_prev(pkg, tables, gpu_lib, mode, B):
    N = 10
    mk = lambda: pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))  # noqa: E731
    before, after, T, F0, F1 = mk(), mk(), mk(), mk(), mk()
    x = _two_ticks(pkg, tables, (before, after, T), pkg.sample_x0(tables, B, seed=21))
    M = _subset(B)
    xn = np.where(M[:, None], pkg.sample_x0(tables, B, seed=77), x)
    up = np.random.default_rng(1).uniform(-0.2, 0.2, (B, 2))
    before.set_u_prev(up), before.reset(M, xn)      # zeroed for M, kept for the others
    after.reset(M, xn), after.set_u_prev(up)        # used by all
    T.set_u_prev(up)
    F0.set_initial_guess(xn)
    F1.set_initial_guess(xn), F1.set_u_prev(up)
    bb, ba = _bits(before, before.make_step(xn)), _bits(after, after.make_step(xn))
    bt, b0, b1 = _bits(T, T.make_step(x)), _bits(F0, F0.make_step(xn)), _bits(F1, F1.make_step(xn))
    _same_rows(bb, bt, ~M, label="before, kept"), _same_rows(bb, b0, M, label="before, reset")
    _same_rows(ba, bt, ~M, label="after, kept"), _same_rows(ba, b1, M, label="after, reset")
    assert not np.array_equal(b0["u0"][M], b1["u0"][M])  # (u_prev matters)
    assert np.array_equal(before.solved_parameters()[1], np.where(M[:, None], 0.0, up)) and np.array_equal(after.solved_parameters()[1], up)
    for m in (before, after, T, F0, F1):
        m.close()


# ---- 6: guess, exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", SHAPES)
def test_guess_is_a_previous_solution_that_did_not_converge(pkg, tables, gpu_lib, mode, B):
    N = 10
    A, G = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode, max_iter=4)) for _ in range(2))
    x0 = pkg.sample_x0(tables, B, seed=21)
    A.set_initial_guess(x0)
    u0 = A.make_step(x0)
    assert (A.status == 2).all()  # MAX_ITER, every instance
    it = A.iterate()
    x1 = A.plant_step(x0, u0)
    ba = _bits(A, A.make_step(x1))
    G.set_guess(np.ones(B, dtype=bool), it["X"], it["U"], C=it["C"], u_prev=u0)
    gi = G.iterate()
    assert all(np.array_equal(gi[k], it[k]) for k in ("X", "C", "U")) and not gi["L1"].any() and not gi["L2"].any()
    bg = _bits(G, G.make_step(x1))
    _same_rows(ba, bg, slice(None))
    assert np.array_equal(G.solved_parameters()[1], u0)
    A.close(), G.close()


# ---- 7: guess against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolate", [False, True])
def test_guess_matches_oracle(pkg, tables, orc, gpu_lib, interpolate):
    """The guess is the oracle's cold solution at x0; the solve is at x1 = plant(x0, u0) with u_prev = u0.  Criteria of
    test_warm_start_options_match_oracle: both sides SOLVED for at least 0.95 of the instances, |u0 - oracle| < 1e-5 there."""
    B, N = 32, 20
    oracle = orc.Oracle(tables.packed())
    x0 = pkg.sample_x0(tables, B, seed=21)
    cold = oracle.solve(x0, N, nthreads=8)
    x1 = oracle.plant_step(x0, cold["u0"])
    Cg = pkg.solver.guess_collocation(cold["X"]) if interpolate else cold["C"]
    ref = oracle.solve(x1, N, uprev=cold["u0"], warm=dict(X=cold["X"], C=Cg, U=cold["U"], L1=np.zeros_like(cold["L1"]), L2=np.zeros_like(cold["L2"])),
                       nthreads=8, prev_status=np.full(B, 2))
    mpc = pkg.BatchedMPC(tables, N, B)
    mpc.set_guess(np.ones(B, dtype=bool), cold["X"], cold["U"], C=None if interpolate else cold["C"], u_prev=cold["u0"])
    u0 = mpc.make_step(x1)
    both = (mpc.status == 0) & (ref["status"] == 0)
    print("both solved", both.mean(), "max |u0 - oracle|", np.abs(u0 - ref["u0"])[both].max(), "iters", mpc.iters.mean(), ref["iters"].mean())
    assert both.mean() >= 0.95, both.mean()
    assert np.abs(u0 - ref["u0"])[both].max() < 1e-5
    mpc.close()


# ---- 8: checkpoint --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", SHAPES)
def test_checkpoint(pkg, tables, gpu_lib, mode, B):
    N = 10
    A = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode))
    x = _two_ticks(pkg, tables, (A,), pkg.sample_x0(tables, B, seed=21))
    blob = A.export_state()
    assert blob.shape == (B, A.warm_state_size) and A.warm_state_size == 34 * N + 18 and np.isfinite(blob).all()
    first = _bits(A, A.make_step(x))
    A.import_state(blob)
    it = A.iterate()
    assert np.array_equal(A.export_state(), blob) and np.array_equal(it["X"].reshape(B, -1), blob[:, 10:10 + 8 * (N + 1)])
    _same_rows(first, _bits(A, A.make_step(x)), slice(None))
    A.close()


# ---- 9, 12: transplant ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
def test_transplant(pkg, tables, gpu_lib, monkeypatch, poison):
    """13 instances of a B = 32 handle (resto_sticky = 2; the INFEASIBLE instance of seed 21 among them), exported in permuted
    order after two ticks, continue bit for bit in a fresh 13-instance handle and in scattered slots of a packed B = 1024
    handle, whose other slots equal their twin."""
    import torch
    if poison:
        monkeypatch.setenv("LTOMPC_POISON", "1")
    dev = torch.device("cuda", 0)
    B, N, mode = 32, 20, 2
    o = _opts(pkg, mode, resto_sticky=2)
    A = pkg.BatchedMPC(tables, N, B, options=o)
    x = _two_ticks(pkg, tables, (A,), pkg.sample_x0(tables, B, seed=21))
    st = A.stats()
    inf = np.flatnonzero(st["status_solver"] == 5)
    assert inf.size >= 1, st["status_solver"]
    rest = np.setdiff1d(np.arange(B), inf[:1])
    sel = np.random.default_rng(9).permutation(np.concatenate([inf[:1], rest[::2][:12]]))
    assert sel.size == 13
    blob = A.export_state(sel)
    G = pkg.BatchedMPC(tables, N, 13, options=o)
    G.import_state(blob)
    # a packed B = 1024 handle and its twin
    Bp = 1024
    P, T = (pkg.BatchedMPC(tables, N, Bp, options=o) for _ in range(2))
    xp0 = pkg.sample_x0(tables, Bp, seed=5)
    xs, us, xns = [], [], []
    packed = False
    for m in (P, T):
        xq = torch.from_numpy(xp0).to(dev)
        uq, xnq = torch.zeros(Bp, 2, dtype=torch.float64, device=dev), torch.empty_like(xq)
        torch.cuda.synchronize(dev)
        m.set_initial_guess_dev(xq.data_ptr())
        m.make_step_dev(xq.data_ptr(), uq.data_ptr())
        packed = packed or _repacked(m)
        m.plant_step_dev(xq.data_ptr(), uq.data_ptr(), xnq.data_ptr(), 100)
        m.synchronize()
        xs.append(xnq), us.append(uq)
    assert packed
    slots = np.random.default_rng(10).choice(Bp, 13, replace=False)
    P.import_state(blob, slots)
    xp = xs[0].cpu().numpy()
    xp[slots] = x[sel]
    xs[0].copy_(torch.from_numpy(xp).to(dev))
    torch.cuda.synchronize(dev)
    ba, bg = _bits(A, A.make_step(x)), _bits(G, G.make_step(x[sel]))
    _same_rows(ba, bg, sel, slice(None), label="fresh handle")
    assert (ba["st_status_solver"][sel] == 5).any() or (ba["st_n_resto"][sel] > 0).any()  # (the sticky path is among them)
    for m, xq, uq in zip((P, T), xs, us):
        m.make_step_dev(xq.data_ptr(), uq.data_ptr())
        m.synchronize()
    bp, bt = _accessor_bits(P), _accessor_bits(T)
    others = np.setdiff1d(np.arange(Bp), slots)
    _same_rows(bp, bt, others, label="other slots")
    assert np.array_equal(us[0].cpu().numpy()[others], us[1].cpu().numpy()[others])
    assert np.array_equal(us[0].cpu().numpy()[slots], ba["u0"][sel])
    for k in bp:
        if k not in ba:
            continue
        assert np.array_equal(bp[k][slots], ba[k][sel], equal_nan=True), ("packed", k)
    for m in (A, G, P, T):
        m.close()


# ---- 10: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, tables, gpu_lib):
    N, B = 10, 13
    A, T, other = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 1)), pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 1)), pkg.BatchedMPC(tables, 12, B)
    x = _two_ticks(pkg, tables, (A, T), pkg.sample_x0(tables, B, seed=21))
    blob, it = A.export_state(), A.iterate()
    ones = np.ones(B, dtype=np.int32)
    dp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    L, h = gpu_lib, A._h
    # usage errors are codes ...
    wrong = other.export_state()
    assert L.ltompc_import_state(h, None, B, dp(np.ascontiguousarray(wrong[:, :blob.shape[1]]))) == -1 and b"header" in L.ltompc_last_error()
    bad = np.arange(B, dtype=np.int32); bad[3] = B
    assert L.ltompc_import_state(h, ip(bad), B, dp(blob)) == -1 and b"range" in L.ltompc_last_error()
    assert L.ltompc_export_state(h, ip(bad), B, dp(np.empty_like(blob))) == -1
    bad[3] = 2
    assert L.ltompc_import_state(h, ip(bad), B, dp(blob)) == -1 and b"twice" in L.ltompc_last_error()
    nan = blob.copy(); nan[5, 40] = np.nan
    assert L.ltompc_import_state(h, None, B, dp(nan)) == -1 and b"non-finite" in L.ltompc_last_error()
    nanx = x.copy(); nanx[2, 1] = np.inf
    assert L.ltompc_reset_instances(h, ip(ones), dp(nanx)) == -1
    nanX = it["X"].copy(); nanX[1, 3, 2] = np.nan
    assert L.ltompc_set_guess(h, ip(ones), dp(nanX), dp(it["C"]), dp(it["U"]), None) == -1
    A.loop_begin(3)
    for call in (lambda: A.reset(ones, x), lambda: A.set_guess(ones, it["X"], it["U"]), lambda: A.import_state(blob)):
        with pytest.raises(pkg.LtompcError, match="open loop"):
            call()
    A.loop_end()
    A.sensitivities()  # ... and left the handle as it was: the last solve can still be differentiated,
    _same_rows(_bits(A, A.make_step(x)), _bits(T, T.make_step(x)), slice(None))  # and the next tick is the twin's
    # after an import or a guess every derivative pass refuses until the next solve
    g = np.ones((B, N + 1, 8))
    for change in (lambda: A.import_state(blob), lambda: A.set_guess(ones, it["X"], it["U"]), lambda: A.reset(ones, x)):
        A.make_step(x)
        A.sensitivities()
        change()
        for deriv in (A.sensitivities, A.param_sensitivities, lambda: A.adjoint(gX=g), lambda: A.jvp(dp=np.ones((B, 10))),
                      lambda: A.adjoint_tables(gX=g)):
            with pytest.raises(pkg.LtompcError):
                deriv()
    for m in (A, T, other):
        m.close()


# ---- 11: SplitMPC ---------------------------------------------------------------------------------------------------------------
def test_split_mpc(pkg, tables, gpu_lib):
    """Three parts, B = 77: reset, guess and export / import by global index equal the single handle."""
    import torch
    dev = torch.device("cuda", 0)
    N, B = 10, 77
    o = _opts(pkg, 2)
    one, three = pkg.BatchedMPC(tables, N, B, options=o), pkg.SplitMPC(tables, N, B, n_parts=3, options=o)
    x0 = pkg.sample_x0(tables, B, seed=21)
    bufs = {}
    for name, m in (("one", one), ("three", three)):
        x, u, xn = torch.from_numpy(x0).to(dev), torch.zeros(B, 2, dtype=torch.float64, device=dev), torch.zeros(B, 8, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        m.set_initial_guess_dev(x.data_ptr())
        bufs[name] = (x, u, xn)

    def tick(set_x=None):
        out = []
        for name, m in (("one", one), ("three", three)):
            x, u, xn = bufs[name]
            if set_x is not None:
                x.copy_(torch.from_numpy(set_x).to(dev))
                torch.cuda.synchronize(dev)
            m.make_step_dev(x.data_ptr(), u.data_ptr())
            m.synchronize()
            for p, (lo, hi) in ((m, (0, B)),) if name == "one" else zip(m.parts, m.bounds):
                p.plant_step_dev(x.data_ptr() + 64 * lo, u.data_ptr() + 16 * lo, xn.data_ptr() + 64 * lo, 100)
                p.synchronize()
            x.copy_(xn)
            torch.cuda.synchronize(dev)
            it, st = m.iterate(), m.stats()
            out.append(dict(u0=u.cpu().numpy(), x=x.cpu().numpy(), **{"it_" + k: v for k, v in it.items()}, **{"st_" + k: v for k, v in st.items()}))
        _same_rows(out[0], out[1], slice(None))
        return out[0]

    tick(), tick()
    M = _subset(B)
    M[:26] = False  # (the first part has nothing to do)
    cur = tick()["x"]
    xn = np.where(M[:, None], pkg.sample_x0(tables, B, seed=77), cur)
    one.reset(M, xn), three.reset(M, xn)
    r = tick(xn)
    M2 = np.zeros(B, dtype=bool); M2[[1, 30, 76]] = True
    one.set_guess(M2, r["it_X"][::-1].copy(), r["it_U"][::-1].copy()), three.set_guess(M2, r["it_X"][::-1].copy(), r["it_U"][::-1].copy())
    tick()
    idx = np.array([70, 3, 27, 51, 26])
    b1, b3 = one.export_state(idx), three.export_state(idx)
    assert np.array_equal(b1, b3) and np.array_equal(one.export_state(), three.export_state())
    to = np.array([0, 76, 25, 52, 40])
    one.import_state(b1, to), three.import_state(b3, to)
    tick(), tick()
    one.close(), three.close()
