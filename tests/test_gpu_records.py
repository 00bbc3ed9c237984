"""Solve records on the GPU (ltompc_record_*): the derivative passes of an EARLIER solve of a handle, from a device
copy of what they read, bit for bit what they returned right after that solve.

"Bits" below: sensitivities(trajectory=True), param_sensitivities(trajectory=True), adjoint(theta=True), jvp(dp, dtheta) and
adjoint_tables(slots=True)'s slot_grad and ok, compared with array_equal.  grad_tables is a sum of atomic adds over the instances:
equal to 1e-10 x the row's scale, the bound tests/test_gpu_table_sets.py uses for it.
Shapes (those of the warm-state tests): N = 10 with B = 13 (mode 1, latency mode: k_sens_eval8, one part-filled wavefront) and
B = 77 (mode 2, two wavefronts and padding); B = 32, N = 20, seed 21, which has an INFEASIBLE instance; B = 1024 where the packed
order is needed."""
import numpy as np
import pytest

from test_gpu_instance_params import _repacked
from test_gpu_warm_state import _opts, _theta_rows, _two_ticks

pytestmark = pytest.mark.gpu

SHAPES = [(1, 13, 10), (2, 77, 10), (2, 32, 20)]  # (latency_mode, batch, horizon)
TAB_TOL = 1e-10


def _dirs(B, N, seed):
    rng = np.random.default_rng(seed)
    return dict(gX=rng.standard_normal((B, N + 1, 8)), gU=rng.standard_normal((B, N, 2)), dp=rng.standard_normal((B, 10)),
                dth=rng.uniform(-0.05, 0.05, (B, 16)))


def _passes(mpc, d, theta=True, tables=True):
    """every pass of the solve the handle's passes refer to now: (bits, grad_tables)"""
    out = {"s_" + k: v for k, v in mpc.sensitivities(trajectory=True).items()}
    if theta:
        out.update({"p_" + k: v for k, v in mpc.param_sensitivities(trajectory=True).items() if k != "names"})
    out.update({"a_" + k: v for k, v in mpc.adjoint(d["gX"], d["gU"], theta=theta).items() if k != "names"})
    out.update({"j_" + k: v for k, v in mpc.jvp(d["dp"], d["dth"] if theta else None).items()})
    gt = None
    if tables:
        T = mpc.adjoint_tables(d["gX"], d["gU"], slots=True)
        out.update(t_slot_grad=T["slot_grad"], t_ok=T["ok"])
        gt = T["grad_tables"]
    return out, gt


def _assert_same(got, want, label=""):
    (a, ga), (b, gb) = got, want
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)
    if gb is not None:
        sc = np.abs(gb).max(axis=1, keepdims=True)
        assert (np.abs(ga - gb) <= TAB_TOL * sc).all(), (label, "grad_tables", np.abs(ga - gb).max())


def _disturb(pkg, tables, mpc, B, x):
    """what takes a live solve away: two more ticks from other states, other theta rows, another v_ref row, a reset of a third of
    the instances and an initial guess"""
    xo = pkg.sample_x0(tables, B, seed=77)
    for _ in range(2):
        xo = mpc.plant_step(xo, mpc.make_step(xo))
    rows = _theta_rows(pkg, mpc, B)
    mpc.set_theta(rows[::-1].copy())
    mpc.set_table_values(3, 0.8 * mpc.table_values()[3])  # (v_ref)
    M = np.arange(B) % 3 == 0
    mpc.reset(M, np.where(M[:, None], x, xo))
    mpc.set_initial_guess(x)
    return xo


def _save_disturb_select(pkg, tables, mode, B, N):
    A, T1, T2 = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, mode)) for _ in range(3))
    rows = _theta_rows(pkg, A, B)
    for m in (A, T1, T2):
        m.set_theta(rows)
    x = _two_ticks(pkg, tables, (A, T1, T2), pkg.sample_x0(tables, B, seed=21))
    d = _dirs(B, N, 5)
    want = _passes(T1, d)
    assert want[0]["s_ok"].sum() >= B // 2
    count = A.solve_count
    rec = A.record()
    assert A.solve_count == count and A.record_stats() == (1, 0)
    xo = _disturb(pkg, tables, A, B, x)
    assert np.array_equal(_disturb(pkg, tables, T2, B, x), xo)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        A.sensitivities()
    A.select_record(rec)
    _assert_same(_passes(A, d), want, "selected")
    # the handle goes on while the record is selected: the live accessors show the live solve, the passes the record
    ua, u2 = A.make_step(xo), T2.make_step(xo)
    assert np.array_equal(ua, u2) and np.array_equal(A.status, T2.status)
    Xa, Xt = A.prediction(), T2.prediction()
    assert np.array_equal(Xa[0], Xt[0]) and np.array_equal(Xa[1], Xt[1])
    _assert_same(_passes(A, d), want, "selected, after a further solve")
    A.select_record(None)
    _assert_same(_passes(A, d), _passes(T2, d), "live again")
    rec.release()
    for m in (A, T1, T2):
        m.close()


# ---- 1: save, disturb, select ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,N", SHAPES)
def test_save_disturb_select(pkg, tables, gpu_lib, mode, B, N):
    _save_disturb_select(pkg, tables, mode, B, N)


# ---- 8: the same with poisoned work buffers ----------------------------------------------------------------------------------
def test_save_disturb_select_poisoned(pkg, tables, gpu_lib, monkeypatch):
    monkeypatch.setenv("LTOMPC_POISON", "1")
    _save_disturb_select(pkg, tables, 1, 13, 10)


# ---- 2: on a packed handle --------------------------------------------------------------------------------------------------------
def test_save_from_a_packed_handle(pkg, tables, gpu_lib):
    """B = 1024 through make_step_dev only, so that no accessor un-packs: the record is gathered from the packed order (d_inv) and
    equals the passes of a twin in the caller's order."""
    import torch
    dev = torch.device("cuda", 0)
    N, B = 10, 1024
    A, T = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2)) for _ in range(2))
    x0 = pkg.sample_x0(tables, B, seed=21)
    xa, xt = (torch.from_numpy(x0).to(dev) for _ in range(2))
    ua, ut = (torch.zeros(B, 2, dtype=torch.float64, device=dev) for _ in range(2))
    xn = torch.empty_like(xa)
    torch.cuda.synchronize(dev)
    for m, x, u in ((A, xa, ua), (T, xt, ut)):
        packed = False
        m.set_initial_guess_dev(x.data_ptr())
        for tick in range(2):
            m.make_step_dev(x.data_ptr(), u.data_ptr())
            packed = packed or _repacked(m)  # (host-side history: no accessor; the handle stays packed from then on)
            if tick == 0:
                m.plant_step_dev(x.data_ptr(), u.data_ptr(), xn.data_ptr(), 100)
                m.synchronize()
                x.copy_(xn)
                torch.cuda.synchronize(dev)
        m.synchronize()
        assert packed, m.history()
    rec = A.record()  # (A is still in packed order: nothing has un-packed it)
    A.plant_step_dev(xa.data_ptr(), ua.data_ptr(), xn.data_ptr(), 100)
    A.make_step_dev(xn.data_ptr(), ua.data_ptr())
    A.synchronize()
    T.iterate()  # (the twin in the caller's order)
    d = _dirs(B, N, 6)
    want = _passes(T, d)
    with A.differentiating(rec):
        _assert_same(_passes(A, d), want, "packed")
    A.close(), T.close()


# ---- 3: several records -----------------------------------------------------------------------------------------------------------
def test_several_records(pkg, tables, gpu_lib):
    N, B = 10, 77
    A = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    twins = [pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2)) for _ in range(4)]
    x = pkg.sample_x0(tables, B, seed=21)
    for m in [A] + twins:
        m.set_initial_guess(x)
    d = _dirs(B, N, 7)
    recs, want = [], []
    for t in range(4):
        u = A.make_step(x)
        for k in range(t, 4):  # twin k stops at tick k
            assert np.array_equal(twins[k].make_step(x), u)
        want.append(_passes(twins[t], d))
        if t < 3:
            recs.append(A.record())
        x = A.plant_step(x, u, 50)
    assert A.record_stats() == (3, 0)
    first = None
    for i in (2, 0, 1, 0):
        A.select_record(recs[i])
        got = _passes(A, d)
        _assert_same(got, want[i], f"record {i}")
        if i == 0 and first is None:
            first = got
    _assert_same(got, first, "second visit of r0")
    A.select_record(None)
    assert A.record(into=recs[1]) is recs[1] and A.record_stats() == (3, 0)
    with A.differentiating(recs[1]):
        _assert_same(_passes(A, d), want[3], "overwritten r1")
    for m in [A] + twins:
        m.close()


# ---- 4: after a rollout -----------------------------------------------------------------------------------------------------------
def test_record_of_a_rollout(pkg, tables, gpu_lib):
    import torch
    dev = torch.device("cuda", 0)
    N, B = 10, 128
    A, T = (pkg.BatchedMPC(tables, N, B) for _ in range(2))
    x0 = pkg.sample_x0(tables, B, seed=21)
    d = _dirs(B, N, 8)
    for m in (A, T):
        xs = torch.from_numpy(x0).to(dev)
        torch.cuda.synchronize(dev)
        m.set_initial_guess_dev(xs.data_ptr())
        m.rollout_dev(xs.data_ptr(), 2, 50)
        m.synchronize()
    want = _passes(T, d, theta=False)
    with pytest.raises(pkg.LtompcError, match="rollout") as live:
        T.adjoint(d["gX"], d["gU"])
    rec = A.record()
    A.make_step(x0)
    with A.differentiating(rec):
        _assert_same(_passes(A, d, theta=False), want, "rollout")
        for call in (lambda: A.adjoint(d["gX"], d["gU"]), lambda: A.param_sensitivities(), lambda: A.jvp(d["dp"], d["dth"])):
            with pytest.raises(pkg.LtompcError, match="rollout"):
                call()
        with pytest.raises(pkg.LtompcError) as e:
            A.adjoint(d["gX"], d["gU"])
        assert str(e.value) == str(live.value)
        _assert_same(_passes(A, d, theta=False), want, "rollout, after the refusals")
    A.param_sensitivities()  # (the live solve is a make_step: its theta passes run)
    A.close(), T.close()


# ---- 5: friction ellipse ----------------------------------------------------------------------------------------------------------
def test_record_with_the_friction_ellipse(pkg, tables, gpu_lib):
    N, B = 10, 13
    p = pkg.default_params()
    p.ell_penalty, p.ell_rho, p.ell_D_f, p.ell_D_r = 10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0
    A, T = (pkg.BatchedMPC(tables, N, B, params=p) for _ in range(2))
    x = _two_ticks(pkg, tables, (A, T), pkg.sample_x0(tables, B, seed=21))
    want = T.sensitivities(trajectory=True)
    assert want["ok"].any()
    rec = A.record()
    A.make_step(pkg.sample_x0(tables, B, seed=77))
    with A.differentiating(rec):
        got = A.sensitivities(trajectory=True)
        with pytest.raises(pkg.LtompcError, match="ell_penalty"):
            A.param_sensitivities()
    assert all(np.array_equal(got[k], want[k]) for k in want)
    A.close(), T.close()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg, tables, gpu_lib):
    import ctypes as C
    L = gpu_lib
    N, B = 10, 13
    A, O = (pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 1)) for _ in range(2))
    x0 = pkg.sample_x0(tables, B, seed=21)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        A.record()
    A.set_initial_guess(x0)
    with pytest.raises(pkg.LtompcError, match="no solve"):
        A.record()
    x = _two_ticks(pkg, tables, (A, O), x0)
    d = _dirs(B, N, 9)
    rec, other = A.record(), O.record()
    A.make_step(x)
    A.select_record(rec)
    want = _passes(A, d)

    def refused(match, fn):
        with pytest.raises((pkg.LtompcError, ValueError), match=match):
            fn()
        _assert_same(_passes(A, d), (want[0], None), match)  # (still selected, the same bits)

    refused("this handle", lambda: A.select_record(other))
    assert L.ltompc_record_select(A._h, other._rec) != 0 and b"not a record of this handle" in L.ltompc_last_error()
    assert L.ltompc_record_release(A._h, other._rec) != 0
    spare = A.record()
    spare.release()
    refused("released", lambda: A.select_record(spare))
    assert L.ltompc_record_select(A._h, spare._rec) != 0 and b"released" in L.ltompc_last_error()
    assert L.ltompc_record_release(A._h, spare._rec) != 0 and b"released" in L.ltompc_last_error()
    refused("record is selected", lambda: A.loop_begin(3))
    A.select_record(None)
    A.loop_begin(3)
    with pytest.raises(pkg.LtompcError, match="open loop"):
        A.select_record(rec)
    keep = A.record()  # (saving is allowed inside an open loop)
    A.loop_end()
    A.select_record(rec)
    refused("record is selected", lambda: A.loop_tick(x, np.zeros((B, 2)), 50))
    refused("no table sets", lambda: A.adjoint_table_sets(d["gX"], d["gU"]))
    # per-instance table sets in effect: no record of such a solve, an earlier record still differentiates
    A.set_table_sets(np.stack([A.table_values(), A.table_values()]), np.arange(B) % 2)
    A.make_step(x)
    refused("out of scope", lambda: A.record())
    A.set_table_sets(None)
    null = C.c_void_p()
    for call in (lambda: L.ltompc_record_size(None), lambda: L.ltompc_record_save(None, C.byref(null)), lambda: L.ltompc_record_select(None, None),
                 lambda: L.ltompc_record_release(None, None), lambda: L.ltompc_record_trim(None), lambda: L.ltompc_record_stats(None, None, None)):
        assert call() < 0 and b"null handle" in L.ltompc_last_error()
    assert L.ltompc_record_save(A._h, None) != 0 and L.ltompc_record_release(A._h, None) != 0
    _assert_same(_passes(A, d), (want[0], None), "after all refusals")
    keep.release()
    A.close(), O.close()
    other.release(), rec.release()  # (no-ops once the handle is closed)


# ---- 7: free list -----------------------------------------------------------------------------------------------------------------
def test_free_list(pkg, tables, gpu_lib):
    N, B = 10, 13
    A = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 1))
    _two_ticks(pkg, tables, (A,), pkg.sample_x0(tables, B, seed=21))
    assert A.record_stats() == (0, 0) and A.record_size > 8 * 83 * N * B
    r0, r1 = A.record(), A.record()
    assert A.record_stats() == (2, 0)
    p0 = r0._rec.value
    r0.release(), r0.release()
    assert r0.released and A.record_stats() == (1, 1)
    r2 = A.record()
    assert r2._rec.value == p0 and A.record_stats() == (2, 0)  # (reused: nothing allocated)
    r1.release()
    del r2  # (dropping a record releases it)
    assert A.record_stats() == (0, 2)
    A.trim_records()
    assert A.record_stats() == (0, 0)
    r3 = A.record()
    assert A.record_stats() == (1, 0)
    with A.differentiating(r3):
        assert A.sensitivities()["ok"].any()
    A.close()
    r3.release()


# ---- 9: SplitMPC ------------------------------------------------------------------------------------------------------------------
def test_split_records_by_part(pkg, tables, gpu_lib):
    import torch
    dev = torch.device("cuda", 0)
    N, B = 10, 77
    S = pkg.SplitMPC(tables, N, B, n_parts=3, options=_opts(pkg, 2))
    T = pkg.BatchedMPC(tables, N, B, options=_opts(pkg, 2))
    x0 = pkg.sample_x0(tables, B, seed=21)
    xs, u = torch.from_numpy(x0).to(dev), torch.zeros(B, 2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    S.set_initial_guess_dev(xs.data_ptr())
    S.make_step_dev(xs.data_ptr(), u.data_ptr())
    S.synchronize()
    T.set_initial_guess(x0)
    assert np.array_equal(T.make_step(x0), u.cpu().numpy())
    d = _dirs(B, N, 10)
    want = dict(S=T.sensitivities(trajectory=True), A=T.adjoint(d["gX"], d["gU"]), J=T.jvp(d["dp"], d["dth"]))
    rec = S.record()
    assert len(rec.parts) == 3 and S.record_stats() == (3, 0) and S.record_size == sum(p.record_size for p in S.parts)
    x1 = torch.from_numpy(pkg.sample_x0(tables, B, seed=77)).to(dev)
    torch.cuda.synchronize(dev)
    S.make_step_dev(x1.data_ptr(), u.data_ptr())
    S.synchronize()
    with S.differentiating(rec):
        got = dict(S=S.sensitivities(trajectory=True), A=S.adjoint(d["gX"], d["gU"]), J=S.jvp(d["dp"], d["dth"]))
    for k in want:
        for f in want[k]:
            if f != "names":
                assert np.array_equal(got[k][f], want[k][f]), (k, f)
    rec.release()
    assert S.record_stats() == (0, 3)
    S.close(), T.close()
