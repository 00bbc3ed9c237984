"""The wave-cooperative kernels as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_harness, on the
lock-step wavefront of hip_shim.h): k_riccati8, k_riccati1, k_eval8 / k_expand8, k_pick and their _pi forms run whole
interior-point solves on the CPU, every work buffer NaN-poisoned and allocated at its exact size (k_riccati1's dynamic LDS too).
An out-of-bounds access or an undefined operation aborts the run, a collective that the lanes of a wavefront do not reach
together ends it with a message, a read of a never-written word shows up as a NaN or as a changed result.

Shapes: B = 9 (the first wavefront of k_riccati8 is full, the second holds one instance and seven padding lane groups; 55 of
the 64 slots of Bp are never written) and N in {2, 8} (2: the shortest horizon at which a stage has a successor to prefetch).
The numbers are compared with the oracle, as in test_host_harness.py, and bit for bit between the kernel paths, as the GPU suite
does (test_compaction_and_serial_riccati_do_not_change_results, test_interleaved_groups_match_uniform_handles).
The kernels whose workgroups have several wavefronts (k_riccati1q, k_step1, k_compact / k_pack*) and the rollout kernels run in
test_host_harness_multiwave.py, which imports this file's batch and helpers.
Test infrastructure only: the package never builds or loads the harness."""
import os

import numpy as np
import pytest

from test_host_harness import _run, harness  # noqa: F401  (the fixture that builds the executable)

RESTORATION_STATE = [226.623754, -0.545036120, -0.0112268024, 8.52329373, 0.122918012, 0.161888169, 0.0837443810, 0.371730909]
OFF_TRACK_STATE = [100.0, 4.0, 0.0, 10.0, 0, 0, 0, 0]
STATUS, ITERS, U0, E0 = 1, 2, slice(3, 5), 5  # columns of a printed line


@pytest.fixture(scope="module")
def batch(pkg, tables):
    """The batch of test_host_harness.py (the reference's x0, five sampled states, a state that needs the restoration phase, one
    off the track) and one more sampled state: B = 9."""
    return np.vstack([pkg.X0_REFERENCE[None], pkg.sample_x0(tables, 5, seed=61), [RESTORATION_STATE], [OFF_TRACK_STATE],
                      pkg.sample_x0(tables, 1, seed=64)])


@pytest.fixture(scope="module")
def runs(harness, tmp_path_factory, tables, batch):
    """Harness runs on the batch, each made once and shared by the tests that compare it."""
    cache = {}

    def run(N, ticks, any_bounds=0, rows=None, args=(), **options):
        key = (N, ticks, any_bounds, None if rows is None else rows.tobytes(), tuple(args), tuple(sorted(options.items())))
        if key not in cache:
            res = _run(harness, tmp_path_factory.mktemp("wave"), tables, batch, N, any_bounds=any_bounds, ticks=ticks, rows=rows, args=args, **options)
            assert len(res) == ticks and all(np.all(np.isfinite(r)) for r in res), key
            cache[key] = res
        return cache[key]
    return run


def check_against_oracle(orc_solver, res, x0, N, subset=None, min_solved=6):
    """What test_device_code_is_sanitizer_clean_and_matches_the_oracle asserts: statuses equal, u0 within 1e-6 where solved,
    iterations within 2, over closed-loop ticks that continue from the harness's own controls."""
    sel = np.arange(len(x0)) if subset is None else np.asarray(subset)
    x, ref, up = x0[sel], None, np.zeros((len(sel), 2))
    for tick, r in enumerate(res):
        r = r[sel]
        ref = orc_solver.solve(x, N, up, ref, nthreads=4, prev_status=None if ref is None else ref["status"])
        assert np.array_equal(r[:, STATUS].astype(int), ref["status"]), (tick, r[:, STATUS], ref["status"])
        both = ref["status"] == 0
        assert both.sum() >= min_solved and np.abs(r[:, U0] - ref["u0"])[both].max() < 1e-6, tick
        assert (np.abs(r[:, ITERS] - ref["iters"])[both] <= 2).all(), tick
        x, up = orc_solver.plant_step(x, r[:, U0], n_sub=100), r[:, U0]


def same_bits(a, b, cols=None):
    return all(np.array_equal(x if cols is None else x[:, cols], y if cols is None else y[:, cols]) for x, y in zip(a, b)) and len(a) == len(b)


PRINTED = [STATUS, ITERS, 3, 4, E0]


@pytest.mark.parametrize("any_bounds", [0, 1])
@pytest.mark.parametrize("N,ticks", [(8, 2), (2, 1)])
def test_wave_riccati_kernels_are_sanitizer_clean_and_match_the_oracle(runs, oracle, batch, N, ticks, any_bounds):
    """k_riccati8 over Bp / 8 waves and k_riccati1 with one wave per instance (it_index / max_sweeps as the library passes
    them), a cold tick and at N = 8 a warm one: each against the oracle, and status, iterations, u0 and E0 of the two bit for bit."""
    r8 = runs(N, ticks, any_bounds, riccati="8")
    r1 = runs(N, ticks, any_bounds, riccati="1")
    check_against_oracle(oracle, r8, batch, N)
    check_against_oracle(oracle, r1, batch, N)
    assert same_bits(r8, r1, PRINTED)
    assert same_bits(r8, runs(N, ticks, any_bounds), PRINTED)  # ... and of the serial kernel (LTOMPC_RICCATI=serial)


def test_wave_evaluation_kernels_match_the_oracle_and_the_slot_kernels(runs, oracle, batch):
    """k_eval8 / k_expand8 with k_riccati8: against the oracle, and against k_eval / k_expand by the rule of
    test_latency_mode_kernels_agree (same statuses, u0 within 1e-8 where both solved, iterations within 1)."""
    N = 8
    e8, es = runs(N, 2, riccati="8", eval="8"), runs(N, 2, riccati="8")
    check_against_oracle(oracle, e8, batch, N)
    for a, b in zip(e8, es):
        assert np.array_equal(a[:, STATUS], b[:, STATUS])
        both = a[:, STATUS] == 0
        assert both.sum() >= 6 and np.abs(a[:, U0] - b[:, U0])[both].max() < 1e-8
        assert (np.abs(a[:, ITERS] - b[:, ITERS])[both] <= 1).all()


@pytest.mark.parametrize("riccati", ["8", "1"])
def test_compacted_instance_list_does_not_change_a_bit(runs, riccati):
    """compact=1: after every iteration the list is the stable compaction of the unfinished instances (k_compact's result), so
    lane groups work on instances other than their own index and the launch ends in padding groups: every printed value
    bit-identical to the identity-list run."""
    assert same_bits(runs(8, 2, riccati=riccati, compact=1), runs(8, 2, riccati=riccati))


def test_soft_constraints_through_the_wave_riccati_kernel(harness, tmp_path, orc, pkg, tables):
    """The elastic planes (options.soft_rho = 100) through k_riccati8: the small case of test_host_harness.py."""
    N = 6
    x0 = pkg.sample_x0(tables, 4, seed=62)
    res = _run(harness, tmp_path, tables, x0, N, soft_rho=100.0, ticks=1, riccati="8")
    o = orc.default_options(); o.soft_rho = 100.0
    ref = orc.Oracle(tables.packed(), options=o).solve(x0, N, nthreads=4)
    assert np.all(np.isfinite(res[0])) and np.array_equal(res[0][:, STATUS].astype(int), ref["status"])
    assert np.abs(res[0][:, U0] - ref["u0"]).max() < 1e-6


def test_friction_ellipse_through_the_wave_riccati_kernel(harness, tmp_path, orc, pkg, tables):
    """The friction-ellipse constraints through k_riccati8: the small case of test_host_harness.py."""
    N = 6
    x0 = pkg.sample_x0(tables, 4, seed=63)
    ell = (10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0)
    res = _run(harness, tmp_path, tables, x0, N, ticks=1, ell=ell, riccati="8")
    p = orc.default_params(); p.ell_penalty, p.ell_rho, p.ell_D_f, p.ell_D_r = ell
    ref = orc.Oracle(tables.packed(), params=p).solve(x0, N, nthreads=4)
    assert np.all(np.isfinite(res[0])) and np.array_equal(res[0][:, STATUS].astype(int), ref["status"])
    ok = ref["status"] == 0
    assert ok.sum() >= 3 and np.abs(res[0][:, U0] - ref["u0"])[ok].max() < 1e-6


# theta_a = defaults with D_f = D_r = 0.9, mass = 1100; theta_b = defaults with q_n = 1.0, r_du = (0.02, 0.005)
THETA_A = {"D_f": 0.9, "D_r": 0.9, "mass": 1100.0}
THETA_B = {"q_n": 1.0, "r_du0": 0.02, "r_du1": 0.005}


def theta_rows(pkg, B):
    """(B, 16) rows, theta_a on the even and theta_b on the odd instances; and the two index sets."""
    p = pkg.default_params()
    names = list(pkg.THETA_NAMES)
    base = np.array([getattr(p, n) for n in names[:-2]] + [p.r_du[0], p.r_du[1]])
    rows = np.tile(base, (B, 1))
    col = lambda k: {"r_du0": 14, "r_du1": 15}.get(k, names.index(k) if k in names else -1)
    for k, v in THETA_A.items():
        rows[0::2, col(k)] = v
    for k, v in THETA_B.items():
        rows[1::2, col(k)] = v
    return rows, np.arange(0, B, 2), np.arange(1, B, 2)


def oracle_params(orc, theta):
    p = orc.default_params()
    for k, v in theta.items():
        if k.startswith("r_du"):
            p.r_du[int(k[-1])] = v
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("riccati,evl", [("8", "slot"), ("1", "8")])
def test_per_instance_rows_match_uniform_runs_bit_for_bit(runs, orc, pkg, tables, batch, riccati, evl):
    """Two rows interleaved over the nine instances, through k_theta_rows, WorkPI and the _pi kernels (k_init_pi, k_eval_pi or
    k_eval8_pi / k_expand8_pi, k_riccati8_pi or k_riccati1_pi, k_linesearch_pi, k_pick_pi, k_plant_pi): every instance's line
    bit-identical to its line in the uniform run made with its row (param.<field>=<value>, the uniform kernels), and each row's
    subset against the oracle created with those params."""
    N = 8
    rows, ia, ib = theta_rows(pkg, len(batch))
    mixed = runs(N, 2, rows=rows, riccati=riccati, eval=evl)
    for theta, idx in ((THETA_A, ia), (THETA_B, ib)):
        uni = runs(N, 2, args=tuple(f"param.{k}={v!r}" for k, v in theta.items()), riccati=riccati, eval=evl)
        for a, b in zip(mixed, uni):
            assert np.array_equal(a[idx], b[idx]), (theta, a[idx], b[idx])
        check_against_oracle(orc.Oracle(tables.packed(), params=oracle_params(orc, theta)), mixed, batch, N, subset=idx, min_solved=3)


# ---------------------------------------------------------------------------------------------------- the derivative passes
class HarnessSolve:
    """What the comparison functions of the GPU tests read from a BatchedMPC (stats, iterate, solved_parameters, B, N, options
    and the passes' outputs), served from one tick of the harness's dump file (derivs=1)."""

    def __init__(self, pkg, rec, cot, B, N):
        self.B, self.N, self.options = B, N, pkg.default_options()
        self._rec, self._cot = rec, cot

    def stats(self):
        r = self._rec
        return dict(status=r["status"].astype(int), status_solver=r["status_solver"].astype(int), mu=r["mu"])

    def iterate(self):
        return {k: self._rec[k] for k in ("X", "C", "U", "L1", "L2", "T", "NU")}

    def solved_parameters(self):
        return self._rec["x0"], self._rec["uprev"], self._rec["u0"]

    def sensitivities(self, trajectory=False):
        r = self._rec
        return dict(du0_dx0=r["s_du0"][:, :, :8].copy(), du0_duprev=r["s_du0"][:, :, 8:].copy(), ok=r["ok"] != 0, margin=r["margin"],
                    dX=r["s_dX"], dU=r["s_dU"])

    def param_sensitivities(self, trajectory=False):
        r = self._rec
        return dict(du0_dtheta=r["p_du0"], ok=r["ok"] != 0, dX=r["p_dX"], dU=r["p_dU"])

    def adjoint(self, gX=None, gU=None, theta=True):
        for c, (cX, cU) in enumerate(self._cot):  # one of the cotangents the harness has swept
            if np.array_equal(cX, gX) and np.array_equal(cU, gU):
                gp, gth = self._rec["adj"][c]
                return dict(grad_x0=gp[:, :8].copy(), grad_uprev=gp[:, 8:].copy(), grad_theta=gth, ok=self._rec["ok"] != 0)
        raise KeyError("a cotangent that was not in the problem file")


def read_dump(path, B, N, ni, ticks, n_cot, loop):
    d = np.fromfile(path)
    pos, out = 0, []

    def take(*shape):
        nonlocal pos
        n = int(np.prod(shape))
        v = d[pos:pos + n].reshape(shape)
        pos += n
        return v
    for _ in range(ticks):
        r = dict(X=take(B, N + 1, 8), C=take(B, N, 8), U=take(B, N, 2), L1=take(B, N, 8), L2=take(B, N, 8), T=take(B, N, ni), NU=take(B, N, ni),
                 x0=take(B, 8), uprev=take(B, 2), u0=take(B, 2), status=take(B), status_solver=take(B), mu=take(B),
                 s_du0=take(B, 2, 10), ok=take(B), margin=take(B), s_dX=take(B, N + 1, 8, 10), s_dU=take(B, N, 2, 10),
                 p_du0=take(B, 2, 16), p_dX=take(B, N + 1, 8, 16), p_dU=take(B, N, 2, 16))
        r["adj"] = [(take(B, 10), take(B, 16)) for _ in range(n_cot)]
        if loop:
            r["phi"] = dict(dx=take(B, 8, 8), du=take(B, 8, 2), dtheta=take(B, 8, 16))
            r["loop"] = dict(dx=take(B, 8, 24), du=take(B, 2, 24), ok=take(B) != 0, ticks=take(B).astype(int))
        out.append(r)
    assert pos == d.size, (pos, d.size)
    return out


ADJ_SEED = 7


def derivative_cotangents(B, N):
    """A seeded dense cotangent (check_against_forward) and check_against_dense's three one-hot placements."""
    from test_gpu_adjoint import _cotangent, _one_hot, _places
    return [_cotangent(B, N, ADJ_SEED)] + [_one_hot(B, N, w) for w in _places(B, N, ADJ_SEED)]


def run_derivs(harness, tmp_path, pkg, tables, batch, N, evl, cot, name, ticks=2, loop=0, rows=None, args=()):
    dump = tmp_path / f"{name}.bin"
    opts = dict(loop=loop) if loop else {}
    res = _run(harness, tmp_path, tables, batch, N, ticks=ticks, cot=cot, rows=rows, args=args, riccati="8", eval=evl, derivs=1, dump=str(dump), **opts)
    assert len(res) == ticks and all(np.all(np.isfinite(r)) for r in res)
    ni = len(__import__("sens_reference").bound_rows(pkg.default_params())) + 3
    recs = read_dump(dump, len(batch), N, ni, ticks, len(cot), loop=bool(loop))
    for t, rec in enumerate(recs):
        for k, v in rec.items():
            for a in ([x for pair in v for x in pair] if k == "adj" else v.values() if isinstance(v, dict) else [v]):
                assert np.all(np.isfinite(a)), (name, t, k)
    return res, recs


def outputs_zero_where_not_ok(rec):
    ok = rec["ok"] != 0
    keys = ("s_du0", "margin", "s_dX", "s_dU", "p_du0", "p_dX", "p_dU")
    return all((rec[k][~ok] == 0).all() for k in keys) and all((gp[~ok] == 0).all() and (gth[~ok] == 0).all() for gp, gth in rec["adj"])


@pytest.mark.parametrize("N,evl", [(2, "slot"), (2, "8"), (8, "slot"), (8, "8")])
def test_derivative_passes_under_sanitizers_match_the_dense_references(harness, tmp_path, pkg, tables, batch, N, evl):
    """derivs=1 over two ticks (a cold solve, then a warm one with u_prev != 0): k_sens_eval or k_sens_eval8, k_sens_riccati8,
    k_sens_forward (both calls), k_psens_cond, k_psens_sweep with trajectories and k_adj_sweep with theta for four cotangents -
    the pass's private QP / RC / RS / LS and the PV, KF, AJ planes NaN-poisoned and at their exact sizes.  The dumped iterate and
    outputs go through the comparison code of the GPU tests, with their constants: ok against the reference's inertia verdict
    outside BAND, every entry within CAP / MEDIAN_CAP / FWD_BOUND, and exactly 0 where ok = 0."""
    import test_gpu_adjoint as TA
    import test_gpu_param_sensitivity as TP
    import test_gpu_sensitivity_dense as TS
    B = len(batch)
    cot = derivative_cotangents(B, N)
    _, recs = run_derivs(harness, tmp_path, pkg, tables, batch, N, evl, cot, "uniform")
    assert np.abs(recs[1]["uprev"]).max() > 0
    for t, rec in enumerate(recs):
        assert outputs_zero_where_not_ok(rec)
        mpc = HarnessSolve(pkg, rec, cot, B, N)
        S, P = mpc.sensitivities(True), mpc.param_sensitivities(True)
        label = f"harness_N{N}_{evl}_t{t}"
        assert len(TS.check_against_reference(pkg, tables, mpc, S, label)) >= 6, label
        assert len(TP.check_against_reference(pkg, tables, mpc, P, label)) >= 6, label
        TA.check_against_forward(mpc, mpc.adjoint(*cot[0]), cot[0][0], cot[0][1], label, S=S, P=P)
        TA.check_against_dense(pkg, tables, mpc, label, ADJ_SEED)


@pytest.mark.parametrize("N,evl", [(2, "8"), (8, "slot")])
def test_derivative_passes_with_per_instance_rows_match_uniform_runs(harness, tmp_path, pkg, tables, batch, N, evl):
    """The _pi forms of the passes (k_sens_eval_pi or k_sens_eval8_pi, k_sens_riccati8_pi, k_psens_cond_pi, k_psens_sweep_pi,
    k_adj_sweep_pi; TH through Wspi) with the two interleaved rows.  The dense references model the default vehicle and cost only,
    so each instance's record is compared bit for bit with the uniform run made with its row (the claim of
    test_interleaved_groups_match_uniform_handles), and the adjoint with the handle's own forward mode within FWD_BOUND."""
    import test_gpu_adjoint as TA
    B = len(batch)
    cot = derivative_cotangents(B, N)[:1]
    rows, ia, ib = theta_rows(pkg, B)
    _, mixed = run_derivs(harness, tmp_path, pkg, tables, batch, N, evl, cot, "rows", rows=rows)
    for theta, idx in ((THETA_A, ia), (THETA_B, ib)):
        _, uni = run_derivs(harness, tmp_path, pkg, tables, batch, N, evl, cot, "uni", args=tuple(f"param.{k}={v!r}" for k, v in theta.items()))
        for t, (a, b) in enumerate(zip(mixed, uni)):
            for k in a:
                if k == "adj":
                    assert all(np.array_equal(x[idx], y[idx]) for pa, pb in zip(a[k], b[k]) for x, y in zip(pa, pb)), (t, k)
                else:
                    assert np.array_equal(a[k][idx], b[k][idx]), (t, k)
    for t, rec in enumerate(mixed):
        assert outputs_zero_where_not_ok(rec) and (rec["ok"] != 0).sum() >= 6
        mpc = HarnessSolve(pkg, rec, cot, B, N)
        TA.check_against_forward(mpc, mpc.adjoint(*cot[0]), cot[0][0], cot[0][1], f"harness_rows_N{N}_{evl}_t{t}")


# ---------------------------------------------------------------------------------------------------- plant step and closed loop
@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("n_sub", [1, 4])
def test_plant_step_sensitivities_under_sanitizers(harness, tmp_path, orc, pkg, tables, batch, n_sub, with_rows):
    """plant_sens=<n_sub>: k_plant_sens (k_plant_sens_pi with the interleaved rows) into a NaN-poisoned plane set of its exact
    size, k_planes_rows, against plant_sens_reference within the GPU test's PLANT_TOL; the cost columns exactly 0; x_next is
    k_plant's own line (the library returns that one) and agrees with the oracle's plant step."""
    import plant_sens_reference as PSR
    from test_gpu_loop_sensitivity import PLANT_TOL
    B = len(batch)
    u = np.random.default_rng(1031 + n_sub).uniform(-1.0, 1.0, size=(B, 2)) * np.array([0.5, 1.0])
    rows = theta_rows(pkg, B)[0] if with_rows else None
    res = _run(harness, tmp_path, tables, batch, 2, ticks=1, u=u, rows=rows, riccati="8", plant_sens=n_sub)
    r = res[0]
    assert r.shape == (B, 8 + 64 + 16 + 128) and np.all(np.isfinite(r))
    got = dict(x_next=r[:, :8], dx=r[:, 8:72].reshape(B, 8, 8), du=r[:, 72:88].reshape(B, 8, 2), dtheta=r[:, 88:].reshape(B, 8, 16))
    ref = PSR.plant_sensitivities(batch, u, tables, n_sub=n_sub) if rows is None else PSR.plant_sensitivities(batch, u, tables, theta=rows, n_sub=n_sub)
    assert np.all(got["dtheta"][:, :, list(pkg.THETA_NAMES).index("q_n"):] == 0.0)
    for k in ("dx", "du", "dtheta"):
        err = np.abs(got[k] - ref[k]).max(axis=(1, 2)) / np.abs(ref[k]).max(axis=(1, 2))
        print(f"harness plant n_sub={n_sub} rows={with_rows} {k}: max error / max|ref| = {err.max():.3e}")
        assert err.max() <= PLANT_TOL, (k, err.max(), PLANT_TOL)
    if rows is None:
        assert np.abs(got["x_next"] - orc.Oracle(tables.packed()).plant_step(batch, u, n_sub=n_sub)).max() < 1e-12


def test_closed_loop_accumulation_under_sanitizers(harness, tmp_path, pkg, tables, batch):
    """loop=3 with derivs=1 over two ticks: k_loop_begin, then per tick k_plant_sens at (x_t, u0_t) and k_loop_accum on the
    passes' du0 outputs, against the float64 recursion _host_tick of the GPU test from the dumped outputs, within its ACCUM_TOL."""
    from test_gpu_loop_sensitivity import ACCUM_TOL, _host_tick
    B, N, mode = len(batch), 8, 3
    _, recs = run_derivs(harness, tmp_path, pkg, tables, batch, N, "slot", [], "loop", loop=mode)
    eye = np.concatenate([np.eye(8), np.zeros((8, 16))], axis=1)
    Sx, Du, alive = np.tile(eye, (B, 1, 1)), np.zeros((B, 2, 24)), np.ones(B, dtype=bool)
    for t, rec in enumerate(recs):
        S = dict(du0_dx0=rec["s_du0"][:, :, :8], du0_duprev=rec["s_du0"][:, :, 8:], ok=rec["ok"] != 0)
        Sx, Du, alive = _host_tick(Sx, Du, alive, S, dict(du0_dtheta=rec["p_du0"]), rec["phi"], mode)
        L = rec["loop"]
        assert np.array_equal(L["ok"], alive)
        scale = np.abs(Sx).max(axis=(1, 2))
        scale[~alive] = 1.0
        err = np.maximum(np.abs(L["dx"] - Sx).max(axis=(1, 2)), np.abs(L["du"] - Du).max(axis=(1, 2))) / scale
        print(f"harness accumulator T={t + 1}: max error / max|Sx| = {err.max():.3e}, alive {alive.sum()}/{B}")
        assert err.max() <= ACCUM_TOL, (t, err.max(), ACCUM_TOL)
        assert np.all(L["dx"][~alive] == 0.0) and np.all(L["du"][~alive] == 0.0) and np.all(L["ticks"][alive] == t + 1)
    assert alive.sum() >= 6


# ---------------------------------------------------------------------------------------------------- slip forces and the ellipse
def test_slip_forces_under_sanitizers_match_the_oracle(harness, tmp_path, oracle, tables, batch):
    """slip=1: k_slip_forces at the harness batch against the oracle (the bounds of test_gpu_parity.py against the recorded
    values: slip angles 1e-14, forces 1e-9)."""
    r = _run(harness, tmp_path, tables, batch, 2, ticks=1, slip=1)[0]
    a, F = oracle.slip_forces(batch)
    assert r.shape == (len(batch), 4) and np.all(np.isfinite(r))
    assert np.abs(r[:, :2] - a).max() < 1e-14 and np.abs(r[:, 2:] - F).max() < 1e-9


def test_friction_ellipse_derivatives_under_sanitizers_match_the_oracle(harness, tmp_path, orc, tables, batch):
    """ellipse=1: k_test_ellipse at the harness batch (steering and throttle spread over their ranges) against the oracle's AD, at
    the bounds of the GPU test of the ellipse."""
    ell = (10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0)
    x = batch.copy()
    x[:, 6], x[:, 7] = np.random.default_rng(2).uniform(-0.5, 0.5, len(x)), np.random.default_rng(3).uniform(-1, 1, len(x))
    r = _run(harness, tmp_path, tables, x, 2, ticks=1, ell=ell, ellipse=1)[0]
    assert r.shape == (len(x), 2 + 16 + 128) and np.all(np.isfinite(r))
    po = orc.default_params(); po.ell_penalty, po.ell_rho, po.ell_D_f, po.ell_D_r = ell
    oracle = orc.Oracle(tables.packed(), params=po)
    for i in range(len(x)):
        vo, go, Ho = oracle.ell_derivs(x[i])
        v, g, H = r[i, :2], r[i, 2:18].reshape(2, 8), r[i, 18:].reshape(2, 8, 8)
        assert np.abs(v - vo).max() <= 1e-12 * (1 + np.abs(vo).max())
        assert np.abs(g - go).max() <= 1e-11 * (1 + np.abs(go).max())
        assert np.abs(H - Ho).max() <= 1e-10 * (1 + np.abs(Ho).max())


# ---------------------------------------------------------------------------------------------------- velocity profile
def test_velocity_profile_kernel_under_sanitizers(harness, tmp_path, orc):
    """k_velocity_profile on exact-size inputs and NaN-poisoned outputs: the closed and the open case of the fixture against
    tests/golden/velocity_profiles.npz with the tolerance of test_gpu_velocity_profile_matches_reference_and_oracle, and a batch
    of two profiles (one closed, one open with s_max < 0, different curvature) and a shorter open path bit for bit against the
    oracle's velocity_profile, as that test compares its batch.  (The kernel takes one length per launch: profiles of different
    length are launches of their own.)"""
    import subprocess
    from test_velocity_profile import FIELDS, FX, _cases, _close, _vehicles
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rng = np.random.default_rng(5)
    s2 = np.tile(FX["s"], (2, 1))
    k2 = FX["k"][None] * rng.uniform(0.5, 2.0, (2, 1)) + rng.uniform(0, 0.01, (2, len(FX["s"])))
    sm2 = np.array([float(FX["s_max"]), -1.0])
    s3, k3, sm3 = FX["s"][None, :117].copy(), k2[1:, :117].copy(), np.array([-1.0])
    launches = [(s[None], k[None], np.array([sm])) for s, k, sm in _cases().values()] + [(s2, k2, sm2), (s3, k3, sm3)]
    for name, V in _vehicles(orc).items():
        prob = tmp_path / f"velocity_{name}.txt"
        with open(prob, "w") as f:
            f.write(" ".join(repr(v) for v in (V.kind, V.n_map, V.mass, V.friction_coef, V.lam, V.D, V.T, V.C_m, V.Cr_0, V.Cr_2)) + "\n")
            f.write(" ".join(repr(float(v)) for v in list(V.map_v) + list(V.map_f)) + f"\n{len(launches)}\n")
            for s, k, sm in launches:
                f.write(f"{s.shape[1]} {s.shape[0]}\n")
                for a in (s, k, sm):
                    np.savetxt(f, a.ravel()[None], fmt="%.17g")
        out = subprocess.run([harness, str(prob), "velocity"], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
        blocks = [b.strip().splitlines()[1:] for b in out.stdout.split("tick")[1:]]
        assert len(blocks) == len(launches)
        for li, ((s, k, sm), lines) in enumerate(zip(launches, blocks)):
            got = np.array([[float(v) for v in ln.split()] for ln in lines]).reshape(s.shape[0], 4, s.shape[1])
            assert np.all(np.isfinite(got)), (name, li)
            if li < 2:
                tag = list(_cases())[li]
                for fi, fld in enumerate(FIELDS):
                    assert _close(got[0, fi], FX[f"{name}_{tag}_{fld}"]), (name, tag, fld)
            ref = orc.velocity_profile(V, s, k, sm)
            for fi, fld in enumerate(FIELDS):
                assert np.array_equal(got[:, fi], ref[fi]), (name, li, fld, np.abs(got[:, fi] - ref[fi]).max())
