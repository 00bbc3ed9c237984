"""The kernels' iterates against the oracle's, pass by pass (tests/lockstep_reference.py).

Every other comparison of the HIP solver with the oracle is made at the end of a solve, where an interior-point Newton method has
forgotten most of what a kernel can get wrong (a slightly wrong Hessian block, a wrong fraction-to-boundary or multiplier step, a
barrier update one pass late: the same KKT point, a pass or two later).  Here a solve is cut by options.max_iter = m on a fresh
handle per budget, and the whole primal-dual iterate (X, C, U, L1, L2, T, NU) with status, iters, n_reg, n_lsfail, n_resto and mu
is compared with the oracle's run at the same iteration count: within 1024 x the oracle's own rounding envelope (at least 1e-13),
discrete outputs equal, mu to 1e-12.  The rule, the alignment of passes with iterations and the exclusions are those of
lockstep_reference.check_runs; the reference of a case is made once and shared by its kernel paths.

Cases (budgets 1 .. 12, then every third up to K):
  a   N = 10, B = 16, K = 30: the reference's x0, 14 sampled states, the state that needs the restoration phase; four kernel paths
  b   N = 40, B = 16, K = 10: default path and latency_mode = 2
  c   N = 3,  B = 12, K = 18 (all converged by 16): the narrow kernels at their shortest staging round
  d   N = 10, B = 70, K = 10, latency_mode = 2: a wide launch, the batch no multiple of 8 or 64; through the narrow kernels and,
      with LTOMPC_RIC1=0 LTOMPC_STEP1=0, through k_riccati8 (70 = 8 * 8 + 6: two padding lane groups)
  e   N = 10, B = 16, K = 12: two parameter groups interleaved (set_theta: mass +-5 %, D_f 0.9 / 1.1), the _pi kernels, one oracle
      per group; latency_mode 1 and 2
  f   N = 10, B = 16, K = 12: set_guess with the oracle's cold solution, u_prev = its u0 != 0, the solve at x1 = plant(x0, u0)
  g   N = 8 and 10, B = 2, K = 30: the elastic phase - the restoration state (n_resto = 1 from k = 7) and a state off the track
      (n_resto = 1 from k = 15), n_resto equal on both sides

Each path asserts from the launch log of its largest budget that its kernel classes ran and the others did not.

Worst ratio of the scaled difference to max(env, 1e-13) measured on MI355X (limit 1024), excluded pairs, and pairs that ran out of
passes while repeating a sweep (the test prints all three):
  a narrow 2.28, a wide 2.30, a riccati1 2.28, a serial 2.28      12 of 288 excluded (two instances, from k = 14 and 15 on)   15
  b default 1.35, b mode2 1.27                                     0 of 160                                                    49
  c default 2.07                                                   0 of 168                                                     3
  d mode2 1.52, d wide 1.52                                        0 of 700                                                    33
  e mode1 1.30, e mode2 1.06                                       0 of 192                                                    11
  f default 2.43                                                   0 of 192                                                     0
  g8 default 1.06, g10 default 1.21                                0 of 36                                                   5, 2
The whole file takes about 6 s."""
import numpy as np
import pytest

import lockstep_reference as LR

pytestmark = pytest.mark.gpu

# a kernel path: options.latency_mode, the environment of the handle, and which launch classes the largest budget's solve must
# (> 0) and must not (== 0) contain - a path that fell back silently would prove nothing
NARROW = dict(mode=1, env={}, ran=("riccati1", "step1"), not_ran=("riccati", "linesearch", "pick", "update"))
WIDE = dict(mode=2, env={"LTOMPC_RIC1": "0", "LTOMPC_STEP1": "0"}, ran=("riccati", "linesearch", "update"), not_ran=("riccati1", "step1"))
RIC1 = dict(mode=0, env={"LTOMPC_RIC1Q": "0"}, ran=("riccati1", "step1"), not_ran=("riccati",))
SERIAL = dict(mode=0, env={"LTOMPC_RICCATI": "serial"}, ran=(), not_ran=("riccati1",))
DEFAULT = dict(mode=0, env={}, ran=("riccati1", "step1"), not_ran=("riccati",))
MODE2 = dict(mode=2, env={}, ran=("riccati1", "step1"), not_ran=("riccati",))

RUNS = [("a", "narrow", NARROW), ("a", "wide", WIDE), ("a", "riccati1", RIC1), ("a", "serial", SERIAL),
        ("b", "default", DEFAULT), ("b", "mode2", MODE2),
        ("c", "default", DEFAULT),
        ("d", "mode2", MODE2), ("d", "wide", WIDE),   # (wide: k_riccati8 with 70 = 8 * 8 + 6 instances, two padding lane groups)
        ("e", "mode1", NARROW), ("e", "mode2", MODE2),
        ("f", "default", DEFAULT),
        ("g8", "default", DEFAULT), ("g10", "default", DEFAULT)]


def _device_runs(pkg, tables, case, how, params=None, budgets=None):
    """{budget m: (iterate, stats)}: a fresh handle per budget, started as the case says; the launch classes of the largest
    budget's solve are checked against the path's."""
    out = {}
    for m in budgets or case.budgets:
        o = pkg.default_options()
        o.max_iter, o.latency_mode = m, how["mode"]
        mpc = pkg.BatchedMPC(tables, case.N, case.B, params=params, options=o)
        try:
            if m == case.budgets[-1]:
                mpc.set_profiling(True)
            if case.groups is not None:
                mpc.set_theta(case.theta())
            if case.guess is not None:
                G = case.guess
                mpc.set_guess(np.ones(case.B, dtype=bool), G["X"], G["U"], C=G["C"], u_prev=G["u_prev"])
            else:
                mpc.set_initial_guess(case.x0)
            mpc.make_step(case.x0)
            out[m] = (mpc.iterate(), mpc.stats())
            if m == case.budgets[-1]:
                ln = mpc.timing()["launches_by_kernel"]
                assert all(ln[c] > 0 for c in how["ran"]) and all(ln[c] == 0 for c in how["not_ran"]), (how, ln)
        finally:
            mpc.close()
    return out


@pytest.mark.parametrize("name,path,how", RUNS, ids=[f"{n}-{p}" for n, p, _ in RUNS])
def test_iterates_match_the_oracle_pass_by_pass(pkg, tables, orc, gpu_lib, monkeypatch, name, path, how):
    case = LR.cases(pkg, tables, orc)[name]
    ref = case.reference(orc, tables)
    ok, n_ex, n = LR.caps_hold(ref["excluded"], case.budgets)
    assert ok, (name, n_ex, n)   # (the reference alone; also a CPU test)
    for k, v in how["env"].items():
        monkeypatch.setenv(k, v)
    runs = _device_runs(pkg, tables, case, how)
    rep = LR.check_runs(ref, runs, label=f"case {name} path {path}")
    assert not rep["failures"], "\n".join(rep["failures"][:40])
    assert rep["excluded"] <= LR.CAP_FRACTION * rep["pairs"], rep
    if name.startswith("g"):   # the elastic phase was inside the compared window
        assert any(st["n_resto"][0] > 0 for _, st in runs.values())


def test_a_handle_with_another_mass_fails_the_comparison(pkg, tables, orc, gpu_lib):
    """The check has teeth on the device side too: a handle whose params.mass is larger by a relative 1e-8 - it converges to the
    same u0 within every other tolerance of the suite - fails for every instance of case a at each of k = 1, 2, 3."""
    case = LR.cases(pkg, tables, orc)["a"]
    p = pkg.default_params()
    p.mass *= 1.0 + 1e-8
    runs = _device_runs(pkg, tables, case, NARROW, params=p, budgets=(1, 2, 3))
    rep = LR.check_runs(case.reference(orc, tables), runs, label="case a, params.mass * (1 + 1e-8)")
    assert len(rep["failures"]) == 3 * case.B and rep["worst"] > LR.FACTOR, rep["failures"][:5]
