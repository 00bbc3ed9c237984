"""k_step1 with the instance's operands staged in LDS (csrc/linesearch.h: d_step1_stage fills a window of slots, d_linesearch
reads it through StepStage, and where one window holds the whole horizon d_update_store takes X, dX, C, dC, U, dU, T, dT from it
too): the default path of a small batch (k_riccati1q + k_step1 from the first pass) against the separate k_linesearch / k_pick /
k_update launches (LTOMPC_STEP1=0), which read the planes.  A cold and two warm closed-loop ticks; u0, status, iterations, the
recovery counters and every array of iterate() must be equal bit for bit.

Horizons: N = 2 (the shortest), 8, 40 (the benchmark's) and the two at the staging boundary of the reference's bound pattern,
derived below from the constants of linesearch.h: N = 67 is the last horizon held by ONE window, N = 68 the first that takes two
(its update reads the planes).  Batches of 3 and 12.  Variants at N = 8, the cheapest horizon at which every one of them runs
(N = 40 for LTOMPC_BOUNDS=any as well: its rows are read with run-time offsets): the run-time bound pattern, soft_rho = 100
(the elastic rows in every iteration), the friction ellipse (two more rows of T), per-instance parameters (k_step1_pi), table
sets (k_step1_ts), the first 12 states of test_gpu_pick_paths.py at their N = 10 (failed line search, shifted restart,
restoration), and LTOMPC_POISON=1 (work buffers start as NaN bit patterns) at N = 40 and N = 68."""
import numpy as np
import pytest

from test_gpu_instance_params import GROUPS, _row
from test_gpu_pick_paths import _states
from test_gpu_table_sets import _values, _variant

pytestmark = pytest.mark.gpu

TICKS = 3
# csrc/linesearch.h: STG_WORDS doubles hold eps, rho, the N partials and stage_cols columns of stage_stride words; a window is one
# column less (the nodes of its slots).  R = ni + NNL + nel rows of T; the reference's pattern has ni = 23.
STG_WORDS, SG_T = 6144, 36


def one_window(N, R):
    return N <= min((STG_WORDS - 2 - N) // (SG_T + 2 * R + 1), 128) - 1


N_LAST = max(N for N in range(2, 200) if one_window(N, 26))  # 67
N_FIRST = N_LAST + 1


def _closed_loop(pkg, tables, N, x0, options=None, params=None, setup=None):
    m = pkg.BatchedMPC(tables, N, x0.shape[0], options=options, params=params)
    try:
        if setup is not None:
            setup(m)
        m.set_profiling(True)
        m.set_initial_guess(x0)
        x, out = x0.copy(), []
        for _ in range(TICKS):
            u = m.make_step(x)
            st = m.stats()
            out.append(dict(u0=u.copy(), status=st["status"].copy(), iters=st["iters"].copy(), n_resto=st["n_resto"].copy(),
                            n_shift=st["n_shift"].copy(), it=m.iterate()))
            x = m.plant_step(x, u, 100)
        return out, m.timing()["launches_by_kernel"]
    finally:
        m.close()


def _compare(pkg, tables, monkeypatch, N, x0, **kw):
    fused, ln = _closed_loop(pkg, tables, N, x0, **kw)
    assert ln["step1"] > 0 and ln["update"] == 0, ln
    monkeypatch.setenv("LTOMPC_STEP1", "0")
    sep, ln = _closed_loop(pkg, tables, N, x0, **kw)
    monkeypatch.delenv("LTOMPC_STEP1")
    assert ln["step1"] == 0 and ln["update"] > 0, ln
    assert len(fused) == len(sep) == TICKS
    for t, (a, b) in enumerate(zip(fused, sep)):
        for key in ("u0", "status", "iters", "n_resto", "n_shift"):
            assert np.array_equal(a[key], b[key]), (N, t, key)
        for key in a["it"]:
            assert np.array_equal(a["it"][key], b["it"][key], equal_nan=True), (N, t, key)
    return fused


def test_the_boundary_is_where_the_header_says():
    assert (N_LAST, N_FIRST) == (67, 68)
    assert one_window(40, 26) and one_window(40, 28)  # the benchmark's horizon, with and without the ellipse's rows


@pytest.mark.parametrize("N,B", [(2, 3), (8, 12), (40, 3), (40, 12), (N_LAST, 12), (N_FIRST, 3), (N_FIRST, 12)])
def test_staged_step1_equals_the_separate_launches(pkg, tables, gpu_lib, monkeypatch, N, B):
    _compare(pkg, tables, monkeypatch, N, pkg.sample_x0(tables, B, seed=83))


@pytest.mark.parametrize("N", [8, 40])
def test_with_a_run_time_bound_pattern(pkg, tables, gpu_lib, monkeypatch, N):
    monkeypatch.setenv("LTOMPC_BOUNDS", "any")
    _compare(pkg, tables, monkeypatch, N, pkg.sample_x0(tables, 12, seed=83))


def test_with_soft_constraints(pkg, tables, gpu_lib, monkeypatch):
    o = pkg.default_options()
    o.soft_rho = 100.0
    _compare(pkg, tables, monkeypatch, 8, pkg.sample_x0(tables, 12, seed=83), options=o)


def test_with_the_friction_ellipse(pkg, tables, gpu_lib, monkeypatch):
    p = pkg.default_params()
    p.ell_penalty, p.ell_rho, p.ell_D_f, p.ell_D_r = 10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0
    _compare(pkg, tables, monkeypatch, 8, pkg.sample_x0(tables, 3, seed=83), params=p)


def test_with_per_instance_parameters(pkg, tables, gpu_lib, monkeypatch):
    rows = np.stack([_row(pkg, GROUPS[b % 4]) for b in range(12)])
    _compare(pkg, tables, monkeypatch, 8, pkg.sample_x0(tables, 12, seed=83), setup=lambda m: m.set_theta(rows))


def test_with_table_sets(pkg, tables, gpu_lib, monkeypatch):
    values = _values([_variant(pkg, tables, g) for g in range(4)])
    _compare(pkg, tables, monkeypatch, 8, pkg.sample_x0(tables, 12, seed=83), setup=lambda m: m.set_table_sets(values, np.arange(12) % 4))


def test_on_states_that_leave_the_common_path(pkg, tables, gpu_lib, monkeypatch):
    runs = _compare(pkg, tables, monkeypatch, 10, _states(pkg, tables)[:12])
    print("n_resto", [r["n_resto"].tolist() for r in runs], "n_shift", [r["n_shift"].tolist() for r in runs])


@pytest.mark.parametrize("N", [40, N_FIRST])
def test_with_poisoned_work_buffers(pkg, tables, gpu_lib, monkeypatch, N):
    monkeypatch.setenv("LTOMPC_POISON", "1")
    _compare(pkg, tables, monkeypatch, N, pkg.sample_x0(tables, 3, seed=83))
