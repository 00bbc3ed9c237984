"""k_step1's split update on the GPU (csrc/linesearch.h: d_update_fetch on wavefronts 1..4 while d_pick runs, d_update_store after
the second barrier): the default path of a batch of 12 (k_riccati1q + k_step1 from the first pass) against the separate
k_linesearch / k_pick / k_update launches (LTOMPC_STEP1=0), which run d_update itself.  A cold and two warm closed-loop ticks;
u0, status, iterations, the recovery counters and every array of iterate() must be equal bit for bit.

N = 10 (one round of fetched slots, partly filled), 41 (the candidate loop wraps, the second round holds slots 32..40) and 79
(slots 64..78 are loaded after the barrier); soft_rho = 100 (the elastic pairs in every iteration) at N = 10; the first 12 states
of test_gpu_pick_paths.py (failed line searches, shifted restart / restoration phase) at their N = 10."""
import numpy as np
import pytest

from test_gpu_pick_paths import _states

pytestmark = pytest.mark.gpu

B, TICKS = 12, 3


def _closed_loop(pkg, tables, N, x0, soft_rho=0.0):
    o = pkg.default_options()
    o.soft_rho = soft_rho
    m = pkg.BatchedMPC(tables, N, B, options=o)
    try:
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


def _compare(pkg, tables, monkeypatch, N, x0, soft_rho=0.0):
    fused, ln = _closed_loop(pkg, tables, N, x0, soft_rho)
    assert ln["step1"] > 0 and ln["update"] == 0, ln
    monkeypatch.setenv("LTOMPC_STEP1", "0")
    sep, ln = _closed_loop(pkg, tables, N, x0, soft_rho)
    assert ln["step1"] == 0 and ln["update"] > 0, ln
    assert len(fused) == len(sep) == TICKS
    for t, (a, b) in enumerate(zip(fused, sep)):
        for key in ("u0", "status", "iters", "n_resto", "n_shift"):
            assert np.array_equal(a[key], b[key]), (N, t, key)
        for key in a["it"]:
            assert np.array_equal(a["it"][key], b["it"][key], equal_nan=True), (N, t, key)
    return fused


@pytest.mark.parametrize("N", [10, 41, 79])
def test_split_update_equals_the_separate_launches(pkg, tables, gpu_lib, monkeypatch, N):
    _compare(pkg, tables, monkeypatch, N, pkg.sample_x0(tables, B, seed=83))


def test_split_update_with_soft_constraints(pkg, tables, gpu_lib, monkeypatch):
    _compare(pkg, tables, monkeypatch, 10, pkg.sample_x0(tables, B, seed=83), soft_rho=100.0)


def test_split_update_on_states_that_leave_the_common_path(pkg, tables, gpu_lib, monkeypatch):
    runs = _compare(pkg, tables, monkeypatch, 10, _states(pkg, tables)[:12])
    print("n_resto", [r["n_resto"].tolist() for r in runs], "n_shift", [r["n_shift"].tolist() for r in runs])
