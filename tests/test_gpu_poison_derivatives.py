"""The derivative passes with NaN-poisoned work planes: the sibling of test_poisoned_work_buffers_give_identical_results
(test_gpu_parity.py), which runs make_step, stats, prediction and iterate only.  The sensitivity, parameter-sensitivity, adjoint,
plant-step and closed-loop passes allocate planes of their own as work buffers (the private QP / RC / RS / LS of the sensitivity
pass, PV, KF, AJ, PSN); with LTOMPC_POISON=1 those start as NaN bit patterns instead of zeros, and a read of a word that no kernel
has written shows as a changed or non-finite result.  Every array the passes return must be bit-identical between the two
settings.  Nothing is provoked: a poisoned plane is an ordinary NaN input to ordinary arithmetic."""
import numpy as np
import pytest

from test_gpu_parity import STALL_STATES

pytestmark = pytest.mark.gpu


def interleaved_rows(pkg, theta0, B):
    """Two rows over the instances, a b a b ...: theta_a = defaults with D_f = D_r = 0.9, mass = 1100; theta_b = defaults with
    q_n = 1.0, r_du = (0.02, 0.005)."""
    names = list(pkg.THETA_NAMES)
    a, b = theta0.copy(), theta0.copy()
    a[names.index("D_f")] = a[names.index("D_r")] = 0.9
    a[names.index("mass")] = 1100.0
    b[names.index("q_n")] = 1.0
    b[len(names) - 2], b[len(names) - 1] = 0.02, 0.005
    return np.where((np.arange(B) % 2 == 0)[:, None], a[None], b[None])


def _passes(pkg, tables, B, N, mode, rows, x0):
    o = pkg.default_options()
    o.latency_mode = mode
    m = pkg.BatchedMPC(tables, N, B, options=o)
    if rows:
        m.set_theta(interleaved_rows(pkg, m.theta(), B))
    m.set_initial_guess(x0)
    u1 = m.make_step(x0)
    x1 = m.plant_step(x0, u1, 50)
    u2 = m.make_step(x1)
    out, ok_of = {"u1": u1, "u2": u2}, {}
    S = m.sensitivities(trajectory=True)
    P = m.param_sensitivities(trajectory=True)
    rng = np.random.default_rng(5)
    A = m.adjoint(rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2)), theta=True)
    assert "grad_theta" in A
    for name, d in (("sens", S), ("psens", P), ("adj", A)):
        for k, v in d.items():
            if k != "names":
                out[f"{name}.{k}"], ok_of[f"{name}.{k}"] = v, d["ok"]
    for k, v in m.plant_sensitivities(x1, u2, n_sub=4).items():
        if k != "names":
            out[f"plant.{k}"] = v
    m.loop_begin(3)
    x = x1
    for _ in range(2):
        u = m.make_step(x)
        x = m.loop_tick(x, u, n_sub=4)
    L = m.loop_sensitivities()
    out["loop.x"] = x
    for k, v in L.items():
        if k != "names":
            out[f"loop.{k}"], ok_of[f"loop.{k}"] = v, L["ok"]
    m.close()
    return out, ok_of


@pytest.mark.parametrize("B,N,mode,rows", [(13, 2, 1, False), (61, 10, 2, False), (13, 10, 1, True), (61, 2, 2, True)])
def test_poisoned_work_planes_do_not_change_the_derivative_passes(pkg, tables, gpu_lib, monkeypatch, B, N, mode, rows):
    """(B, N, latency_mode, per-instance rows): a cold make_step, a plant step and a warm make_step (u_prev != 0) with one
    instance that goes through the restoration phase in slot 0; then sensitivities and param_sensitivities with trajectories,
    an adjoint sweep with theta for a seeded cotangent, plant_sensitivities(n_sub=4) and a two-tick loop in mode 3."""
    x0 = pkg.sample_x0(tables, B, seed=31)
    x0[0] = STALL_STATES[20][0]
    res = []
    for poison in ("0", "1"):
        monkeypatch.setenv("LTOMPC_POISON", poison)
        res.append(_passes(pkg, tables, B, N, mode, rows, x0))
    monkeypatch.delenv("LTOMPC_POISON")
    (clean, _), (poisoned, ok_of) = res
    assert clean.keys() == poisoned.keys()
    for k in clean:
        assert np.array_equal(clean[k], poisoned[k], equal_nan=False), k
    for k, v in poisoned.items():
        ok = ok_of.get(k)
        if ok is None:
            assert np.all(np.isfinite(v)), k
        else:
            assert np.all(np.isfinite(np.asarray(v, dtype=float)[ok])), k
    assert poisoned["sens.ok"].sum() >= B // 2 and poisoned["loop.ok"].sum() >= B // 2  # (the passes did run on most instances)
