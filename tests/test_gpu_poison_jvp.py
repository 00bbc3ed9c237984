"""The directional pass with NaN-poisoned work planes (the sibling of test_gpu_poison_derivatives.py for ltompc_get_jvp): its kff
planes are allocated as a work buffer, so with LTOMPC_POISON=1 they start as NaN bit patterns, as do the PV planes and the private
stage / Riccati buffers it shares; a read of a word no kernel has written shows as a changed or non-finite result.  Nothing is
provoked: a poisoned plane is an ordinary NaN input to ordinary arithmetic."""
import numpy as np
import pytest

from test_gpu_poison_derivatives import interleaved_rows

pytestmark = pytest.mark.gpu


def _jvp(pkg, tables, B, N, mode, rows, x0):
    o = pkg.default_options()
    o.latency_mode = mode
    m = pkg.BatchedMPC(tables, N, B, options=o)
    if rows:
        m.set_theta(interleaved_rows(pkg, m.theta(), B))
    m.set_initial_guess(x0)
    u1 = m.make_step(x0)
    m.make_step(m.plant_step(x0, u1, 50))  # (warm: u_prev != 0)
    rng = np.random.default_rng(6)
    dp, dth = rng.standard_normal((B, 10)), rng.uniform(-0.05, 0.05, (B, 16)) * m.theta()
    out = {}
    for name, J in (("both", m.jvp(dp, dth)), ("dp", m.jvp(dp, None)), ("dth", m.jvp(None, dth))):  # (the pass first: it makes everything itself)
        out.update({f"{name}.{k}": v for k, v in J.items()})
    m.close()
    return out


@pytest.mark.parametrize("B,N,mode,rows", [(13, 2, 1, False), (61, 10, 2, True)])
def test_poisoned_work_planes_do_not_change_the_directional_pass(pkg, tables, gpu_lib, monkeypatch, B, N, mode, rows):
    x0 = pkg.sample_x0(tables, B, seed=31)
    res = []
    for poison in ("0", "1"):
        monkeypatch.setenv("LTOMPC_POISON", poison)
        res.append(_jvp(pkg, tables, B, N, mode, rows, x0))
    monkeypatch.delenv("LTOMPC_POISON")
    clean, poisoned = res
    for k in clean:
        assert np.array_equal(clean[k], poisoned[k], equal_nan=False), k
        assert np.all(np.isfinite(np.asarray(poisoned[k], dtype=float))), k  # (instances with ok = 0 are exact zeros)
    assert poisoned["both.ok"].sum() >= B // 2
