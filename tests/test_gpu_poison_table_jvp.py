"""The directional pass in the track tables with NaN-poisoned work planes (the sibling of test_gpu_poison_jvp.py for
ltompc_get_jvp_tables): its stage-vector planes and its kff planes are allocated as work buffers, so with LTOMPC_POISON=1 they
start as NaN bit patterns, as do the private stage / Riccati buffers it shares; a read of a word no kernel has written shows as a
changed or non-finite result.  Nothing is provoked: a poisoned plane is an ordinary NaN input to ordinary arithmetic."""
import numpy as np
import pytest

from test_gpu_poison_derivatives import interleaved_rows

pytestmark = pytest.mark.gpu


def _pass(pkg, tables, B, N, mode, rows, x0):
    o = pkg.default_options()
    o.latency_mode = mode
    m = pkg.BatchedMPC(tables, N, B, options=o)
    if rows:
        m.set_theta(interleaved_rows(pkg, m.theta(), B))
    m.set_initial_guess(x0)
    u1 = m.make_step(x0)
    m.make_step(m.plant_step(x0, u1, 50))  # (warm: u_prev != 0)
    rng = np.random.default_rng(6)
    y = np.stack([tables.kappa, tables.n_left, tables.n_right, tables.v_ref])
    dp, dy = rng.standard_normal((B, 10)), 0.01 * np.abs(y).max(axis=1, keepdims=True) * rng.standard_normal(y.shape)
    ds = rng.standard_normal((B, N, 10)) * 1e-3
    out = {}
    for name, J in (("all", m.jvp_tables(dp, dy, ds)), ("tables", m.jvp_tables(dtables=dy)), ("slot", m.jvp_tables(dslot=ds)),
                    ("dp", m.jvp_tables(dp=dp))):  # (the pass first: it makes everything itself)
        out.update({f"{name}.{k}": v for k, v in J.items()})
    m.close()
    return out


@pytest.mark.parametrize("B,N,mode,rows", [(13, 2, 1, False), (61, 10, 2, True)])
def test_poisoned_work_planes_do_not_change_the_table_direction_pass(pkg, tables, gpu_lib, monkeypatch, B, N, mode, rows):
    x0 = pkg.sample_x0(tables, B, seed=31)
    res = []
    for poison in ("0", "1"):
        monkeypatch.setenv("LTOMPC_POISON", poison)
        res.append(_pass(pkg, tables, B, N, mode, rows, x0))
    monkeypatch.delenv("LTOMPC_POISON")
    clean, poisoned = res
    for k in clean:
        assert np.array_equal(clean[k], poisoned[k], equal_nan=False), k
        assert np.all(np.isfinite(np.asarray(poisoned[k], dtype=float))), k  # (instances with ok = 0 are exact zeros)
    assert poisoned["all.ok"].sum() >= B // 2
