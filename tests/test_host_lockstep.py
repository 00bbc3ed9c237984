"""The lock-step comparison of tests/lockstep_reference.py on a machine without a GPU: the device code as host C++ under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_harness, as it is, through test_host_harness._run with the max_iter
option it already takes) against the oracle at the same budget.

Batch: that of test_host_harness_wave.py (B = 9: the reference's x0, sampled states, the restoration state, one off the track), N = 8,
one cold solve per budget k in {1, 2, 3, 5, 8, 13}, through k_riccati8 and through k_riccati1.  The harness prints status, iters,
u0 (= U_0 of the iterate) and E0 per instance; by the rule of DESIGN.md §6 (instance b against the oracle run at max_iter =
iters[b]; pairs the reference excludes left out) status and iters are equal, n_resto too, u0 is within 1024 x max(env, 1e-13) of
the oracle's in the scaled measure, env the envelope of the whole iterate, and E0 within 1024 x max(env_kkt, 1e-13) of the oracle's
kkt, env_kkt the envelope of the oracle's own kkt under the same perturbations."""
import numpy as np
import pytest

import lockstep_reference as LR
from test_host_harness import _run, harness  # noqa: F401  (the fixture that builds the executable)
from test_host_harness_wave import E0, ITERS, STATUS, U0, batch  # noqa: F401

N = 8
BUDGETS = (1, 2, 3, 5, 8, 13)
N_RESTO = 6  # column of a printed line


@pytest.fixture(scope="module")
def reference(orc, tables, batch):
    traj, env, unstable = LR.envelope(LR.factory(orc, tables), batch, N, range(0, max(BUDGETS) + 1))
    return dict(traj=traj, env=env, excluded=LR.excluded(env, unstable))


def test_reference_meets_the_caps(reference):
    ok, n_ex, n = LR.caps_hold(reference["excluded"], BUDGETS)
    print(f"host lock-step: excluded {n_ex} of {n} pairs")
    assert ok, (n_ex, n)


@pytest.mark.parametrize("riccati", ["8", "1"])
def test_harness_iterates_match_the_oracle_budget_by_budget(harness, tmp_path, reference, tables, batch, riccati):
    worst_u, worst_e, n_ex, failures = 0.0, 0.0, 0, []
    for m in BUDGETS:
        (r,) = _run(harness, tmp_path, tables, batch, N, ticks=1, riccati=riccati, max_iter=m)
        assert r.shape[0] == len(batch) and np.all(np.isfinite(r)), m
        iters = r[:, ITERS].astype(int)
        assert (iters <= m).all() and (iters >= 0).all(), (m, iters)
        ref, env = LR.aligned(reference["traj"], reference["env"], iters)
        _, ex = LR.aligned(reference["traj"], reference["excluded"], iters)
        nxt, _ = LR.aligned(reference["traj"], reference["env"], np.minimum(iters + 1, max(BUDGETS)))
        u_ref = ref["U"][:, 0, :]
        du = (np.abs(r[:, U0] - u_ref) / (1.0 + np.abs(u_ref))).max(axis=1) / np.maximum(env, LR.ENV_FLOOR)
        de = np.abs(r[:, E0] - ref["kkt"]) / (1.0 + np.abs(ref["kkt"])) / np.maximum(ref["env_kkt"], LR.ENV_FLOOR)
        n_ex += int(ex.sum())
        for b in np.flatnonzero(~ex):
            why = []
            if int(r[b, STATUS]) != ref["status"][b]:
                why.append(f"status {int(r[b, STATUS])} != {ref['status'][b]}")
            if int(r[b, N_RESTO]) != ref["n_resto"][b]:
                why.append(f"n_resto {int(r[b, N_RESTO])} != {ref['n_resto'][b]}")
            if ref["status"][b] == LR.STATUS_MAX_ITER and nxt["n_reg"][b] == 0 and iters[b] != m:
                # (the harness does not print n_reg: where the ORACLE needs no repeated sweep up to and in the iteration that
                #  follows this iterate, a pass is an iteration)
                why.append(f"iters {iters[b]} != budget")
            if not du[b] <= LR.FACTOR:
                why.append(f"u0 ratio {du[b]:.3g}")
            if not de[b] <= LR.FACTOR:
                why.append(f"E0 ratio {de[b]:.3g} ({r[b, E0]!r} against {ref['kkt'][b]!r}, env {ref['env_kkt'][b]:.2e})")
            if why:
                failures.append(f"m={m} b={b} (k={iters[b]}): " + "; ".join(why))
            worst_u, worst_e = max(worst_u, float(du[b])), max(worst_e, float(de[b]))
    print(f"host lock-step riccati={riccati}: worst ratio u0 {worst_u:.3g}, E0 {worst_e:.3g} (limit {LR.FACTOR:g}), excluded {n_ex} of "
          f"{len(BUDGETS) * len(batch)} pairs, failures {len(failures)}")
    assert not failures, "\n".join(failures)
