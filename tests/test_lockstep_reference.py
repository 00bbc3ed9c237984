"""tests/lockstep_reference.py by the oracle alone (CPU): the reference of every case of test_gpu_lockstep.py meets the caps on
excluded pairs, the comparison has teeth (a relative 1e-8 in params.mass, tau_min 0.99 -> 0.995 fail it in the first iterations),
and the oracle against itself passes with ratio 0."""
import numpy as np
import pytest

import lockstep_reference as LR

CASE_NAMES = ("a", "b", "c", "d", "e", "f", "g8", "g10")


@pytest.fixture(scope="module")
def all_cases(pkg, tables, orc):
    return LR.cases(pkg, tables, orc)


def test_case_list_is_complete(all_cases):
    assert tuple(all_cases) == CASE_NAMES
    assert LR.budgets(30) == list(range(1, 13)) + [15, 18, 21, 24, 27, 30] and LR.budgets(10) == list(range(1, 11))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_meets_the_caps_on_excluded_pairs(all_cases, orc, tables, name):
    """No pair excluded for k <= 10, at most 10 % of the pairs of the case excluded (env > 1e-8 or a discrete output changed under
    a rounding-level perturbation of x0, from that k on), over the budgets the GPU case runs and over every k = 0 .. K."""
    case = all_cases[name]
    ref = case.reference(orc, tables)
    assert sorted(ref["traj"]) == list(range(case.K + 1))
    for ks in (case.budgets, None):
        ok, n_ex, n = LR.caps_hold(ref["excluded"], ks)
        print(f"case {name}: N={case.N} B={case.B} K={case.K}: excluded {n_ex} of {n} pairs; largest envelope "
              f"{max(float(ref['env'][k].max()) for k in ref['env']):.2e}, at k <= 10 {max(float(ref['env'][k].max()) for k in range(11)):.2e}")
        assert ok, (name, n_ex, n)
    first = min((k for k in ref["excluded"] if ref["excluded"][k].any()), default=None)
    assert first is None or first > LR.CAP_FIRST_K
    # exclusion is for good: once out, out at every larger k
    for k in range(1, case.K + 1):
        assert not (ref["excluded"][k - 1] & ~ref["excluded"][k]).any()


def test_case_c_runs_until_convergence(all_cases, orc, tables):
    c = all_cases["c"]
    last = c.reference(orc, tables)["traj"][c.K]
    assert (last["status"] == 0).all() and last["iters"].max() <= c.budgets[-2] + 3, (last["status"], last["iters"])


@pytest.mark.parametrize("name", ["g8", "g10", "a"])
def test_elastic_phase_is_inside_the_compared_window(all_cases, orc, tables, name):
    """Case g (and the last instance of case a): an instance whose oracle trajectory has n_resto > 0 at budgets that are not
    excluded - from the entry of the restoration phase to its end."""
    case = all_cases[name]
    ref = case.reference(orc, tables)
    b = 0 if name != "a" else case.B - 1
    inside = [k for k in case.budgets if ref["traj"][k]["n_resto"][b] > 0 and not ref["excluded"][k][b]]
    assert len(inside) >= 6 and min(inside) <= 10, inside
    assert ref["traj"][case.K]["status"][b] == 0   # ... and it returns to the hard problem and converges


def test_oracle_against_itself_passes_with_ratio_zero(all_cases, orc, tables):
    """compare at every k, and check_runs with the oracle's own runs in the place of the device's."""
    for name in ("a", "e", "f", "g10"):
        case = all_cases[name]
        ref = case.reference(orc, tables)
        for k in case.budgets:
            r = ref["traj"][k]
            c = LR.compare(r, r, r, ref["env"][k])
            assert c["ok"].all() and c["ratio"].max() == 0.0, (name, k)
        rep = LR.check_runs(ref, {k: (ref["traj"][k], ref["traj"][k]) for k in case.budgets}, label=f"oracle as device, case {name}")
        assert not rep["failures"] and rep["worst"] == 0.0, rep["failures"][:5]


def test_a_perturbed_copy_is_inside_the_bound(all_cases, orc, tables):
    """The oracle from a sixth perturbed copy of x0 (another seed) stays within FACTOR x the envelope of the five: the envelope is
    not an artefact of the copies it was made from."""
    case = all_cases["a"]
    ref = case.reference(orc, tables)
    x = LR.perturbed(case.x0, copies=1, seed=99)[0]
    traj = LR.trajectory(LR.factory(orc, tables), x, case.N, case.budgets)
    rep = LR.check_runs(ref, {k: (traj[k], traj[k]) for k in case.budgets}, label="a sixth perturbed copy")
    assert not rep["failures"], rep["failures"][:5]


def test_the_comparison_has_teeth(all_cases, orc, tables):
    """A relative change of 1e-8 in params.mass fails compare for EVERY instance at each of k = 1, 2, 3; tau_min = 0.995 in place
    of 0.99 fails it for every instance by k = 2.  (Both still reach the same KKT point: nothing else in the suite sees them.)"""
    case = all_cases["a"]
    ref = case.reference(orc, tables)
    p = orc.default_params()
    p.mass *= 1.0 + 1e-8
    heavier = LR.trajectory(LR.factory(orc, tables, params=p), case.x0, case.N, [1, 2, 3])
    tau = LR.trajectory(LR.factory(orc, tables, tau_min=0.995), case.x0, case.N, [1, 2, 3])
    for k in (1, 2, 3):
        c = LR.compare(heavier[k], heavier[k], ref["traj"][k], ref["env"][k])
        print(f"k={k}: mass (1 + 1e-8): ratio {c['ratio'].min():.3g} .. {c['ratio'].max():.3g}")
        assert not c["ok"].any() and c["ratio"].min() > LR.FACTOR, (k, c["ratio"])
    c = LR.compare(tau[2], tau[2], ref["traj"][2], ref["env"][2])
    print(f"k=2: tau_min 0.995: ratio {c['ratio'].min():.3g} .. {c['ratio'].max():.3g}")
    assert not c["ok"].any() and c["ratio"].min() > LR.FACTOR
    rep = LR.check_runs(ref, {k: (heavier[k], heavier[k]) for k in (1, 2, 3)}, label="mass (1 + 1e-8) as device")
    assert len(rep["failures"]) == 3 * case.B


def test_discrete_outputs_and_mu_are_compared(all_cases, orc, tables):
    """A run whose iterate is the reference's but whose counters or barrier parameter are not fails."""
    case = all_cases["a"]
    ref = case.reference(orc, tables)
    k = 8
    r = ref["traj"][k]
    for key, change in (("n_reg", 1), ("n_lsfail", 1), ("status", -2), ("mu", 1e-10), ("n_resto", 1)):
        st = {n: v.copy() for n, v in r.items()}
        st[key][3] = st[key][3] + change if key != "mu" else st[key][3] * (1.0 + change)
        rep = LR.check_runs(ref, {k: (r, st)}, label=f"changed {key}")
        assert len(rep["failures"]) == 1 and "b=3" in rep["failures"][0] and key in rep["failures"][0], (key, rep["failures"])
    st = {n: v.copy() for n, v in r.items()}
    st["iters"][3] -= 1   # (compared with the oracle one iteration earlier: the iterate is then off by a whole step)
    assert LR.check_runs(ref, {k: (r, st)}, label="changed iters")["failures"]
