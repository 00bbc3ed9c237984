"""k_step1's split update (csrc/linesearch.h: d_update_fetch beside d_pick on wavefronts 1..4, d_update_store after the second
barrier) on the sanitizer harness of test_host_harness.py: the k_step1 path (step=1) against the separate k_linesearch / k_pick /
k_update launches (the harness's default), which still run d_update itself - bit for bit.

Compared per tick: every printed value (status, iterations, u0, E0, the recovery counters, the largest elastic variable, g(x0)) and,
through the harness's derivs=1 record, the whole iterate (X, C, U, L1, L2, T, NU), mu and the outputs of the derivative passes that
read it.  With the friction ellipse the harness makes no such record (its derivative passes refuse the ellipse): there the
printed values and the final=1 block (x0, u_prev, the last node, U_0, E0) are compared, over two ticks, the second of which starts
from the first one's iterate.  The elastic variables are not in the record either; they enter every later iteration's step.

Every k_step1 run is made with the wavefronts in ascending and in descending order between two barriers: d_update_fetch reads
while d_pick writes, so a word that both touched would differ between the two orders.

Shapes: two ticks, B = 2 (the reference's x0 and the state that needs the restoration phase, which runs on elastic variables), at
N = 8, 40 (the benchmark's: every slot fetched ahead, rows 0..7 of slots 32..39 in the second round), 41 (the candidate loop wraps)
and 79 (slots 64..78 are loaded after the barrier).  soft_rho = 100 (elastic pairs in every iteration), the friction ellipse
(elastic rows 3, 4) and LTOMPC_BOUNDS=any's instantiation once each at the cheapest horizon where the mapping's clamps differ from
the plain case: N = 8.  The states of test_gpu_pick_paths.py, three ticks at N = 10: their run takes the shifted restart
(SI_SHIFT: d_update_store calls d_update), asserted from the counters the harness prints.  Test infrastructure only."""
import numpy as np
import pytest

from test_gpu_pick_paths import _states
from test_host_harness import _run, harness  # noqa: F401  (the fixture that builds the executable)
from test_host_harness_wave import RESTORATION_STATE, read_dump, same_bits

NSHIFT = 7  # column of a printed line (harness.cpp): SI_NSHIFT


def _ni(pkg, soft=False):
    return len(__import__("sens_reference").bound_rows(pkg.default_params())) + 3


def _three(harness, tmp, pkg, tables, x0, N, ticks, record=True, **kw):  # noqa: F811
    """The run through the separate launches and the two through k_step1; with record, (printed, iterate record) each."""
    out = []
    for name, args in (("sep", ()), ("asc", ("step=1", "wave_order=asc")), ("desc", ("step=1", "wave_order=desc"))):
        extra = dict(derivs=1, dump=str(tmp / f"{name}.bin")) if record else dict(final=1)
        res = _run(harness, tmp, tables, x0, N, ticks=ticks, riccati="1q", args=args, **extra, **kw)
        assert len(res) == ticks + (0 if record else 1) and all(np.all(np.isfinite(r)) for r in res), name
        rec = read_dump(tmp / f"{name}.bin", len(x0), N, _ni(pkg), ticks, 0, loop=False) if record else None
        out.append((res, rec))
    return out


def _assert_same(runs):
    (r0, d0) = runs[0]
    for r, d in runs[1:]:
        assert same_bits(r0, r)
        if d0 is not None:
            for t, (a, b) in enumerate(zip(d0, d)):
                for key in a:
                    if key != "adj":
                        assert np.array_equal(a[key], b[key], equal_nan=True), (t, key)


@pytest.fixture(scope="module")
def x2(pkg):
    return np.array([pkg.X0_REFERENCE, RESTORATION_STATE])


@pytest.mark.parametrize("N", [8, 40, 41, 79])
def test_split_update_matches_d_update_bit_for_bit(harness, tmp_path, pkg, tables, x2, N):  # noqa: F811
    runs = _three(harness, tmp_path, pkg, tables, x2, N, 2)
    _assert_same(runs)
    # (the restoration state's solve ran on elastic variables: the elastic pairs of d_update_store were written)
    assert runs[0][0][0][1, 6] >= 1


def test_split_update_with_soft_constraints(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, soft_rho=100.0))


def test_split_update_with_the_friction_ellipse(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, record=False, ell=(10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0)))


def test_split_update_with_a_run_time_bound_pattern(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, any_bounds=1))


def test_shifted_restart_through_the_split_update(harness, tmp_path, pkg, tables):  # noqa: F811
    x0 = _states(pkg, tables)[:12]
    runs = _three(harness, tmp_path, pkg, tables, x0, 10, 3)
    _assert_same(runs)
    n_shift = sum(int(r[:, NSHIFT].sum()) for r in runs[1][0])
    assert n_shift >= 1, [r[:, NSHIFT] for r in runs[1][0]]
