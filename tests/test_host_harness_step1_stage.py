"""k_step1 with the instance's operands staged in LDS (csrc/linesearch.h: d_step1_stage, StepStage) on the sanitizer harness of
test_host_harness.py: the k_step1 path (step=1) against the separate k_linesearch / k_pick / k_update launches (the harness's
default), which read the planes - bit for bit.  __shared__ is a static array of the program there, NaN-free only where the
staging wrote it: a read of a word that was not staged, or staged from the wrong place, changes the bits; a read or a write past
the array or past a plane (every buffer at its exact size) ends the run in AddressSanitizer.

Compared per tick, as tests/test_host_harness_step1_update.py does (its helpers are used): every printed value and, through the
harness's derivs=1 record, the whole iterate; where the harness makes no record (the friction ellipse) or the record is not needed
for the point (the _pi form), the printed values and the final=1 block over two ticks.  Every k_step1 run is made with the
wavefronts in ascending and in descending order between two barriers: the staging writes what other wavefronts read, and the
second window overwrites what the readers of the first have read.

Horizons: N = 2 (the shortest: three columns, 106 rows of lanes), 8, 40 (the benchmark's: one window, the update reads it) and the
two at the staging boundary of the reference's bound pattern, derived below from the constants of linesearch.h: N = 67 is the last
horizon held by ONE window, N = 68 the first that takes two (one slot in the second; its update reads the planes).  B = 2: the
reference's x0 and the state that needs the restoration phase (elastic rows in use).  Two ticks (the second starts from the first
one's iterate) at N = 2 and 8, one cold tick from N = 40 on, and the restoration state alone at the two boundary horizons, where
one instance's tick under the sanitizers takes ten seconds or more in each of the three runs.  Variants at
N = 8: the run-time bound pattern, soft_rho = 100, the friction ellipse (two more rows of T, R = 28), the _pi form; the states of
test_gpu_pick_paths.py at N = 10 take the shifted restart (asserted).  Test infrastructure only."""
import re

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_instance_params import GROUPS, _row
from test_gpu_pick_paths import _states
from test_host_harness import harness  # noqa: F401  (the fixture that builds the executable)
from test_host_harness_step1_update import NSHIFT, _assert_same, _ni, _three
from test_host_harness_wave import RESTORATION_STATE


def _constants():
    src = open(f"{ROOT}/lap-time-optimization_amd/csrc/linesearch.h").read()
    words = int(re.search(r"constexpr int STG_WORDS = (\d+);", src).group(1))
    sg_t = int(re.search(r"SG_T = (\d+) \}", src).group(1))
    assert "return SG_T + 2 * R + 1;" in src and "(STG_WORDS - 2 - N) / stage_stride(R)" in src and "c < 128 ? c : 128" in src
    return words, sg_t


def one_window(N, R):
    """StepStage::whole(): N <= stage_cols(N, R) - 1."""
    words, sg_t = _constants()
    return N <= min((words - 2 - N) // (sg_t + 2 * R + 1), 128) - 1


@pytest.fixture(scope="module")
def boundary(pkg):
    R = _ni(pkg) + 3  # ni rows of slacks and the three elastic rows of the track constraints
    last = max(N for N in range(2, 300) if one_window(N, R))
    assert not one_window(last + 1, R)
    return last, last + 1


@pytest.fixture(scope="module")
def x2(pkg):
    return np.array([pkg.X0_REFERENCE, RESTORATION_STATE])


def test_the_boundary_of_the_reference_pattern(pkg, boundary):
    assert _ni(pkg) == 23 and boundary == (67, 68)
    assert one_window(40, 26) and one_window(40, 28)  # the benchmark's horizon, without and with the ellipse's rows


@pytest.mark.parametrize("N", [2, 8, 40, "last", "first"])
def test_staged_step1_matches_the_separate_launches_bit_for_bit(harness, tmp_path, pkg, tables, x2, boundary, N):  # noqa: F811
    N = {"last": boundary[0], "first": boundary[1]}.get(N, N)
    x0 = x2 if N <= 40 else x2[1:]
    runs = _three(harness, tmp_path, pkg, tables, x0, N, 2 if N < 40 else 1)  # (a cold solve is 15 - 30 passes of k_step1)
    _assert_same(runs)
    assert runs[0][0][0][-1, 6] >= 1  # (the restoration state's solve ran on elastic variables)


def test_with_a_run_time_bound_pattern(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, any_bounds=1))


def test_with_soft_constraints(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, soft_rho=100.0))


def test_with_the_friction_ellipse(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, record=False, ell=(10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0)))


def test_the_pi_form(harness, tmp_path, pkg, tables, x2):  # noqa: F811
    rows = np.stack([_row(pkg, GROUPS[0]), _row(pkg, GROUPS[2])])
    _assert_same(_three(harness, tmp_path, pkg, tables, x2, 8, 2, record=False, rows=rows))


def test_a_shifted_restart(harness, tmp_path, pkg, tables):  # noqa: F811
    runs = _three(harness, tmp_path, pkg, tables, _states(pkg, tables)[:12], 10, 3)
    _assert_same(runs)
    assert sum(int(r[:, NSHIFT].sum()) for r in runs[1][0]) >= 1
