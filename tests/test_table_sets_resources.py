"""Register budget of the per-instance-table-set kernels (the _ts entry points), compiled device-only for gfx950
with the flags of _build.py; the kernels that existed before them, the _pi ones included, still in the report under their
mangled names; the two textual copies (k_step1_ts, k_tab_scatter_ts) agree with their originals.  Needs hipcc, not a GPU."""
import os

import pytest

from conftest import ROOT
from test_instance_params_resources import CEILINGS as PI_CEILINGS, EXISTING, NO_SPILL as PI_NO_SPILL, REF, _kernel_text
from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

ANY = "INS_9BoundsAnyEEE"
LAUNCH = "vPKNS_6ConstsEPKNS_6WorkTSENS_6LaunchE"
# no VGPR spilled, no scratch: the plant and sens kernels of the issue, and the others that reach it
NO_SPILL = ["_ZN6ltompc10k_plant_tsENS_6ConstsEPKdS2_PKiiiS2_S2_diPd",
            "_ZN6ltompc15k_roll_plant_tsENS_6ConstsENS_6WorkTSEPddiPKiS4_",
            "_ZN6ltompc13k_riccati8_tsENS_6ConstsENS_6WorkTSENS_6LaunchEii",
            "_ZN6ltompc13k_riccati1_tsENS_6ConstsENS_6WorkTSENS_6LaunchEii",
            "_ZN6ltompc14k_riccati1q_tsENS_6ConstsENS_6WorkTSENS_6LaunchEii",
            "_ZN6ltompc9k_pick_tsEPKNS_6ConstsEPKNS_6WorkTSENS_6LaunchEi",
            f"_ZN6ltompc15k_linesearch_ts{REF}{LAUNCH}ii",
            f"_ZN6ltompc15k_linesearch_ts{ANY}{LAUNCH}ii",
            f"_ZN6ltompc13k_tab_cond_ts{REF}vPKNS_6ConstsEPKNS_6WorkTSEPKdPKiPd",
            f"_ZN6ltompc13k_tab_cond_ts{ANY}vPKNS_6ConstsEPKNS_6WorkTSEPKdPKiPd",
            "_ZN6ltompc16k_tab_scatter_tsEPKNS_6ConstsENS_4WorkEPKiPKdPdS5_",
            "_ZN6ltompc9k_init_tsEPKNS_6ConstsEPKNS_6WorkTSEi",
            "_ZN6ltompc11k_init_m_tsEPKNS_6ConstsEPKNS_6WorkTSEPKi",
            "_ZN6ltompc14k_roll_init_tsEPKNS_6ConstsEPKNS_6WorkTSENS_6LaunchEi",
            "_ZN6ltompc16k_roll_init_m_tsEPKNS_6ConstsEPKNS_6WorkTSENS_6LaunchEPKi",
            "_ZN6ltompc10k_ts_indexEPKiPiii"]
# in the report (they spill like their _pi forms: DESIGN.md §16 has the numbers)
PRESENT = [f"_ZN6ltompc9k_eval_ts{ANY}{LAUNCH}", f"_ZN6ltompc11k_expand_ts{ANY}{LAUNCH}", f"_ZN6ltompc10k_step1_ts{REF}{LAUNCH}",
           f"_ZN6ltompc10k_step1_ts{ANY}{LAUNCH}", f"_ZN6ltompc14k_sens_eval_ts{REF}vPKNS_6ConstsEPKNS_6WorkTSE",
           f"_ZN6ltompc14k_sens_eval_ts{ANY}vPKNS_6ConstsEPKNS_6WorkTSE"]
# one wavefront per SIMD at the benchmark's bound pattern, as the _pi forms; (VGPR spill, scratch bytes) reached by this build,
# pinned as ceilings.  The _pi forms reach (18, 76) and (16, 0): the set's index and pointers did not cost a register here.
CEILINGS = {f"_ZN6ltompc9k_eval_ts{REF}{LAUNCH}": (14, 60),
            f"_ZN6ltompc11k_expand_ts{REF}{LAUNCH}": (0, 0)}


@pytest.mark.parametrize("kernel", NO_SPILL)
def test_ts_kernels_do_not_spill(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r


@pytest.mark.parametrize("kernel", sorted(CEILINGS))
def test_ts_evaluation_kernels_keep_one_wavefront_per_simd(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    spill, scratch = CEILINGS[kernel]
    assert r["Occupancy"] == 1, r
    assert r["VGPRs Spill"] <= spill, r
    assert r["ScratchSize"] <= scratch, r


def test_every_ts_kernel_and_every_earlier_kernel_is_in_the_report(resources):  # noqa: F811
    missing = [k for k in PRESENT + EXISTING + PI_NO_SPILL + sorted(PI_CEILINGS) if k not in resources]
    assert not missing, missing


def _src(name):
    return open(os.path.join(ROOT, "lap-time-optimization_amd", "csrc", name)).read()


def test_step1_ts_is_step1_with_the_ts_functions():
    """k_step1_ts is a copy of k_step1, as k_step1_pi is (a shared device function changed the uniform kernel's code): the texts
    agree up to the name, the Work type and the _ts instantiations, so that a change to one cannot leave the other behind."""
    src = _src("linesearch.h")
    uni, ts = _kernel_text(src, "k_step1"), _kernel_text(src, "k_step1_ts")
    expect = (uni.replace("template <class BP, bool ELL>\n", "template <class BP>\n")
              .replace(" k_step1(const Consts* __restrict__ Kp, const Work* __restrict__ Wp,", " k_step1_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp,")
              .replace("d_linesearch<BP, false, ELL>(", "d_linesearch<BP, false, false, true, true>(")
              .replace("d_pick(K, W, b, tid >> 3, 1, false);", "d_pick<true, true>(K, W, b, tid >> 3, 1, false);"))
    assert ts.strip() == expect.strip()


def test_tab_scatter_ts_is_tab_scatter_into_the_block_of_the_set():
    """k_tab_scatter_ts is a copy of k_tab_scatter with one more argument and one more line (through a shared device function
    the uniform kernel's multiplies changed their operand order)."""
    src = _src("table_sensitivity.h")
    uni, ts = _kernel_text(src, "k_tab_scatter"), _kernel_text(src, "k_tab_scatter_ts")
    squeeze = lambda t: " ".join(t.split())
    expect = (squeeze(uni).replace(" k_tab_scatter(", " k_tab_scatter_ts(")
              .replace("double* __restrict__ grad_tables) {", "double* __restrict__ grad_tables, const int* __restrict__ tsi) {")
              .replace("const int n = T.n;", "const int n = T.n; grad_tables += (size_t)tsi[ob] * TAB_ROWS * n;"))
    assert squeeze(ts) == expect
