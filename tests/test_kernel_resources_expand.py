"""Register budget of the step expansion (k_expand, linearise.h) and of the RK4 plant step (k_plant, k_roll_plant): compiled
device-only for gfx950 with the flags of _build.py.  The instantiation the benchmark runs (the reference's bound pattern, no
friction ellipse) and both plant kernels have no VGPR spilled and no scratch memory; k_expand stays at one wavefront per SIMD
(two were measured 1.6 - 2x slower) and its SGPR spills do not grow.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

EXPAND_REF = "_ZN6ltompc8k_expandINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE"
PLANT = ["_ZN6ltompc7k_plantENS_6ConstsEiPKdS2_diPd",                      # ltompc::k_plant
         "_ZN6ltompc12k_roll_plantENS_6ConstsENS_4WorkEPddiPKiS4_"]        # ltompc::k_roll_plant
# the other instantiations: spilled VGPRs no higher than before the costate was pinned ahead of the linearisation
EXPAND_OTHERS = {
    "_ZN6ltompc8k_expandINS_9BoundsAnyELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE": 34,                           # <BoundsAny, false>
    "_ZN6ltompc8k_expandINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE": 113,  # <BoundsRef, true>
    "_ZN6ltompc8k_expandINS_9BoundsAnyELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE": 68,                           # <BoundsAny, true>
}
SGPR_SPILL_MAX = 64  # builds with 100 - 160 spilled SGPRs gave run-to-run varying results in the last interval


def _row(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    return resources[kernel]


def test_expand_bench_instantiation_does_not_spill(resources):  # noqa: F811
    r = _row(resources, EXPAND_REF)
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 1, r
    assert r["SGPRs Spill"] <= SGPR_SPILL_MAX, r


@pytest.mark.parametrize("kernel", sorted(EXPAND_OTHERS))
def test_expand_other_instantiations_spill_no_more(resources, kernel):  # noqa: F811
    r = _row(resources, kernel)
    assert r["VGPRs Spill"] <= EXPAND_OTHERS[kernel], r
    assert r["Occupancy"] == 1, r


@pytest.mark.parametrize("kernel", PLANT)
def test_plant_step_does_not_spill(resources, kernel):  # noqa: F811
    r = _row(resources, kernel)
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
