"""Register budget of the step-selection kernels after d_pick and d_head8 were given one batch of loads each (profiles/r06):
compiled device-only for gfx950 with the flags of _build.py, k_pick and k_pick_pi hold the whole batch (state, filter, step
partials, measures of two candidates) in registers - no VGPR spilled, no scratch memory - and the SGPRs spilled to VGPR lanes
by them and by the bench's k_step1 stay at what that change reached (before it: 128 in k_pick, 132 in k_pick_pi, 109 in
k_step1<BoundsRef, false>).  k_riccati8, whose head now fetches its state in one batch as well, keeps the budget that
test_kernel_resources.py pins.  What that change made worse is held where it left it: the SGPRs spilled by k_riccati1 and
k_riccati1q (109 -> 155, 104 -> 160: to VGPR lanes, no memory traffic; both kernels got faster, profiles/r06) and the spills of
k_step1_pi, which is not spill-free before either (16 -> 24 VGPRs in the same 68 B of scratch for <BoundsRef>).  Needs hipcc, not
a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture: one device-only compilation)

REF = "INS_11BoundsFixedILj3ELj3ELj205ELj196EEE"
K_PICK = "_ZN6ltompc6k_pickEPKNS_6ConstsEPKNS_4WorkENS_6LaunchEi"
K_PICK_PI = "_ZN6ltompc9k_pick_piEPKNS_6ConstsEPKNS_6WorkPIENS_6LaunchEi"
K_STEP1 = f"_ZN6ltompc7k_step1{REF}Lb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE"
K_RICCATI8 = "_ZN6ltompc10k_riccati8ENS_6ConstsENS_4WorkENS_6LaunchEii"
K_RICCATI1 = "_ZN6ltompc10k_riccati1ENS_6ConstsENS_4WorkENS_6LaunchEii"
K_RICCATI1Q = "_ZN6ltompc11k_riccati1qENS_6ConstsENS_4WorkENS_6LaunchEii"
K_STEP1_PI = f"_ZN6ltompc10k_step1_pi{REF}EEvPKNS_6ConstsEPKNS_6WorkPIENS_6LaunchE"
K_STEP1_PI_ANY = "_ZN6ltompc10k_step1_piINS_9BoundsAnyEEEvPKNS_6ConstsEPKNS_6WorkPIENS_6LaunchE"
SGPR_SPILL_CEILING = {K_PICK: 141, K_PICK_PI: 133, K_STEP1: 95, K_RICCATI1: 155, K_RICCATI1Q: 160}  # (before: 128, 132, 109, 109, 104)
STEP1_PI_CEILING = {K_STEP1_PI: (24, 68), K_STEP1_PI_ANY: (12, 52)}  # spilled VGPRs, scratch bytes per lane (before: (16, 68), (12, 52))


@pytest.mark.parametrize("kernel", [K_PICK, K_PICK_PI])
def test_pick_kernels_do_not_spill_vgprs(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r


@pytest.mark.parametrize("kernel", sorted(SGPR_SPILL_CEILING))
def test_sgpr_spills_stay_where_the_batched_loads_left_them(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["SGPRs Spill"] <= SGPR_SPILL_CEILING[kernel], r


def test_step1_of_the_bench_does_not_spill_vgprs(resources):  # noqa: F811
    """The batch of d_pick is sized (PICK_Q stages per lane) so that it fits the 256 registers of k_step1's two wavefronts per SIMD."""
    r = resources[K_STEP1]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 2, r


@pytest.mark.parametrize("kernel", sorted(STEP1_PI_CEILING))
def test_step1_pi_spills_no_more_than_it_does(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    spill, scratch = STEP1_PI_CEILING[kernel]
    assert r["VGPRs Spill"] <= spill, r
    assert r["ScratchSize"] <= scratch, r
    assert r["Occupancy"] == 2, r


def test_riccati8_keeps_its_budget(resources):  # noqa: F811
    r = resources[K_RICCATI8]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 1, r
