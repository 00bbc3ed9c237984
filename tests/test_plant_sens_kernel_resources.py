"""Register budget of the plant-step sensitivity kernels and the closed-loop accumulator (plant_sensitivity.h): compiled
device-only for gfx950 with the flags of _build.py, they run with no VGPR spilled and no scratch memory.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

KERNELS = ["_ZN6ltompc12k_plant_sensENS_6ConstsEiiPKdS2_diiPd",           # k_plant_sens
           "_ZN6ltompc15k_plant_sens_piENS_6ConstsEPKdiiS2_S2_diiPd",     # k_plant_sens_pi
           "_ZN6ltompc12k_loop_accumEiiiPKdS1_PKiS1_PdS4_PiS5_"]          # k_loop_accum


@pytest.mark.parametrize("kernel", KERNELS)
def test_plant_sens_kernels_do_not_spill(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
