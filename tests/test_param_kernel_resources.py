"""Register budget of the parameter-sensitivity kernels (param_sensitivity.h): compiled device-only for gfx950 with the flags of
_build.py, they run with no VGPR spilled and no scratch memory.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

KERNELS = ["_ZN6ltompc12k_psens_condINS_11BoundsFixedILj3ELj3ELj205ELj196EEEEEvPKNS_6ConstsEPKNS_4WorkEPd",  # k_psens_cond<BoundsRef>
           "_ZN6ltompc12k_psens_condINS_9BoundsAnyEEEvPKNS_6ConstsEPKNS_4WorkEPd",                      # k_psens_cond<BoundsAny>
           "_ZN6ltompc13k_psens_sweepENS_4WorkEddPKdS2_PKiPdS5_S5_S5_",                               # k_psens_sweep
           "_ZN6ltompc18k_psens_keep_uprevENS_4WorkEPdPKi"]                                         # k_psens_keep_uprev


@pytest.mark.parametrize("kernel", KERNELS)
def test_param_sensitivity_kernels_do_not_spill(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
