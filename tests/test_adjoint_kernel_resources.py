"""Register budget of the adjoint kernels (adjoint.h): compiled device-only for gfx950 with the flags of _build.py, both forms
of the sweep and the prediction gather run with no VGPR spilled and no scratch memory.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

KERNELS = ["_ZN6ltompc11k_adj_sweepENS_4WorkEddPKdS2_PKiS2_S2_PdS5_S5_",     # k_adj_sweep
           "_ZN6ltompc14k_adj_sweep_piENS_6WorkPIEPKdS2_PKiS2_S2_PdS5_S5_",  # k_adj_sweep_pi
           "_ZN6ltompc16k_prediction_devENS_4WorkEPdS1_"]                    # k_prediction_dev


@pytest.mark.parametrize("kernel", KERNELS)
def test_adjoint_kernels_do_not_spill(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
