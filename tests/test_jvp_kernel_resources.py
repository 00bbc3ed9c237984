"""Register budget of the directional sweep (jvp.h): compiled device-only for gfx950 with the flags of _build.py,
k_jvp_sweep and k_jvp_sweep_pi run with no VGPR spilled and no scratch memory.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the fixture: one device-only compile with the resource report)

KERNELS = ["_ZN6ltompc11k_jvp_sweepENS_4WorkEddPKdS2_PKiS2_S2_PdS5_S5_",  # ltompc::k_jvp_sweep
           "_ZN6ltompc14k_jvp_sweep_piENS_6WorkPIEPKdS2_PKiS2_S2_PdS5_S5_"]  # ltompc::k_jvp_sweep_pi


@pytest.mark.parametrize("kernel", KERNELS)
def test_jvp_sweep_does_not_spill(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report: {[k for k in resources if 'jvp' in k]}"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
