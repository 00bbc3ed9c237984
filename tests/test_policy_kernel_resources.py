"""Register budget of the feedback-policy kernels (policy.h): compiled device-only for gfx950 with the flags of
_build.py, k_policy_gather, k_policy_step and k_policy_run / _pi / _ts run with no VGPR spilled and no scratch memory, like the
plant kernels whose d_plant the run kernels inline.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the fixture: one device-only compile with the resource report)

# the mangled names up to the argument list: ltompc::k_policy_gather, ...
KERNELS = ["_ZN6ltompc15k_policy_gatherE", "_ZN6ltompc13k_policy_stepE", "_ZN6ltompc12k_policy_runE", "_ZN6ltompc15k_policy_run_piE",
           "_ZN6ltompc15k_policy_run_tsE"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_policy_kernels_do_not_spill(resources, kernel):  # noqa: F811
    names = [k for k in resources if k.startswith(kernel)]
    assert len(names) == 1, f"{kernel}* not once in the compiler's resource report: {[k for k in resources if 'policy' in k]}"
    r = resources[names[0]]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
