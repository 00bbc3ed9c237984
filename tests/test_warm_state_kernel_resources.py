"""The kernels of csrc/warm_state.h, compiled device-only for gfx950 with the flags of _build.py: none of them
spills a register or uses scratch memory, by the compiler's own report.  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

# a unique part of every kernel's mangled name
KERNELS = ["11k_load_x0_mE", "8k_init_mE", "11k_init_m_piE", "13k_roll_mark_mE", "13k_roll_init_mE", "16k_roll_init_m_piE",
           "15k_ws_reset_markE", "15k_ws_reset_initE", "10k_ws_guessE", "11k_ws_exportE", "11k_ws_importE"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_warm_state_kernels_do_not_spill(resources, kernel):  # noqa: F811
    names = [n for n in resources if n.startswith("_ZN6ltompc" + kernel)]
    assert len(names) == 1, (kernel, names)
    r = resources[names[0]]
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
