"""Register budget of the table-gradient kernels (table_sensitivity.h): compiled device-only for gfx950 with the flags of
_build.py.  None of the kernels spills a VGPR or uses scratch memory; the counts below are what the compiler
reports today, pinned as ceilings (k_tab_cond holds E1, E2, Hc and the M8 factor beside one column: all 256 architectural VGPRs
and up to 124 accumulation registers as spill space, one wavefront per SIMD, like k_psens_cond).  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

REF, ANY = "NS_11BoundsFixedILj3ELj3ELj205ELj196EEE", "NS_9BoundsAnyE"
# kernel -> ceilings (VGPRs, AGPRs)
KERNELS = {
    "_ZN6ltompc15k_adj_sweep_tabENS_4WorkEddPKdS2_Pd": (164, 0),              # k_adj_sweep_tab
    "_ZN6ltompc18k_adj_sweep_tab_piENS_6WorkPIEPKdS2_Pd": (164, 0),           # k_adj_sweep_tab_pi
    "_ZN6ltompc13k_tab_scatterEPKNS_6ConstsENS_4WorkEPKiPKdPd": (52, 0),     # k_tab_scatter
    "_ZN6ltompc9k_tab_addEPdPKdi": (8, 0),                                   # k_tab_add
    f"_ZN6ltompc10k_tab_condI{REF}EEvPKNS_6ConstsEPKNS_4WorkEPKdPKiPd": (256, 124),       # k_tab_cond<BoundsRef>
    f"_ZN6ltompc10k_tab_condI{ANY}EEvPKNS_6ConstsEPKNS_4WorkEPKdPKiPd": (256, 124),       # k_tab_cond<BoundsAny>
    f"_ZN6ltompc13k_tab_cond_piI{REF}EEvPKNS_6ConstsEPKNS_6WorkPIEPKdPKiPd": (256, 124),  # k_tab_cond_pi<BoundsRef>
    f"_ZN6ltompc13k_tab_cond_piI{ANY}EEvPKNS_6ConstsEPKNS_6WorkPIEPKdPKiPd": (256, 124),  # k_tab_cond_pi<BoundsAny>
}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_table_kernels_stay_within_their_registers(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r, (vgprs, agprs) = resources[kernel], KERNELS[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["VGPRs"] <= vgprs and r["AGPRs"] <= agprs, r
