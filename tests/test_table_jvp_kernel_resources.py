"""Register budget of the kernels of the directional pass in the track tables (table_jvp.h): compiled device-only for gfx950 with
the flags of _build.py.  None of the kernels spills a VGPR or uses scratch memory; the counts below are what the compiler reports
today, pinned as ceilings (k_tabjvp_cond holds E1, E2, Hc and the M8 factor beside the summed kappa column: one wavefront per SIMD,
like k_tab_cond; the sweep has k_jvp_sweep's budget).  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

REF, ANY = "NS_11BoundsFixedILj3ELj3ELj205ELj196EEE", "NS_9BoundsAnyE"
# kernel -> ceilings (VGPRs, AGPRs)
KERNELS = {
    "_ZN6ltompc15k_jvp_sweep_tabENS_4WorkEddPKdPKiS2_PdS5_S5_": (180, 0),                          # k_jvp_sweep_tab
    "_ZN6ltompc18k_jvp_sweep_tab_piENS_6WorkPIEPKdPKiS2_PdS5_S5_": (180, 0),                       # k_jvp_sweep_tab_pi
    f"_ZN6ltompc13k_tabjvp_condI{REF}EEvPKNS_6ConstsEPKNS_4WorkEPKiPKdSC_Pd": (256, 36),          # k_tabjvp_cond<BoundsRef>
    f"_ZN6ltompc13k_tabjvp_condI{ANY}EEvPKNS_6ConstsEPKNS_4WorkEPKiPKdSB_Pd": (256, 28),          # k_tabjvp_cond<BoundsAny>
    f"_ZN6ltompc16k_tabjvp_cond_piI{REF}EEvPKNS_6ConstsEPKNS_6WorkPIEPKiPKdSC_Pd": (256, 36),     # k_tabjvp_cond_pi<BoundsRef>
    f"_ZN6ltompc16k_tabjvp_cond_piI{ANY}EEvPKNS_6ConstsEPKNS_6WorkPIEPKiPKdSB_Pd": (256, 34),     # k_tabjvp_cond_pi<BoundsAny>
    f"_ZN6ltompc16k_tabjvp_cond_tsI{REF}EEvPKNS_6ConstsEPKNS_6WorkTSEPKiPKdSC_Pd": (256, 40),     # k_tabjvp_cond_ts<BoundsRef>
    f"_ZN6ltompc16k_tabjvp_cond_tsI{ANY}EEvPKNS_6ConstsEPKNS_6WorkTSEPKiPKdSB_Pd": (256, 34),     # k_tabjvp_cond_ts<BoundsAny>
}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_table_jvp_kernels_stay_within_their_registers(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r, (vgprs, agprs) = resources[kernel], KERNELS[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["VGPRs"] <= vgprs and r["AGPRs"] <= agprs, r
