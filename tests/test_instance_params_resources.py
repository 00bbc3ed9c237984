"""Register budget of the per-instance-parameter kernels (the _pi entry points), compiled device-only for gfx950
with the flags of _build.py, and the kernels that existed before them still in the report under their mangled names.  Needs
hipcc, not a GPU."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the compiler's resource report, one compile per module)

REF = "INS_11BoundsFixedILj3ELj3ELj205ELj196EEEEE"  # the reference's bound pattern (BoundsRef), the benchmark's
# no VGPR spilled, no scratch
NO_SPILL = ["_ZN6ltompc13k_riccati8_piENS_6ConstsENS_6WorkPIENS_6LaunchEii",
            "_ZN6ltompc13k_riccati1_piENS_6ConstsENS_6WorkPIENS_6LaunchEii",
            "_ZN6ltompc14k_riccati1q_piENS_6ConstsENS_6WorkPIENS_6LaunchEii",
            "_ZN6ltompc10k_plant_piENS_6ConstsEPKdiiS2_S2_diPd",
            "_ZN6ltompc15k_roll_plant_piENS_6ConstsENS_6WorkPIEPddiPKiS4_",
            f"_ZN6ltompc15k_psens_cond_pi{REF}vPKNS_6ConstsEPKNS_6WorkPIEPd",
            "_ZN6ltompc15k_psens_cond_piINS_9BoundsAnyEEEvPKNS_6ConstsEPKNS_6WorkPIEPd",
            "_ZN6ltompc16k_psens_sweep_piENS_6WorkPIEPKdS2_PKiPdS5_S5_S5_",
            "_ZN6ltompc18k_sens_riccati8_piENS_6ConstsENS_6WorkPIEPKiPi"]
# one wavefront per SIMD at the benchmark's bound pattern, as the uniform kernels; the spills reached are pinned as ceilings
# (the uniform k_eval<BoundsRef> does not spill, its _pi form keeps the rows' loads and addresses beside it)
CEILINGS = {f"_ZN6ltompc9k_eval_pi{REF}vPKNS_6ConstsEPKNS_6WorkPIENS_6LaunchE": (18, 76),
            f"_ZN6ltompc11k_expand_pi{REF}vPKNS_6ConstsEPKNS_6WorkPIENS_6LaunchE": (16, 0)}
EXISTING = [
    "_ZN6ltompc10k_riccati1ENS_6ConstsENS_4WorkENS_6LaunchEii",
    "_ZN6ltompc10k_riccati8ENS_6ConstsENS_4WorkENS_6LaunchEii",
    "_ZN6ltompc10k_store_u0ENS_4WorkEPdPKi",
    "_ZN6ltompc11k_pack_permEPKiS1_PiS2_S2_",
    "_ZN6ltompc11k_riccati1qENS_6ConstsENS_4WorkENS_6LaunchEii",
    "_ZN6ltompc11k_roll_initEPKNS_6ConstsEPKNS_4WorkENS_6LaunchEi",
    "_ZN6ltompc11k_roll_markENS_4WorkEPKdii",
    "_ZN6ltompc11k_sens_evalINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb0EEEvPKNS_6ConstsEPKNS_4WorkE",
    "_ZN6ltompc11k_sens_evalINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb1EEEvPKNS_6ConstsEPKNS_4WorkE",
    "_ZN6ltompc11k_sens_evalINS_9BoundsAnyELb0EEEvPKNS_6ConstsEPKNS_4WorkE",
    "_ZN6ltompc11k_sens_evalINS_9BoundsAnyELb1EEEvPKNS_6ConstsEPKNS_4WorkE",
    "_ZN6ltompc12k_linesearchINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchEii",
    "_ZN6ltompc12k_linesearchINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchEii",
    "_ZN6ltompc12k_linesearchINS_9BoundsAnyELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchEii",
    "_ZN6ltompc12k_linesearchINS_9BoundsAnyELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchEii",
    "_ZN6ltompc12k_psens_condINS_11BoundsFixedILj3ELj3ELj205ELj196EEEEEvPKNS_6ConstsEPKNS_4WorkEPd",
    "_ZN6ltompc12k_psens_condINS_9BoundsAnyEEEvPKNS_6ConstsEPKNS_4WorkEPd",
    "_ZN6ltompc12k_roll_beginENS_4WorkEi",
    "_ZN6ltompc12k_roll_plantENS_6ConstsENS_4WorkEPddiPKiS4_",
    "_ZN6ltompc12k_sens_eval8EPKNS_6ConstsEPKNS_4WorkE",
    "_ZN6ltompc12k_test_modelENS_6ConstsEidPKdS2_PdS3_S3_S3_S3_S3_S3_S3_S3_",
    "_ZN6ltompc12k_zero_uprevENS_4WorkE",
    "_ZN6ltompc13k_psens_sweepENS_4WorkEddPKdS2_PKiPdS5_S5_S5_",
    "_ZN6ltompc13k_roll_finishENS_4WorkENS_6LaunchEPdPiS3_iS3_S3_",
    "_ZN6ltompc13k_slip_forcesENS_6ConstsEiPKdPdS3_",
    "_ZN6ltompc14k_act_identityEPiS0_i",
    "_ZN6ltompc14k_pack_inverseEPKiPii",
    "_ZN6ltompc14k_sens_forwardENS_4WorkEPKiiPdPiS3_S3_S3_S2_",
    "_ZN6ltompc14k_test_ellipseENS_6ConstsEiPKdPdS3_S3_",
    "_ZN6ltompc15k_sens_riccati8ENS_6ConstsENS_4WorkEPKiPi",
    "_ZN6ltompc15k_status_countsENS_4WorkEPiPy",
    "_ZN6ltompc18k_psens_keep_uprevENS_4WorkEPdPKi",
    "_ZN6ltompc18k_velocity_profileE17ltompc_vp_vehicleiiPKdS2_S2_PdS3_S3_S3_",
    "_ZN6ltompc6k_evalINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc6k_evalINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc6k_evalINS_9BoundsAnyELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc6k_evalINS_9BoundsAnyELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc6k_initEPKNS_6ConstsEPKNS_4WorkEi",
    "_ZN6ltompc6k_packENS_4WorkEPKiS2_iPiiii",
    "_ZN6ltompc6k_pickEPKNS_6ConstsEPKNS_4WorkENS_6LaunchEi",
    "_ZN6ltompc7k_eval8EPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc7k_plantENS_6ConstsEiPKdS2_diPd",
    "_ZN6ltompc7k_shiftENS_4WorkEi",
    "_ZN6ltompc7k_step1INS_11BoundsFixedILj3ELj3ELj205ELj196EEELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc7k_step1INS_11BoundsFixedILj3ELj3ELj205ELj196EEELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc7k_step1INS_9BoundsAnyELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc7k_step1INS_9BoundsAnyELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc8k_expandINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc8k_expandINS_11BoundsFixedILj3ELj3ELj205ELj196EEELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc8k_expandINS_9BoundsAnyELb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc8k_expandINS_9BoundsAnyELb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc8k_updateEPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc9k_compactEPKiS1_S1_PiS2_",
    "_ZN6ltompc9k_expand8EPKNS_6ConstsEPKNS_4WorkENS_6LaunchE",
    "_ZN6ltompc9k_load_x0ENS_4WorkEPKdPKiii",
    "_ZN6ltompc9k_riccatiEPKNS_6ConstsEPKNS_4WorkENS_6LaunchEi",
]


@pytest.mark.parametrize("kernel", NO_SPILL)
def test_pi_kernels_do_not_spill(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r


@pytest.mark.parametrize("kernel", sorted(CEILINGS))
def test_pi_evaluation_kernels_keep_one_wavefront_per_simd(resources, kernel):  # noqa: F811
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    spill, scratch = CEILINGS[kernel]
    assert r["Occupancy"] == 1, r
    assert r["VGPRs Spill"] <= spill, r
    assert r["ScratchSize"] <= scratch, r


def test_existing_kernels_keep_their_names(resources):  # noqa: F811
    missing = [k for k in EXISTING if k not in resources]
    assert not missing, missing


def _kernel_text(src, name):
    i = src.index(f" {name}(")
    start = src.rindex("template", 0, i) if src.rindex("template", 0, i) > src.rindex("\n}\n", 0, i) else src.rindex("\n", 0, i)
    return src[start:src.index("\n}\n", i) + 3]


def test_step1_pi_is_step1_with_the_pi_functions():
    """k_step1_pi is a copy of k_step1 (a shared device function changed the uniform kernel's code): the two texts agree up to
    the name, the Work type and the _pi instantiations, so that a change to one cannot leave the other behind."""
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "lap-time-optimization_amd", "csrc", "linesearch.h")).read()
    uni, pi = _kernel_text(src, "k_step1"), _kernel_text(src, "k_step1_pi")
    expect = (uni.replace("template <class BP, bool ELL>\n", "template <class BP>\n")
              .replace(" k_step1(const Consts* __restrict__ Kp, const Work* __restrict__ Wp,", " k_step1_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp,")
              .replace("d_linesearch<BP, false, ELL>(", "d_linesearch<BP, false, false, true>(")
              .replace("d_pick(K, W, b, tid >> 3, 1, false);", "d_pick<true>(K, W, b, tid >> 3, 1, false);"))
    assert pi.strip() == expect.strip()
