"""Register budget and memory waits of k_step1 after its update was split (csrc/linesearch.h: d_update_fetch on wavefronts 1..4
beside d_pick, d_update_store after the second barrier; profiles/r08): from one device-only compilation for gfx950 with the flags
of _build.py, the three forms of the reference's bound pattern - k_step1, k_step1_pi, k_step1_ts - spill no VGPR, use no scratch
memory and keep two wavefronts per SIMD although 48 more words per lane are in flight while d_pick runs; k_update, which still
runs d_update itself, is as spill-free as before; and in the ISA of the benchmark's k_step1 the `s_waitcnt vmcnt` that follow new
global loads stay at what the split reached: d_update's dozen dependent round trips are no longer in the kernel (its branch for the
shifted restart is, called by d_update_store).  Needs hipcc, not a GPU."""
import pytest

from test_kernel_resources_lut import isa  # noqa: F401  (the module-scoped fixture: one device-only compilation to assembly)

REF = "INS_11BoundsFixedILj3ELj3ELj205ELj196EEE"
K_STEP1 = f"_ZN6ltompc7k_step1{REF}Lb0EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE"
K_STEP1_ELL = f"_ZN6ltompc7k_step1{REF}Lb1EEEvPKNS_6ConstsEPKNS_4WorkENS_6LaunchE"
K_STEP1_PI = f"_ZN6ltompc10k_step1_pi{REF}EEvPKNS_6ConstsEPKNS_6WorkPIENS_6LaunchE"
K_STEP1_TS = f"_ZN6ltompc10k_step1_ts{REF}EEvPKNS_6ConstsEPKNS_6WorkTSENS_6LaunchE"
K_UPDATE = "_ZN6ltompc8k_updateEPKNS_6ConstsEPKNS_4WorkENS_6LaunchE"
# waits after one or two new loads / after any new loads, measured from the final build   (the parent commit)
SHORT_WAIT_CEILING = 27  # (36)
LOAD_WAIT_CEILING = 58   # (69)


@pytest.mark.parametrize("kernel", [K_STEP1, K_STEP1_ELL, K_STEP1_PI, K_STEP1_TS, K_UPDATE])
def test_no_spills_and_two_wavefronts_per_simd(isa, kernel):  # noqa: F811
    rows, _ = isa
    assert kernel in rows, f"{kernel} not in the compiler's resource report"
    r = rows[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 2, r


def test_waits_of_the_update_are_gone_from_step1(isa):  # noqa: F811
    _, waits = isa
    assert K_STEP1 in waits, f"{K_STEP1} not in the assembly"
    short = sum(1 for loads, stores in waits[K_STEP1] if 1 <= loads <= 2 and stores == 0)
    with_loads = sum(1 for loads, stores in waits[K_STEP1] if loads >= 1)
    print(K_STEP1, "waits", len(waits[K_STEP1]), "after one or two loads", short, "after any loads", with_loads)
    assert short <= SHORT_WAIT_CEILING, (short, waits[K_STEP1])
    assert with_loads <= LOAD_WAIT_CEILING, (with_loads, waits[K_STEP1])
