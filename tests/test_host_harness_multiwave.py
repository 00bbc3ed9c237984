"""The kernels whose workgroups have several wavefronts, as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer on the
lock-step workgroup of tests/host_harness/hip_shim.h: k_riccati1q (256 lanes, four wavefronts exchanging through LDS at
WG_SYNC_LDS barriers), k_step1 (320 lanes, two __syncthreads()), k_compact and k_pack_perm (1024 lanes, a scan in LDS), k_pack /
k_pack_inverse, the rollout kernels (k_roll_begin / _mark / _init / _finish / _plant) and the _pi forms.  Beside what the
sanitizers see (every buffer at its exact size and NaN-filled, k_riccati1q's dynamic LDS too), the executor ends a run in which
the lanes of a workgroup do not reach the same barrier, and EVERY multi-wavefront run here is made twice, with the wavefronts
running in ascending and in descending order between two barriers (wave_order=asc|desc): all printed values must be
bit-identical.  A missing barrier between a write of one wavefront and a read of another makes the two orders read different
values, which no sanitizer sees; the executor's self-test below shows that on a kernel with the barrier compiled out.

Shapes: the B = 9 batch of test_host_harness_wave.py (restoration state and off-track state included) and N in {2, 8, 11}
(11: d_riccati1q's staging loop makes a full round and a clamped remainder round of 3; 2: the shortest horizon with a successor
stage); one run at N = 41 with B = 2 takes k_step1 through its second, partial pass of 320 threads.  The multi-wavefront forms
are compared bit for bit with the one-wavefront forms and the separate launches (the project's rule for kernel paths) and with
the oracle by check_against_oracle of test_host_harness_wave.py.

What the harness cannot model: several lanes adding to ONE LDS word in the same instruction, the ordering of global memory
between workgroups (blocks run one after the other), and the rollout's two streams (the plant kernel runs after its pass).

Wall time, each file alone on the same 8-core machine: this file 323 s (164 s for the fixture's compilation of the harness,
which the first harness file of a session pays, and 159 s for the tests); tests/test_host_harness_wave.py at the parent commit
271 s (139 s + 132 s).  The tests take 27 s longer than that file's although the ticks are cut to the least that still reaches
the code (one cold tick, a warm one only at N = 2, in one run at N = 8, in the re-packing runs and in the rollout's three):
every multi-wavefront run is made twice, and the shapes (B = 9; N = 2, 8, 11; N = 41) are kept.  Every harness run is made once
per session and shared.  Test infrastructure only: the package never builds or
loads the harness."""
import os
import subprocess

import numpy as np
import pytest

from test_host_harness import _run, harness  # noqa: F401  (the fixture that builds the executable)
from test_host_harness_wave import (E0, ITERS, PRINTED, STATUS, THETA_A, THETA_B, U0, batch, check_against_oracle,  # noqa: F401
                                    oracle_params, same_bits, theta_rows)

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
LOGGED = [STATUS, ITERS, 3, 4]  # what the rollout logs per tick: status, iterations, u0


def _direct(harness, *args):
    """A mode of the harness that reads no problem file (selftest=..., scan)."""
    return subprocess.run([harness, "-", *args], capture_output=True, text=True, env=ENV, timeout=300)


def _clean(out):
    return "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


@pytest.fixture(scope="module")
def mruns(harness, tmp_path_factory, tables, batch):
    """Harness runs, each made once and shared.  both=True (a run with multi-wavefront kernels): made with wave_order=asc and
    with wave_order=desc, every printed value of the two bit-identical; the ascending run is returned."""
    cache = {}

    def run(N, ticks, any_bounds=0, rows=None, x0=None, both=True, args=(), **options):
        key = (N, ticks, any_bounds, None if rows is None else rows.tobytes(), None if x0 is None else x0.tobytes(), both, tuple(args),
               tuple(sorted(options.items())))
        if key not in cache:
            res = []
            for order in (("asc", "desc") if both else ("asc",)):
                r = _run(harness, tmp_path_factory.mktemp("multiwave"), tables, batch if x0 is None else x0, N, any_bounds=any_bounds, ticks=ticks,
                         rows=rows, args=tuple(args) + (f"wave_order={order}",), **options)
                assert len(r) == ticks + (1 if options.get("final") else 0) and all(np.all(np.isfinite(a)) for a in r), (key, order)
                res.append(r)
            assert len(res) == 1 or same_bits(res[0], res[1]), ("the two wavefront orders differ: a barrier is missing", key)
            cache[key] = res[0]
        return cache[key]
    return run


# ---------------------------------------------------------------------------------------------------- the executor itself
def test_executor_orders_detect_a_missing_barrier_and_report_a_diverged_one(harness):
    """The harness's own two-wavefront kernel: thread 64 writes an LDS word, thread 0 reads it.  With the barrier both orders
    read the written value; with the barrier compiled out the orders differ (the detector works); a barrier inside
    `if (threadIdx.x < 64)` while the other lanes wait at a later one, and a __shfl that only half of each wavefront reaches, end
    the run with exit status 3 and a report that names the sites and the lanes."""
    val = {}
    for case in ("barrier", "nobarrier"):
        for order in ("asc", "desc"):
            out = _direct(harness, f"selftest={case}", f"wave_order={order}")
            assert out.returncode == 0 and _clean(out), out.stderr[-2000:]
            val[case, order] = out.stdout.strip()
    assert val["barrier", "asc"] == val["barrier", "desc"] == "value 7"
    assert val["nobarrier", "asc"] != val["nobarrier", "desc"], val
    for order in ("asc", "desc"):
        out = _direct(harness, "selftest=diverged_barrier", f"wave_order={order}")
        assert out.returncode == 3 and _clean(out), (out.returncode, out.stderr[-2000:])
        assert "MISMATCHED COLLECTIVE in k_selftest<diverged_barrier>" in out.stderr and "stand at different barriers" in out.stderr
        sites = [ln for ln in out.stderr.splitlines() if "at __syncthreads, " in ln]
        assert len(sites) == 2 and sites[0].endswith("lanes 0-63") and sites[1].endswith("lanes 64-127"), out.stderr
        assert sites[0].split(": lanes")[0] != sites[1].split(": lanes")[0]  # two different lines of harness.cpp
        out = _direct(harness, "selftest=diverged_shfl", f"wave_order={order}")
        assert out.returncode == 3 and _clean(out), (out.returncode, out.stderr[-2000:])
        assert "MISMATCHED COLLECTIVE in k_selftest<diverged_shfl>" in out.stderr and "never reach" in out.stderr
        assert any("at __shfl, " in ln and ln.endswith("lanes 0-31 64-95") for ln in out.stderr.splitlines()), out.stderr
        assert any(ln.strip() == "returned from the kernel: lanes 32-63 96-127" for ln in out.stderr.splitlines()), out.stderr


def test_scan_kernels_match_a_stable_partition(harness):
    """k_compact and k_pack_perm (1024 lanes) outside a solve, on seeded flag arrays of the sizes 0, 1, 9, 1023, 1024, 1025 and
    2500 (above 1024 a thread's chunk has 2 or 3 elements and the last threads' chunks are empty) with the patterns all finished,
    none finished, alternating, only the last element unfinished and random: dst / ndst and perm / act / nact exactly those of a
    plain stable partition written in the harness, every array at its exact size (dst has as many entries as there are
    unfinished elements), in both wavefront orders."""
    outs = [_direct(harness, "scan", f"wave_order={order}") for order in ("asc", "desc")]
    for out in outs:
        assert out.returncode == 0 and _clean(out) and "MISMATCH" not in out.stdout + out.stderr, (out.stdout[-2000:], out.stderr[-2000:])
    assert outs[0].stdout == outs[1].stdout
    lines = outs[0].stdout.splitlines()
    for kern in ("k_compact", "k_pack_perm"):
        for n in (0, 1, 9, 1023, 1024, 1025, 2500):
            for pattern in ("all_finished", "none_finished", "alternating", "last_unfinished", "random"):
                assert sum(ln.startswith(f"{kern} n={n} {pattern} ") and ln.endswith(" ok") for ln in lines) == 1, (kern, n, pattern)
    assert len(lines) == 70
    count = {ln.split()[1] + " " + ln.split()[2]: int(ln.split()[3].split("=")[1]) for ln in lines if ln.startswith("k_compact")}
    assert count["n=2500 none_finished"] == 2500 and count["n=2500 all_finished"] == 0 and count["n=1025 alternating"] == 513
    assert count["n=1025 last_unfinished"] == 1 and count["n=0 none_finished"] == 0


# ---------------------------------------------------------------------------------------------------- k_riccati1q, k_step1
CASES = [(8, 1), (2, 2), (11, 1)]  # (N, ticks): the warm tick (u_prev != 0, warm start) at the cheapest horizon, and at N = 8 below


@pytest.mark.parametrize("any_bounds", [0, 1])
@pytest.mark.parametrize("N,ticks", CASES)
def test_four_wavefront_riccati_matches_the_one_wavefront_forms_and_the_oracle(mruns, oracle, batch, N, ticks, any_bounds):
    """riccati=1q: k_riccati1q with one 256-lane workgroup per listed instance, exact-size dynamic LDS, it_index / max_sweeps as
    launch_iteration_t passes them.  Status, iterations, u0 and E0 bit for bit those of k_riccati1 and k_riccati8; each of the
    three against the oracle."""
    rq = mruns(N, ticks, any_bounds, riccati="1q")
    r1 = mruns(N, ticks, any_bounds, both=False, riccati="1")
    r8 = mruns(N, ticks, any_bounds, both=False, riccati="8")
    assert same_bits(rq, r1, PRINTED) and same_bits(rq, r8, PRINTED)
    for r in (rq, r1, r8):
        check_against_oracle(oracle, r, batch, N)


@pytest.mark.parametrize("any_bounds", [0, 1])
@pytest.mark.parametrize("N,ticks", CASES)
def test_fused_step_selection_matches_the_separate_launches(mruns, oracle, batch, N, ticks, any_bounds):
    """step=1: k_step1 with one 320-lane workgroup per listed instance instead of k_linesearch / k_pick / k_linesearch / k_pick /
    k_update, both bound-pattern instantiations: every printed value bit for bit that of the separate launches."""
    fused = mruns(N, ticks, any_bounds, riccati="1q", step=1)
    assert same_bits(fused, mruns(N, ticks, any_bounds, riccati="1q"))
    check_against_oracle(oracle, fused, batch, N)


def test_warm_tick_through_the_multi_wavefront_kernels(mruns, oracle, batch):
    """N = 8, a cold and a warm tick through k_riccati1q and k_step1 together: against the oracle and bit for bit against
    k_riccati1 with the separate launches."""
    both = mruns(8, 2, riccati="1q", step=1)
    assert same_bits(both, mruns(8, 2, both=False, riccati="1"))
    check_against_oracle(oracle, both, batch, 8)


@pytest.mark.parametrize("N,ticks", [(2, 2), (11, 1)])
def test_per_instance_rows_through_the_multi_wavefront_kernels(mruns, orc, pkg, tables, batch, N, ticks):
    """The interleaved rows of test_host_harness_wave.py through k_riccati1q_pi and k_step1_pi: bit for bit the run with
    k_riccati1_pi and the separate _pi launches, each instance's line bit for bit its line in the uniform run made with its row
    (the uniform kernels), and each row's subset against the oracle created with those params."""
    rows, ia, ib = theta_rows(pkg, len(batch))
    mixed = mruns(N, ticks, rows=rows, riccati="1q", step=1)
    assert same_bits(mixed, mruns(N, ticks, rows=rows, both=False, riccati="1"))
    for theta, idx in ((THETA_A, ia), (THETA_B, ib)):
        uni = mruns(N, ticks, both=False, args=tuple(f"param.{k}={v!r}" for k, v in theta.items()), riccati="1")
        for a, b in zip(mixed, uni):
            assert np.array_equal(a[idx], b[idx]), (theta, a[idx], b[idx])
        check_against_oracle(orc.Oracle(tables.packed(), params=oracle_params(orc, theta)), mixed, batch, N, subset=idx, min_solved=3)


def test_fused_step_selection_with_soft_constraints(harness, tmp_path, orc, pkg, tables):
    """The elastic planes (options.soft_rho = 100) through k_step1: the small case of test_host_harness.py, against the oracle and
    bit for bit against the separate launches, in both wavefront orders."""
    N = 6
    x0 = pkg.sample_x0(tables, 4, seed=62)
    res = [_run(harness, tmp_path, tables, x0, N, soft_rho=100.0, ticks=1, riccati="8", args=a)
           for a in (("step=1", "wave_order=asc"), ("step=1", "wave_order=desc"), ())]
    assert same_bits(res[0], res[1]) and same_bits(res[0], res[2])
    o = orc.default_options(); o.soft_rho = 100.0
    ref = orc.Oracle(tables.packed(), options=o).solve(x0, N, nthreads=4)
    assert np.all(np.isfinite(res[0][0])) and np.array_equal(res[0][0][:, STATUS].astype(int), ref["status"])
    assert np.abs(res[0][0][:, U0] - ref["u0"]).max() < 1e-6


def test_fused_step_selection_with_the_friction_ellipse(harness, tmp_path, orc, pkg, tables):
    """The friction-ellipse constraints (k_step1<., true>): the small case of test_host_harness.py, likewise."""
    N = 6
    x0 = pkg.sample_x0(tables, 4, seed=63)
    ell = (10.0, 5.0, 0.8 * 4905.0, 0.8 * 4905.0)
    res = [_run(harness, tmp_path, tables, x0, N, ticks=1, ell=ell, riccati="8", args=a)
           for a in (("step=1", "wave_order=asc"), ("step=1", "wave_order=desc"), ())]
    assert same_bits(res[0], res[1]) and same_bits(res[0], res[2])
    p = orc.default_params(); p.ell_penalty, p.ell_rho, p.ell_D_f, p.ell_D_r = ell
    ref = orc.Oracle(tables.packed(), params=p).solve(x0, N, nthreads=4)
    assert np.all(np.isfinite(res[0][0])) and np.array_equal(res[0][0][:, STATUS].astype(int), ref["status"])
    ok = ref["status"] == 0
    assert ok.sum() >= 3 and np.abs(res[0][0][:, U0] - ref["u0"])[ok].max() < 1e-6


def test_second_pass_of_the_fused_step_selection(mruns, oracle, pkg):
    """N = 41, the first horizon at which N * n_linesearch = 328 exceeds k_step1's 320 lanes, so that its candidate loop makes a
    second, partial pass (and d_riccati1q's staging loop five rounds and a remainder of one): B = 2, the reference's x0 and the
    restoration state, one cold tick, against the oracle and bit for bit against the separate launches."""
    from test_host_harness_wave import RESTORATION_STATE
    N = 41
    x0 = np.array([pkg.X0_REFERENCE, RESTORATION_STATE])
    fused = mruns(N, 1, x0=x0, riccati="1q", step=1)
    assert same_bits(fused, mruns(N, 1, x0=x0, both=False, riccati="1"))
    check_against_oracle(oracle, fused, x0, N, min_solved=2)


# ---------------------------------------------------------------------------------------------------- compaction, packing, rollout
def test_list_compacted_by_the_kernel_does_not_change_a_bit(mruns):
    """compact=kernel: after every iteration the instance list is made by k_compact itself (ping-pong lists as in
    ltompc_make_step_dev), the launches are k_riccati1q and k_step1 over that list: bit for bit the run with the host loop of
    compact=1 (k_riccati1, separate launches) and the identity-list run.  One cold tick: every iteration after the first
    instance has finished runs on a compacted list."""
    kern = mruns(8, 1, riccati="1q", step=1, compact="kernel")
    assert same_bits(kern, mruns(8, 1, both=False, riccati="1", compact=1))
    assert same_bits(kern, mruns(8, 1, riccati="1q", step=1))


@pytest.mark.parametrize("with_rows", [False, True])
def test_repacked_instances_do_not_change_a_bit(mruns, pkg, batch, with_rows):
    """pack=1 pack_min=4: by the library's rule (at most 6 / 8 of the launch unfinished) the instances are moved with k_pack_perm
    and both passes of k_pack while the launch is wider than 4, the list is compacted by k_compact below that; x0 in and u0 out
    through `orig`; the second tick starts from the packed order; at the end k_pack_inverse and k_pack restore the caller's
    order.  Two ticks and the state left behind (x0, u_prev, last node, E0, orig) bit for bit those of the run that never moves
    anything: st, si, filt, x0, uprev and orig travel with their instance, the restoration and the off-track instance among them.
    With rows, TH stays in the caller's order and is read through orig."""
    rows = theta_rows(pkg, len(batch))[0] if with_rows else None
    packed = mruns(8, 2, rows=rows, riccati="8", pack=1, pack_min=4, final=1)
    plain = mruns(8, 2, rows=rows, both=False, riccati="8", final=1)
    assert packed[2][0, -1] >= 2 and plain[2][0, -1] == 0, packed[2][:, -1]  # instances were moved, in both ticks or twice in one
    assert same_bits(packed[:2], plain[:2]) and np.array_equal(packed[2][:, :-1], plain[2][:, :-1])
    assert np.array_equal(packed[2][:, -10], np.arange(len(batch)))  # orig is the identity again


@pytest.mark.parametrize("with_rows", [False, True])
def test_rollout_kernels_reproduce_the_synchronous_ticks(mruns, pkg, batch, with_rows):
    """rollout=3: k_roll_begin, then per pass k_roll_mark, k_roll_init (_pi), the iteration (k_riccati1q, k_step1), k_roll_finish,
    k_roll_plant (_pi) on the pass's list and k_compact on SI_FINAL by the library's rule - ltompc_rollout_dev's loop on one
    stream.  The logs (status, iterations, u0 per tick) and the state left behind bit for bit those of three synchronous ticks."""
    N = 2 if with_rows else 8
    rows = theta_rows(pkg, len(batch))[0] if with_rows else None
    roll = mruns(N, 3, rows=rows, riccati="1q", step=1, rollout=3, final=1)
    sync = mruns(N, 3, rows=rows, both=False, riccati="1", final=1)  # (k_riccati1 and the separate launches: one wavefront each)
    assert same_bits(roll[:3], sync[:3], LOGGED)
    assert np.array_equal(roll[3], sync[3])
