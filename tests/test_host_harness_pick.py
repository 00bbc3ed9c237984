"""d_pick's filter (csrc/linesearch.h) on the sanitizer harnesses.  d_pick holds the filter in registers and, when an accepted
step augments a full filter (nfilt == FILTER_MAX), writes the pairs 1 .. FILTER_MAX - 1 from those registers one row down and
appends the new pair: the one place where the stored data no longer comes from the memory it goes back to.

test_filter_plane_after_one_launch looks at the filter itself.  tests/host_harness/pick_harness.cpp runs ONE launch of k_pick
(phase 0) on seeded state and prints, per instance, the whole filter plane and the state d_pick may write; the expectation is
restated here from the rule (Waechter & Biegler 2006, eqs. 18 - 20, with this solver's constants), in plain Python on the numbers
of the file.  Every seeded number is a multiple of 2^-10 small enough that the sums over the horizon are exact in any order, so
the comparison is bit for bit.  Cases: a full filter augmented (shift + append), 15 pairs (append, no shift), first test of a
solve (theta0 < 0: the filter restarts), a few pairs, a candidate dominated by the LAST pair of a full filter (rejected: nothing
but SI_LSMORE and the list of rejected steps may change), a full filter with switching condition and Armijo (accepted, filter
untouched), theta above theta_max, a scaled penalty, a full filter at the first test; at N = 10 and at N = 41 (a stage beyond
the 40 of the first batch of loads).  Writing pair f instead of pair f + 1 in the shift fails this test.

test_full_filter_through_pick_and_step1: the first eight states of tests/test_gpu_pick_paths.py (N = 10) through whole solves.
Instance 3 ends STALLED after 101 iterations and two restoration phases; its solve goes through the full-filter branch (seen with
a print in a scratch copy of d_pick; this test cannot see the filter and does not claim to).  The run through k_pick and the run
through k_step1 (both wavefront orders) must agree bit for bit, and with the oracle, with ASan watching the plane W.filt, which is
allocated at its exact size."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pick_paths import _states
from test_host_harness import _run, harness  # noqa: F401  (the fixture that builds the executable)
from test_host_harness_wave import ITERS, STATUS, U0, same_bits

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")
EXE = os.path.join(HARNESS_DIR, "pick_harness")
FILTER_MAX = 16
G_TH, G_PH, ETA_PH, S_TH, S_PH = 1e-5, 1e-8, 1e-8, 1.1, 2.3  # the constants of the filter rule (linesearch.h)


@pytest.fixture(scope="module")
def pick_harness():
    srcs = [os.path.join(HARNESS_DIR, f) for f in ("pick_harness.cpp", "hip_shim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    srcs.append(os.path.join(ROOT, "include", "ltompc.h"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLTOMPC_HOST_HARNESS",
                               "-I", CSRC, "-I", HARNESS_DIR, os.path.join(HARNESS_DIR, "pick_harness.cpp"), "-o", EXE, "-lpthread"])
    return EXE


def _grid(rng, lo, hi, n):
    """n multiples of 2^-10 in [lo, hi)."""
    return rng.integers(int(lo * 1024), int(hi * 1024), n) / 1024.0


def _cases(N, rng):
    """Per instance: dict(nfilt, theta0, thmax, thmin, mu, c00, rho, filt (2 FILTER_MAX, pair f = rows 2f, 2f + 1), SP (3, N), LS (6, N))."""
    out = []
    for kind in ("full", "fifteen", "first", "few", "dominated_by_last", "switching", "above_theta_max", "scaled", "full_first"):
        c = dict(mu=0.125, c00=_grid(rng, 1, 4, 1)[0], rho=4000.0 if kind == "scaled" else 0.0, theta0=8.0, thmax=8e4, thmin=8e-4)
        th0k = _grid(rng, 0.5, 2.0, N)
        LS = np.stack([th0k, _grid(rng, 0, 3, N), _grid(rng, -2, 2, N), th0k / 2, _grid(rng, 0, 3, N), _grid(rng, -2, 2, N)])
        SP = np.stack([np.full(N, 1.0), np.full(N, 1.0), _grid(rng, 0.25, 1.0, N)])  # gphid > 0: no switching condition
        SP[0, N // 2], SP[1, N - 1] = 0.75, 0.5                                        # the minima a_pri, a_dua
        c["nfilt"] = {"full": 16, "fifteen": 15, "first": 0, "few": 3, "dominated_by_last": 16, "switching": 16, "above_theta_max": 5,
                      "scaled": 16, "full_first": 16}[kind]
        filt = np.empty(2 * FILTER_MAX)
        filt[0::2], filt[1::2] = _grid(rng, 0.125, 64, FILTER_MAX), 1000.0 + _grid(rng, 0, 64, FILTER_MAX)  # (phi far above: no pair dominates)
        th1, ph1 = LS[3].sum(), (c["c00"] + LS[4].sum()) - c["mu"] * LS[5].sum()
        if kind in ("first", "full_first"):
            c["theta0"] = -1.0
        if kind == "dominated_by_last":
            filt[2 * 15], filt[2 * 15 + 1] = th1 / 2, ph1 - 1.0
        if kind == "switching":
            SP[2] = -0.75            # gphid = -0.75 N: alpha (-gphid)^2.3 > theta^1.1
            LS[4] = LS[1] - 1.0      # ... and Armijo holds
        if kind == "above_theta_max":
            c["thmax"] = th1 / 2
        c.update(filt=filt, SP=SP, LS=LS, kind=kind)
        out.append(c)
    return out


def _expected(c):
    """The filter rule on one instance, phase 0 (only the full step is tried): what memory holds afterwards."""
    SP, LS = c["SP"], c["LS"]
    S = c["rho"] / 1000.0 if c["rho"] > 1000.0 else 1.0
    a_pri, a_dua, gphid = min(1.0, SP[0].min()), min(1.0, SP[1].min()), SP[2].sum()
    th0, ph0 = LS[0].sum(), (c["c00"] + LS[1].sum()) - c["mu"] * LS[2].sum()
    th1, ph1 = LS[3].sum(), (c["c00"] + LS[4].sum()) - c["mu"] * LS[5].sum()
    nfilt, theta0, thmax, thmin = c["nfilt"], c["theta0"], c["thmax"], c["thmin"]
    filt = c["filt"].copy()
    filt[2 * nfilt:] = np.nan   # (what the harness leaves there)
    first = theta0 < 0.0
    if first:
        theta0, thmax, thmin, nfilt = th0, 1e4 * max(1.0, th0), 1e-4 * max(1.0, th0), 0
    accepted = False
    if th1 <= thmax and not any(th1 >= filt[2 * f] and ph1 >= filt[2 * f + 1] for f in range(nfilt)):
        sw = gphid < 0.0 and a_pri * (-gphid * (1.0 / S)) ** S_PH > th0 ** S_TH
        armijo = ph1 <= ph0 + ETA_PH * a_pri * gphid
        accepted = armijo if (th0 <= thmin and sw) else (th1 <= (1.0 - G_TH) * th0 or ph1 <= ph0 - G_PH * S * th0)
        if accepted and not (sw and armijo):
            if nfilt == FILTER_MAX:
                filt[:-2] = filt[2:].copy()
                nfilt -= 1
            filt[2 * nfilt], filt[2 * nfilt + 1] = (1.0 - G_TH) * th0, ph0 - G_PH * S * th0
            nfilt += 1
    if accepted:   # nfilt lsmore step iters ntiny nlsfail skip_eval | alpha adua force_reg
        ints, dbl = [nfilt, 0, 1, 8, 0, 0, 0], [a_pri, a_dua, 0.0]
    else:          # nothing has been modified: phase 1 decides
        ints, dbl = [c["nfilt"], 1, 1, 7, 3, 0, -7], [-7.0, -7.0, 0.5]
    # (theta0 and its limits: written at the first test of a solve, whatever follows)
    return accepted, np.array(ints), np.array(dbl + ([theta0, thmax, thmin] if first else [c["theta0"], c["thmax"], c["thmin"]])), filt


@pytest.mark.parametrize("N", [10, 41])
def test_filter_plane_after_one_launch(pick_harness, tmp_path, N):
    cases = _cases(N, np.random.default_rng(606 + N))
    prob = tmp_path / "pick.txt"
    with open(prob, "w") as f:
        f.write(f"{len(cases)} {N}\n")
        for c in cases:
            row = np.concatenate([[c["nfilt"], c["theta0"], c["thmax"], c["thmin"], c["mu"], c["c00"], c["rho"]], c["filt"], c["SP"].ravel(), c["LS"].ravel()])
            np.savetxt(f, row[None], fmt="%.17g")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([pick_harness, str(prob)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr and "MISMATCHED" not in out.stderr, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) + 1
    rejected, n_shift = [], 0
    for b, (c, line) in enumerate(zip(cases, lines)):
        w = line.split()
        assert w[0] == "inst" and int(w[1]) == b
        ints, dbl, filt = np.array([int(v) for v in w[2:9]]), np.array([float(v) for v in w[9:15]]), np.array([float(v) for v in w[15:]])
        accepted, e_ints, e_dbl, e_filt = _expected(c)
        assert filt.size == 2 * FILTER_MAX
        assert np.array_equal(ints, e_ints), (c["kind"], ints, e_ints)
        assert np.array_equal(dbl, e_dbl), (c["kind"], dbl, e_dbl)
        assert np.array_equal(filt, e_filt, equal_nan=True), (c["kind"], filt, e_filt)
        if not accepted:
            rejected.append(b)
        n_shift += int(accepted and c["nfilt"] == FILTER_MAX and c["theta0"] >= 0.0 and not np.array_equal(e_filt, c["filt"]))
    # the cases are what they are meant to be: two full filters shifted, two candidates rejected, one accepted without augmenting
    kinds = [c["kind"] for c in cases]
    assert n_shift == 2 and [kinds[b] for b in rejected] == ["dominated_by_last", "above_theta_max"]
    sw = cases[kinds.index("switching")]
    assert _expected(sw)[0] and np.array_equal(_expected(sw)[3], sw["filt"])
    got = [int(v) for v in lines[-1].split()[1:]]
    assert lines[-1].startswith("list ") and got[0] == len(rejected) and sorted(got[1:]) == rejected


def test_full_filter_through_pick_and_step1(harness, tmp_path, oracle, pkg, tables):  # noqa: F811
    N = 10
    x0 = _states(pkg, tables)[:8]
    res = [_run(harness, tmp_path, tables, x0, N, ticks=1, riccati="8", args=a)
           for a in ((), ("step=1", "wave_order=asc"), ("step=1", "wave_order=desc"))]
    assert all(len(r) == 1 and np.all(np.isfinite(r[0])) for r in res)
    assert same_bits(res[0], res[1]) and same_bits(res[1], res[2])
    ref = oracle.solve(x0, N, nthreads=4)
    r = res[0][0]
    # the scenario is the one described above: the long solve with its failed line searches and restoration phases is there
    assert ref["status"][3] == 4 and ref["iters"][3] >= 100 and ref["n_resto"][3] == 2 and ref["n_lsfail"][3] >= 1
    assert np.array_equal(r[:, STATUS].astype(int), ref["status"]), (r[:, STATUS], ref["status"])
    ok = ref["status"] == 0
    assert ok.sum() == 7 and np.abs(r[:, U0] - ref["u0"])[ok].max() < 1e-6
    assert (np.abs(r[:, ITERS] - ref["iters"]) <= 2).all(), (r[:, ITERS], ref["iters"])
