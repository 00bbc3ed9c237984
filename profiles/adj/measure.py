"""Cost of the adjoint pass: N = 40, batch 8192 (sampled x0) and batch 1 (X0_REFERENCE), warm ticks.  After each solve, in turn
by tick: adjoint_dev computed fresh (it factorises and condenses), or adjoint_dev after both forward passes (factorisation and
PV planes present); grad_p alone; prediction_dev; and the forward route to the same 26 numbers per instance - sensitivities_dev
+ param_sensitivities_dev (du0 only), and on the last ticks the trajectory host calls plus the numpy contraction.  Wall times in
ms, host-synchronised, medians.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o adj -- python profiles/adj/measure.py [wall.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("lap-time-optimization_amd")
tables = pkg.TrackTables.load_npz(os.path.join(ROOT, "tests", "golden", "tables_buckmore_mx5_curvature.npz"))
out = {}
dev = torch.device("cuda", 0)
N = 40
for B in (8192, 1):
    x = pkg.X0_REFERENCE[None].copy() if B == 1 else pkg.sample_x0(tables, B, seed=1)
    mpc = pkg.BatchedMPC(tables, N, B)
    xd = torch.from_numpy(x).to(dev)
    ud = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(2)
    gX, gU = rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))
    gXd, gUd = torch.from_numpy(gX).to(dev), torch.from_numpy(gU).to(dev)
    g10 = torch.zeros(B, 2, 10, dtype=torch.float64, device=dev)
    g16 = torch.zeros(B, 2, 16, dtype=torch.float64, device=dev)
    gp = torch.zeros(B, 10, dtype=torch.float64, device=dev)
    gt = torch.zeros(B, 16, dtype=torch.float64, device=dev)
    Xd = torch.zeros(B, N + 1, 8, dtype=torch.float64, device=dev)
    Ud = torch.zeros(B, N, 2, dtype=torch.float64, device=dev)
    ok = torch.zeros(B, dtype=torch.int32, device=dev)
    mpc.set_initial_guess_dev(xd.data_ptr())
    keys = ("solve", "adj_fresh", "adj_again", "sens_dev", "psens_dev", "adj_after_forward", "adj_p_only", "prediction_dev",
            "fwd_traj_host", "fwd_contract", "adj_host")
    t = {k: [] for k in keys}

    def timed(key, fn, keep):
        t0 = time.perf_counter()
        r = fn()
        mpc.synchronize()
        if keep:
            t[key].append(time.perf_counter() - t0)
        return r

    for tick in range(24):
        keep = tick >= 4
        timed("solve", lambda: mpc.make_step_dev(xd.data_ptr(), ud.data_ptr()), keep)
        timed("prediction_dev", lambda: mpc.prediction_dev(Xd.data_ptr(), Ud.data_ptr()), keep)
        if tick % 2 == 0:  # the adjoint first: it makes the factorisation, ok and the PV planes
            timed("adj_fresh", lambda: mpc.adjoint_dev(gXd.data_ptr(), gUd.data_ptr(), gp.data_ptr(), gt.data_ptr(), ok.data_ptr()), keep)
            timed("adj_again", lambda: mpc.adjoint_dev(gXd.data_ptr(), gUd.data_ptr(), gp.data_ptr(), gt.data_ptr(), ok.data_ptr()), keep)
        else:  # the forward route to the same numbers (du0 only on the device), then the adjoint on what it left
            timed("sens_dev", lambda: mpc.sensitivities_dev(g10.data_ptr(), ok.data_ptr()), keep)
            timed("psens_dev", lambda: mpc.param_sensitivities_dev(g16.data_ptr(), ok.data_ptr()), keep)
            timed("adj_after_forward", lambda: mpc.adjoint_dev(gXd.data_ptr(), gUd.data_ptr(), gp.data_ptr(), gt.data_ptr(), ok.data_ptr()), keep)
            timed("adj_p_only", lambda: mpc.adjoint_dev(gXd.data_ptr(), gUd.data_ptr(), gp.data_ptr(), 0, 0), keep)
        if tick >= 20:
            A = timed("adj_host", lambda: mpc.adjoint(gX, gU), True)
            S, P = timed("fwd_traj_host", lambda: (mpc.sensitivities(trajectory=True), mpc.param_sensitivities(trajectory=True)), True)
            t0 = time.perf_counter()
            fp = np.einsum("bki,bkij->bj", gX, S["dX"]) + np.einsum("bkc,bkcj->bj", gU, S["dU"])
            ft = np.einsum("bki,bkij->bj", gX, P["dX"]) + np.einsum("bkc,bkcj->bj", gU, P["dU"])
            t["fwd_contract"].append(time.perf_counter() - t0)
            dp = np.einsum("bki,bkij->bj", np.abs(gX), np.abs(S["dX"])) + np.einsum("bkc,bkcj->bj", np.abs(gU), np.abs(S["dU"]))
            dt = np.einsum("bki,bkij->bj", np.abs(gX), np.abs(P["dX"])) + np.einsum("bkc,bkcj->bj", np.abs(gU), np.abs(P["dU"]))
    out[B] = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    out[B]["ok_fraction"] = float(A["ok"].mean())
    got, want = np.concatenate([A["grad_x0"], A["grad_uprev"], A["grad_theta"]], axis=1), np.concatenate([fp, ft], axis=1)
    den = np.concatenate([dp, dt], axis=1)
    err = (np.abs(got - want) / np.where(den > 0, den, 1.0)).max(axis=1)  # the measure of tests/test_gpu_adjoint.py, per instance
    out[B]["error_to_forward_max"], out[B]["error_to_forward_median"] = float(err.max()), float(np.median(err))
    mpc.close()
print(json.dumps(out, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
