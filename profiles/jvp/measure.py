"""Cost of the directional pass and of the autograd layer: N = 40, batch 8192 (sampled x0) and batch 1 (X0_REFERENCE), warm ticks.
After each solve, in turn by tick: jvp_dev computed fresh (it factorises and condenses) and once more (everything present), or
jvp_dev after both forward passes; dp alone; and the forward-trajectory route to the same numbers - the trajectory host calls plus
the numpy contraction - on the last ticks.  Then the layer: mpc_solve forward + backward of a quadratic loss against the raw
make_step_dev + prediction_dev + adjoint_dev calls it is made of.  Wall times in ms, host-synchronised, medians.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o jvp -- python profiles/jvp/measure.py [wall.json]"""
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
layer = importlib.import_module("lap-time-optimization_amd.autograd")
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
    dp, dth = rng.standard_normal((B, 10)), rng.uniform(-0.05, 0.05, (B, 16)) * mpc.theta()
    dpd, dthd = torch.from_numpy(dp).to(dev), torch.from_numpy(dth).to(dev)
    g10 = torch.zeros(B, 2, 10, dtype=torch.float64, device=dev)
    g16 = torch.zeros(B, 2, 16, dtype=torch.float64, device=dev)
    tX = torch.zeros(B, N + 1, 8, dtype=torch.float64, device=dev)
    tU = torch.zeros(B, N, 2, dtype=torch.float64, device=dev)
    ok = torch.zeros(B, dtype=torch.int32, device=dev)
    mpc.set_initial_guess_dev(xd.data_ptr())
    keys = ("solve", "jvp_fresh", "jvp_again", "sens_dev", "psens_dev", "jvp_after_forward", "jvp_dp_only", "fwd_traj_host", "fwd_contract",
            "jvp_host")
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
        if tick % 2 == 0:  # the directional pass first: it makes the factorisation, ok and the PV planes
            timed("jvp_fresh", lambda: mpc.jvp_dev(dpd.data_ptr(), dthd.data_ptr(), tX.data_ptr(), tU.data_ptr(), ok.data_ptr()), keep)
            timed("jvp_again", lambda: mpc.jvp_dev(dpd.data_ptr(), dthd.data_ptr(), tX.data_ptr(), tU.data_ptr(), ok.data_ptr()), keep)
        else:  # the two forward passes (du0 only on the device), then the directional pass on what they left
            timed("sens_dev", lambda: mpc.sensitivities_dev(g10.data_ptr(), ok.data_ptr()), keep)
            timed("psens_dev", lambda: mpc.param_sensitivities_dev(g16.data_ptr(), ok.data_ptr()), keep)
            timed("jvp_after_forward", lambda: mpc.jvp_dev(dpd.data_ptr(), dthd.data_ptr(), tX.data_ptr(), tU.data_ptr(), ok.data_ptr()), keep)
            timed("jvp_dp_only", lambda: mpc.jvp_dev(dpd.data_ptr(), 0, tX.data_ptr(), tU.data_ptr(), 0), keep)
        if tick >= 20:
            J = timed("jvp_host", lambda: mpc.jvp(dp, dth), True)
            S, P = timed("fwd_traj_host", lambda: (mpc.sensitivities(trajectory=True), mpc.param_sensitivities(trajectory=True)), True)
            t0 = time.perf_counter()
            fX = np.einsum("bkij,bj->bki", S["dX"], dp) + np.einsum("bkij,bj->bki", P["dX"], dth)
            fU = np.einsum("bkij,bj->bki", S["dU"], dp) + np.einsum("bkij,bj->bki", P["dU"], dth)
            t["fwd_contract"].append(time.perf_counter() - t0)
            dX = np.einsum("bkij,bj->bki", np.abs(S["dX"]), np.abs(dp)) + np.einsum("bkij,bj->bki", np.abs(P["dX"]), np.abs(dth))
            dU = np.einsum("bkij,bj->bki", np.abs(S["dU"]), np.abs(dp)) + np.einsum("bkij,bj->bki", np.abs(P["dU"]), np.abs(dth))
    out[B] = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    out[B]["ok_fraction"] = float(J["ok"].mean())
    err = np.concatenate([(np.abs(J["tX"] - fX) / np.where(dX > 0, dX, 1.0)).reshape(B, -1),
                          (np.abs(J["tU"] - fU) / np.where(dU > 0, dU, 1.0)).reshape(B, -1)], axis=1).max(axis=1)  # tests/test_gpu_jvp.py's measure
    out[B]["error_to_forward_max"], out[B]["error_to_forward_median"] = float(err.max()), float(np.median(err))
    # the layer against the calls it is made of (u_prev and theta left to the handle; a loss of the whole prediction)
    Xd, Ud = torch.zeros(B, N + 1, 8, dtype=torch.float64, device=dev), torch.zeros(B, N, 2, dtype=torch.float64, device=dev)
    gp = torch.zeros(B, 10, dtype=torch.float64, device=dev)
    tl = {"layer_forward_backward": [], "raw_solve_prediction_adjoint": []}
    for tick in range(12):
        x0 = xd.clone().requires_grad_(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u0, X, U, _ = layer.mpc_solve(mpc, x0)
        (0.5 * ((X * X).sum() + (U * U).sum())).backward()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mpc.make_step_dev(xd.data_ptr(), ud.data_ptr())
        mpc.prediction_dev(Xd.data_ptr(), Ud.data_ptr())
        mpc.sensitivities_dev(0, ok.data_ptr())
        mpc.adjoint_dev(Xd.data_ptr(), Ud.data_ptr(), gp.data_ptr(), 0, 0)
        mpc.synchronize()
        t2 = time.perf_counter()
        if tick >= 2:
            tl["layer_forward_backward"].append(t1 - t0), tl["raw_solve_prediction_adjoint"].append(t2 - t1)
    out[B].update({k: 1e3 * float(np.median(v)) for k, v in tl.items()})
    mpc.close()
print(json.dumps(out, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
