"""Cost and use of the per-instance warm-start calls on one MI355X, N = 40, batch 8192.

    python profiles/warm_state/measure.py time [out.json]   reset of 1 % and of 100 % of the instances against set_initial_guess;
                                                            export and import of all instances (bytes moved, bytes/s).  Wall times
                                                            in ms, host-synchronised, medians of 20; kernel times come from
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ws -- python profiles/warm_state/measure.py time
    python profiles/warm_state/measure.py loop [out.json]   a closed loop of 60 ticks, once as it is and once re-seeding every
                                                            instance whose solver status is INFEASIBLE to a fresh sample_x0 state
                                                            with reset(): solved fraction and ms per tick of both"""
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
dev = torch.device("cuda", 0)
N, B = 40, 8192
what = sys.argv[1] if len(sys.argv) > 1 else "time"
out = {}


def med_ms(mpc, fn, n=20):
    t = []
    for _ in range(n):
        mpc.synchronize()
        t0 = time.perf_counter()
        fn()
        mpc.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


if what == "time":
    x0 = pkg.sample_x0(tables, B, seed=1)
    mpc = pkg.BatchedMPC(tables, N, B)
    xd, xn = torch.from_numpy(x0).to(dev), torch.zeros(B, 8, dtype=torch.float64, device=dev)
    ud = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    S = mpc.warm_state_size
    blob = torch.zeros(B, S, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(3)
    m1 = np.zeros(B, dtype=np.int32)
    m1[rng.choice(B, B // 100, replace=False)] = 1
    mask1, mask100 = torch.from_numpy(m1).to(dev), torch.ones(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    mpc.set_initial_guess_dev(xd.data_ptr())
    for _ in range(3):  # a warm, packed handle
        mpc.make_step_dev(xd.data_ptr(), ud.data_ptr())
        mpc.plant_step_dev(xd.data_ptr(), ud.data_ptr(), xn.data_ptr())
        mpc.synchronize()
        xd.copy_(xn)
        torch.cuda.synchronize(dev)
    for packed in (True, False):
        if not packed:
            mpc.iterate()  # an accessor: back to the caller's order
        tag = "packed" if packed else "unpacked"
        out[f"export_all_ms_{tag}"] = med_ms(mpc, lambda: mpc.export_state_dev(0, B, blob.data_ptr()))
        out[f"import_all_ms_{tag}"] = med_ms(mpc, lambda: mpc.import_state_dev(0, B, blob.data_ptr()))
        out[f"reset_1pct_ms_{tag}"] = med_ms(mpc, lambda: mpc.reset_dev(mask1.data_ptr(), xd.data_ptr()))
        mpc.import_state_dev(0, B, blob.data_ptr())  # (the warm start again)
    out["reset_100pct_ms"] = med_ms(mpc, lambda: mpc.reset_dev(mask100.data_ptr(), xd.data_ptr()))
    out["set_initial_guess_ms"] = med_ms(mpc, lambda: mpc.set_initial_guess_dev(xd.data_ptr()))
    out["blob_bytes_per_instance"], out["blob_bytes"] = 8 * S, 8 * S * B
    mpc.close()
else:
    T = 60
    fresh = pkg.sample_x0(tables, B * 4, seed=11)
    for reseed in (False, True):
        x0 = pkg.sample_x0(tables, B, seed=1)
        mpc = pkg.BatchedMPC(tables, N, B)
        xd, xn = torch.from_numpy(x0).to(dev), torch.zeros(B, 8, dtype=torch.float64, device=dev)
        ud = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        mpc.set_initial_guess_dev(xd.data_ptr())
        solved, infeasible, ms, ms_reset, n_reset, used = [], [], [], [], [], 0
        for t in range(T):
            mpc.synchronize()
            t0 = time.perf_counter()
            mpc.make_step_dev(xd.data_ptr(), ud.data_ptr())
            mpc.plant_step_dev(xd.data_ptr(), ud.data_ptr(), xn.data_ptr())
            mpc.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            xd.copy_(xn)
            torch.cuda.synchronize(dev)
            c, _ = mpc.status_counts()
            solved.append(float(c[0]) / B), infeasible.append(int(mpc.solver_status_counts()[5]))
            if reseed:
                t0 = time.perf_counter()
                bad = mpc.stats()["status_solver"] == 5
                k = int(bad.sum())
                if k:
                    xh = xd.cpu().numpy()
                    xh[bad] = fresh[used:used + k]
                    used = (used + k) % (3 * B)
                    mpc.reset(bad, xh)
                    xd.copy_(torch.from_numpy(xh).to(dev))
                    torch.cuda.synchronize(dev)
                ms_reset.append(1e3 * (time.perf_counter() - t0)), n_reset.append(k)
        out["reseed" if reseed else "as_today"] = dict(solved_frac_per_tick=solved, solver_infeasible_per_tick=infeasible, ms_per_tick=ms,
                                                       ms_per_tick_median=float(np.median(ms[1:])), ms_reset_per_tick=ms_reset, n_reset_per_tick=n_reset)
        mpc.close()
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
