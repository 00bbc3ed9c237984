"""Cost of per-instance vehicle and cost parameters: N = 40, batch 8192 (sampled x0), 20 warm ticks after 4 of
warm-up, make_step_dev per tick, host-synchronised; wall ms per tick (median, min) and the iterations of the last tick.
  (a) a uniform handle;
  (b) per-instance rows all equal to the handle's values: the same bits and iterations as (a), the _pi kernels - the cost of
      reading the rows;
  (c) rows spread +-10 % in D_f, D_r and the mass (uniform random, seed 3).
The three handles are created and timed in turn, (a) (b) (c) (a) (b) (c), one at a time.

    rocprofv3 --kernel-trace --stats -d <dir> -o pinst -- python profiles/pinst/measure.py [wall.json] [a|b|c]"""
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
B, N, WARM, TICKS = 8192, 40, 4, 20
dev = torch.device("cuda", 0)
x = pkg.sample_x0(tables, B, seed=1)
only = sys.argv[2] if len(sys.argv) > 2 else None


def rows(case, th):
    if case == "a":
        return None
    r = np.tile(th, (B, 1))
    if case == "c":
        rng = np.random.default_rng(3)
        for name in ("D_f", "D_r", "mass"):
            r[:, pkg.THETA_NAMES.index(name)] *= rng.uniform(0.9, 1.1, B)
    return r


def run(case):
    mpc = pkg.BatchedMPC(tables, N, B)
    r = rows(case, mpc.theta())
    if r is not None:
        mpc.set_theta(r)
    xd = torch.from_numpy(x).to(dev)
    ud = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    mpc.set_initial_guess_dev(xd.data_ptr())
    t = []
    for tick in range(WARM + TICKS):
        t0 = time.perf_counter()
        mpc.make_step_dev(xd.data_ptr(), ud.data_ptr())
        mpc.synchronize()
        if tick >= WARM:
            t.append(time.perf_counter() - t0)
    st = mpc.stats()
    res = dict(median_ms=1e3 * float(np.median(t)), min_ms=1e3 * float(np.min(t)), iters_sum=int(st["iters"].sum()),
               u0_sum=float(ud.sum().item()))
    mpc.close()
    return res


out = {}
for rep in range(2):
    for case in ("a", "b", "c"):
        if only and case != only:
            continue
        out.setdefault(case, []).append(run(case))
print(json.dumps(out, indent=1))
if len(sys.argv) > 1 and sys.argv[1] != "-":
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
