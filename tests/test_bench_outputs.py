"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files that two builds can be compared by."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench(args, env=None, timeout=600):
    out = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_write_outputs_caps_the_size_with_a_fixed_sample(tmp_path):
    import bench
    n = 1000
    arrays = {"u0": np.arange(2 * n, dtype=np.float64).reshape(n, 2), "status": np.arange(n, dtype=np.int32)}
    bench.write_outputs(str(tmp_path), arrays, max_bytes=10 ** 9)
    assert np.array_equal(np.load(tmp_path / "u0.npy"), arrays["u0"]) and np.load(tmp_path / "status.npy").dtype == np.float64
    assert not (tmp_path / "sample_rows.npy").exists()
    cap = 8000
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), arrays, max_bytes=cap)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= cap
    for f in ("u0.npy", "status.npy", "sample_rows.npy"):  # the same rows of every array, the same sample every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), rows)
    bench.write_outputs(str(tmp_path / "a"), arrays, max_bytes=10 ** 9)  # an unsampled dump leaves no stale sample index behind
    assert not (tmp_path / "a" / "sample_rows.npy").exists()


@pytest.mark.parametrize("gpus", [1, 2])
def test_dump_outputs_holds_the_last_timed_step_of_every_rank(tmp_path, gpus):
    """The stand-in solver of --selftest-stub writes row + k into the controls of step k: the dump has every rank's rows of
    step K - 1, so --steps K set the number of timed steps."""
    env = dict(os.environ, MASTER_PORT=str(29561 + gpus), OMP_NUM_THREADS="1")
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    r = _bench(["--gpus", str(gpus), "--steps", "4", "--warmup", "1", "--batch", "50", "--selftest-stub", "--dump-outputs", str(tmp_path)], env=env)
    assert r["steps"] == 4 and r["n_gpus"] == gpus
    u0 = np.load(tmp_path / "u0.npy")
    assert u0.dtype == np.float64 and np.array_equal(u0, np.repeat(np.arange(50.0 * gpus)[:, None], 2, 1) + 3)


@pytest.mark.gpu
def test_dump_outputs_is_the_benchmarks_loop_and_repeats(tmp_path, pkg, gpu_lib):
    """Two runs of the same command (one handle / two split handles) dump the same bits, and those are the outputs of the
    benchmark's loop restated here: W + K ticks of make_step + plant step from the seeded states."""
    import torch
    import bench
    B, N, W, K = 256, 40, 2, 3
    common = ["--batch", str(B), "--horizon", str(N), "--warmup", str(W), "--steps", str(K), "--no-extras", "--no-cpu-baseline"]
    runs = {}
    for parts in (1, 2):
        d = tmp_path / f"parts{parts}"
        r = _bench(common + ["--parts", str(parts), "--dump-outputs", str(d)])
        assert r["steps"] == K and len(r["solved_frac_per_tick"]) == K
        runs[parts] = {k: np.load(d / f"{k}.npy") for k in ("u0", "x_next", "status", "iters")}
        assert {k: v.shape for k, v in runs[parts].items()} == {"u0": (B, 2), "x_next": (B, 8), "status": (B,), "iters": (B,)}
        st, n = np.unique(runs[parts]["status"].astype(int), return_counts=True)
        assert {bench.STATUS_NAMES[s]: int(c) for s, c in zip(st, n)} == r["status_histogram_last_tick"]
    for k in runs[1]:
        assert np.array_equal(runs[1][k], runs[2][k]), k

    tables = pkg.build_tables()
    opts = pkg.default_options()
    opts.max_iter, opts.soft_rho, opts.resto_sticky = 1000, 0.0, 0  # bench.py's defaults
    dev = torch.device("cuda", 0)
    mpc = pkg.BatchedMPC(tables, n_horizon=N, batch=B, options=opts)
    mpc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    mpc.set_poll_every(4)
    x = torch.from_numpy(pkg.sample_x0(tables, B, seed=pkg.scenarios.SEED)).to(dev)
    xn, u = torch.empty_like(x), torch.zeros(B, 2, dtype=torch.float64, device=dev)
    mpc.set_initial_guess_dev(x.data_ptr())
    for _ in range(W + K):
        mpc.make_step_dev(x.data_ptr(), u.data_ptr())
        mpc.plant_step_dev(x.data_ptr(), u.data_ptr(), xn.data_ptr(), bench.PLANT_SUBSTEPS)
        x, xn = xn, x
    torch.cuda.synchronize(dev)
    st = mpc.stats()
    mpc.close()
    assert np.array_equal(runs[1]["u0"], u.cpu().numpy()) and np.array_equal(runs[1]["x_next"], x.cpu().numpy())
    assert np.array_equal(runs[1]["status"], st["status"]) and np.array_equal(runs[1]["iters"], st["iters"])
