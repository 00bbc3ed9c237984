"""Lock-step comparison of a solve's iterates with the oracle's, pass by pass.  TEST INFRASTRUCTURE ONLY.

The oracle is the same algorithm as the kernels by construction, and a solve cut by options.max_iter = k stops at
a deterministic primal-dual iterate on both sides.  So the whole iterate (X, C, U, L1, L2, T, NU) and the counters can be compared
at every k, not only at convergence, and no second implementation of a pass is needed.

How close the two must be comes from the oracle alone: the ENVELOPE env[b, k] is the largest scaled difference of any iterate
component between the oracle's run from x0 and its runs from P = 5 copies of x0 perturbed at rounding level (a relative 4e-16 on
every component, 1e-13 m on s; fixed seed).  It measures how far rounding-sized input changes move iterate k of instance b.
The device has to stay within FACTOR * max(env, ENV_FLOOR): FACTOR = 1024 covers the rounding of ~1e3 operations per stage over
N stages and k iterations (a random walk of a few hundred ulps, times a safety factor of about 5), where the envelope sees a
handful of one-off input perturbations only.  Where the reference itself is not reproducible - env[b, k] > ENV_MAX, or a
perturbation changed a status, an iteration count, n_reg, n_lsfail or mu - the pair (b, k) and every later k of that instance is
EXCLUDED; the caps on how many pairs may be excluded (none for k <= 10, at most 10 % per case) are checked on the CPU
(test_lockstep_reference.py).

Scaled difference of two iterates a, r (r the reference): max over all components of |a - r| / (1 + |r|).

Alignment of the budgets: the device counts PASSES (a sweep repeated for the inertia correction is one more pass, SI_SWEEPS), the
oracle counts ITERATIONS (its retries are free).  Instance b of a device run with budget m is therefore compared with the oracle
run whose max_iter equals the device's reported iters[b] (`aligned`), which needs the oracle's result at every k = 0 .. K."""
from __future__ import annotations

import numpy as np

COMPONENTS = ("X", "C", "U", "L1", "L2", "T", "NU")
DISCRETE = ("status", "iters", "n_reg", "n_lsfail")
STATUS_MAX_ITER = 2
P_COPIES = 5
PERTURB_REL, PERTURB_S = 4e-16, 1e-13
ENV_FLOOR, ENV_MAX, FACTOR, MU_RTOL = 1e-13, 1e-8, 1024.0, 1e-12
CAP_FIRST_K, CAP_FRACTION = 10, 0.10


def budgets(K):
    """The budgets a GPU case runs: k = 1 .. 12, then every third up to K."""
    return [k for k in range(1, K + 1) if k <= 12 or k % 3 == 0]


def factory(orc, tables, params=None, **options):
    """oracle_factory for `trajectory`: max_iter -> an Oracle over `tables` with `params` and the given options."""
    def make(max_iter):
        o = orc.default_options()
        for k, v in options.items():
            setattr(o, k, v)
        o.max_iter = int(max_iter)
        return orc.Oracle(tables.packed(), params=params, options=o)
    return make


def _tile(v, n):
    if isinstance(v, dict):
        return {k: _tile(a, n) for k, a in v.items()}
    if isinstance(v, np.ndarray):
        return np.concatenate([v] * n, axis=0)
    return v


def trajectory(oracle_factory, x0, N, budgets, **solve_kw):
    """{k: the oracle's result dict at max_iter = k} for k in budgets.  solve_kw: uprev, warm, prev_status of Oracle.solve."""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    solve_kw.setdefault("nthreads", 8)
    return {int(k): oracle_factory(int(k)).solve(x0, N, **solve_kw) for k in budgets}


def perturbed(x0, copies=P_COPIES, seed=20240611):
    """`copies` perturbed copies of x0 (B,8): every component times 1 +- 4e-16, s +- 1e-13 m, signs from a fixed seed."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(copies):
        sg = rng.choice([-1.0, 1.0], size=x0.shape)
        x = x0 * (1.0 + PERTURB_REL * sg)
        x[:, 0] += PERTURB_S * rng.choice([-1.0, 1.0], size=x0.shape[0])
        out.append(x)
    return out


def scaled_difference(a, ref):
    """Per instance: max over the iterate's components of |a - ref| / (1 + |ref|); a NaN counts as infinite.  (The slack and
    multiplier slots of the path constraints of the last stage, which has none, are compared too: both sides initialise them
    the same way, t = 1 and nu = mu, and never step them.)"""
    return np.max(list(component_differences(a, ref).values()), axis=0)


def component_differences(a, ref):
    """{component: (B,)}: the scaled difference of each component of the iterate on its own (which one a mismatch sits in)."""
    B = ref["X"].shape[0]
    out = {}
    for key in COMPONENTS:
        r, v = np.asarray(ref[key]), np.asarray(a[key])
        assert r.shape == v.shape, (key, r.shape, v.shape)
        e = np.abs(v - r) / (1.0 + np.abs(r))
        e = np.where(np.isnan(e), np.inf, e)
        out[key] = e.reshape(B, -1).max(axis=1)
    return out


def envelope(oracle_factory, x0, N, budgets, **solve_kw):
    """(traj, env, unstable) over k in budgets: traj as `trajectory` from the unperturbed x0; env {k: (B,)} the largest scaled
    difference between a perturbed and the unperturbed run; unstable {k: (B,) bool} whether a perturbation changed status, iters,
    n_reg, n_lsfail or mu (mu beyond MU_RTOL).  One oracle batch per budget holds the unperturbed batch and its P copies.
    traj[k]["env_kkt"] (B,): the same envelope of the KKT error alone, |kkt' - kkt| / (1 + |kkt|) (test_host_lockstep.py)."""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    B = x0.shape[0]
    allx = np.concatenate([x0] + perturbed(x0), axis=0)
    kw = {k: _tile(v, P_COPIES + 1) for k, v in solve_kw.items()}
    both = trajectory(oracle_factory, allx, N, budgets, **kw)
    traj, env, unstable = {}, {}, {}
    for k, r in both.items():
        part = lambda p: {key: v[p * B:(p + 1) * B] for key, v in r.items()}
        base = part(0)
        e, u = np.zeros(B), np.zeros(B, dtype=bool)
        base["env_kkt"] = np.zeros(B)
        for p in range(1, P_COPIES + 1):
            q = part(p)
            e = np.maximum(e, scaled_difference(q, base))
            base["env_kkt"] = np.maximum(base["env_kkt"], np.abs(q["kkt"] - base["kkt"]) / (1.0 + np.abs(base["kkt"])))
            for key in DISCRETE:
                u |= q[key] != base[key]
            u |= np.abs(q["mu"] - base["mu"]) > MU_RTOL * np.abs(base["mu"])
        traj[k], env[k], unstable[k] = base, e, u
    return traj, env, unstable


def excluded(env, unstable):
    """{k: (B,) bool}: pair (b, k) is left out - env[b, k] > ENV_MAX or a discrete output changed under perturbation, at k or at
    any smaller budget of the same instance."""
    out, acc = {}, None
    for k in sorted(env):
        now = (env[k] > ENV_MAX) | unstable[k]
        acc = now if acc is None else (acc | now)
        out[k] = acc.copy()
    return out


def caps_hold(excl, ks=None):
    """The caps the reference alone must meet over the budgets ks (default: all): (no pair excluded for k <= 10, excluded
    fraction <= 10 %), and the counts (excluded, pairs)."""
    ks = sorted(excl) if ks is None else [k for k in ks]
    n_ex = sum(int(excl[k].sum()) for k in ks)
    n = sum(excl[k].size for k in ks)
    early = sum(int(excl[k].sum()) for k in ks if k <= CAP_FIRST_K)
    return early == 0 and n_ex <= CAP_FRACTION * n, n_ex, n


def aligned(traj, by_k, iters):
    """Per-instance rows of the oracle runs whose max_iter equals iters[b]: (ref dict, by_k values (B,)).  by_k: {k: (B,)}."""
    iters = np.asarray(iters).astype(int)
    B = iters.shape[0]
    first = traj[min(traj)]
    ref = {key: np.empty_like(v) for key, v in first.items()}
    vals = np.empty(B, dtype=by_k[min(by_k)].dtype)
    for b in range(B):
        k = int(iters[b])
        if k not in traj:
            raise KeyError(f"instance {b}: the device reports iters = {k}, no oracle run at that budget (have {min(traj)}..{max(traj)})")
        for key in ref:
            ref[key][b] = traj[k][key][b]
        vals[b] = by_k[k][b]
    return ref, vals


def compare(gpu_iterate, gpu_stats, ref_k, env_k):
    """The device result against the reference rows ref_k (a result dict of Oracle.solve, row b the run instance b is compared
    with) and their envelope env_k (B,).  Returns dict(diff, ratio = diff / max(env, ENV_FLOOR), discrete (B,) bool: status,
    iters, n_reg, n_lsfail all equal, mu (B,) bool: equal to MU_RTOL relative, ok = ratio <= FACTOR & discrete & mu)."""
    diff = scaled_difference(gpu_iterate, ref_k)
    ratio = diff / np.maximum(env_k, ENV_FLOOR)
    disc = np.ones(diff.shape[0], dtype=bool)
    for key in DISCRETE:
        disc &= np.asarray(gpu_stats[key]).astype(int) == np.asarray(ref_k[key]).astype(int)
    mu = np.abs(np.asarray(gpu_stats["mu"]) - ref_k["mu"]) <= MU_RTOL * np.abs(ref_k["mu"])
    return dict(diff=diff, ratio=ratio, discrete=disc, mu=mu, ok=(ratio <= FACTOR) & disc & mu)


def check_runs(ref, runs, label=""):
    """Device runs {budget m: (iterate, stats)} of one case against its reference (Case.reference): the rule of DESIGN.md §6.
    Instance b of the run with budget m is compared with the oracle run at max_iter = iters[b] (`aligned`) unless that pair is
    excluded.  Asserted for every pair that is not excluded:
      - iters[b] <= m, and iters[b] == m where both sides report n_reg == 0 and status MAX_ITER (no repeated sweep: one pass per
        iteration);
      - scaled difference of the iterate <= FACTOR * max(env, ENV_FLOOR);
      - status, iters, n_lsfail and n_resto equal; n_reg equal and mu equal to MU_RTOL relative - except for an instance that ran
        out of passes WHILE REPEATING A SWEEP (status MAX_ITER on both sides, n_reg larger than the oracle's): it keeps the iterate
        of its last completed iteration j (asserted as above), but the head of iteration j has run, so its mu must be that of the
        oracle's run at max_iter = j + 1, and its n_reg at most that run's.
    Returns dict(worst ratio, excluded, pairs, failures: list of strings); prints one line."""
    traj, env, excl = ref["traj"], ref["env"], ref["excluded"]
    K = max(traj)
    worst, n_ex, n_pairs, failures, n_cut = 0.0, 0, 0, [], 0
    for m in sorted(runs):
        it, st = runs[m]
        iters = np.asarray(st["iters"]).astype(int)
        B = iters.shape[0]
        n_pairs += B
        if (iters > m).any() or (iters < 0).any():
            failures.append(f"m={m}: iters {iters.tolist()} outside 0..m")
            continue
        r, e = aligned(traj, env, iters)
        _, ex = aligned(traj, excl, iters)
        nxt, _ = aligned(traj, env, np.minimum(iters + 1, K))
        c = compare(it, st, r, e)
        comp = component_differences(it, r)
        both_cut = (np.asarray(st["status"]) == STATUS_MAX_ITER) & (r["status"] == STATUS_MAX_ITER)
        in_retry = both_cut & (iters < m) & (np.asarray(st["n_reg"]) > r["n_reg"])
        n_ex += int(ex.sum())
        n_cut += int((in_retry & ~ex).sum())
        for b in np.flatnonzero(~ex):
            why = []
            if both_cut[b] and st["n_reg"][b] == 0 and r["n_reg"][b] == 0 and iters[b] != m:
                why.append(f"iters {iters[b]} != budget")
            if not c["ratio"][b] <= FACTOR:
                k = max(comp, key=lambda n: comp[n][b])
                why.append(f"ratio {c['ratio'][b]:.3g} (diff {c['diff'][b]:.3e}, env {e[b]:.3e}, largest in {k})")
            for key in ("status", "iters", "n_lsfail", "n_resto"):
                if int(st[key][b]) != int(r[key][b]):
                    why.append(f"{key} {int(st[key][b])} != {int(r[key][b])}")
            if in_retry[b]:
                if not int(st["n_reg"][b]) <= int(nxt["n_reg"][b]):
                    why.append(f"n_reg {int(st['n_reg'][b])} > {int(nxt['n_reg'][b])} of the next iteration")
                if not abs(st["mu"][b] - nxt["mu"][b]) <= MU_RTOL * abs(nxt["mu"][b]):
                    why.append(f"mu {st['mu'][b]!r} != {nxt['mu'][b]!r} of the next iteration")
            else:
                if int(st["n_reg"][b]) != int(r["n_reg"][b]):
                    why.append(f"n_reg {int(st['n_reg'][b])} != {int(r['n_reg'][b])}")
                if not c["mu"][b]:
                    why.append(f"mu {st['mu'][b]!r} != {r['mu'][b]!r}")
            if why:
                failures.append(f"m={m} b={b} (k={iters[b]}): " + "; ".join(why))
            worst = max(worst, float(c["ratio"][b])) if np.isfinite(c["ratio"][b]) else np.inf
    print(f"lockstep {label}: worst ratio {worst:.3g} (limit {FACTOR:g}), excluded {n_ex} of {n_pairs} pairs, cut inside a repeated sweep {n_cut}, "
          f"failures {len(failures)}")
    return dict(worst=worst, excluded=n_ex, pairs=n_pairs, failures=failures, cut_in_retry=n_cut)


# ---------------------------------------------------------------------------------------------------- the cases
RESTORATION_STATE = [226.623754, -0.545036120, -0.0112268024, 8.52329373, 0.122918012, 0.161888169, 0.0837443810, 0.371730909]
OFF_TRACK_STATE = [100.0, 4.0, 0.0, 10.0, 0, 0, 0, 0]
THETA_GROUPS = ({"mass": 1050.0, "D_f": 0.9}, {"mass": 950.0, "D_f": 1.1})  # case e: instance b has group b % 2


class Case:
    """One case: the batch, the horizon, the largest budget K, how both sides start, and - made once, by the oracle alone - the
    reference trajectory at every k = 0 .. K with its envelope and exclusions.  groups: per-instance parameter sets (case e; one
    oracle per group); guess: dict(X, C, U, u_prev) both sides start from instead of a cold start (case f)."""

    def __init__(self, name, x0, N, K, groups=None, guess=None):
        self.name, self.x0, self.N, self.K, self.groups, self.guess = name, np.ascontiguousarray(x0, dtype=np.float64), N, K, groups, guess
        self.B = self.x0.shape[0]
        self.budgets = budgets(K)
        self._ref = None

    def group_rows(self, g):
        return np.arange(g, self.B, len(self.groups))

    def theta(self):
        """The argument of BatchedMPC.set_theta (None: a uniform handle)."""
        if self.groups is None:
            return None
        return {n: np.array([self.groups[b % len(self.groups)][n] for b in range(self.B)]) for n in self.groups[0]}

    def reference(self, orc, tables):
        if self._ref is None:
            ks = range(0, self.K + 1)
            parts = []
            for g, theta in enumerate(self.groups or (None,)):
                rows = np.arange(self.B) if theta is None else self.group_rows(g)
                p = None
                if theta is not None:
                    p = orc.default_params()
                    for n, v in theta.items():
                        setattr(p, n, v)
                kw = {}
                if self.guess is not None:
                    G = self.guess
                    kw = dict(uprev=G["u_prev"][rows], prev_status=np.full(len(rows), STATUS_MAX_ITER),
                              warm=dict(X=G["X"][rows], C=G["C"][rows], U=G["U"][rows], L1=np.zeros_like(G["C"][rows]), L2=np.zeros_like(G["C"][rows])))
                parts.append((rows, envelope(factory(orc, tables, params=p), self.x0[rows], self.N, ks, **kw)))
            traj, env, uns = {}, {}, {}
            for k in ks:
                traj[k] = {}
                for key, v in parts[0][1][0][k].items():
                    full = np.empty((self.B,) + v.shape[1:], dtype=v.dtype)
                    for rows, (t, _, _) in parts:
                        full[rows] = t[k][key]
                    traj[k][key] = full
                env[k], uns[k] = np.empty(self.B), np.empty(self.B, dtype=bool)
                for rows, (_, e, u) in parts:
                    env[k][rows], uns[k][rows] = e[k], u[k]
            self._ref = dict(traj=traj, env=env, unstable=uns, excluded=excluded(env, uns))
        return self._ref


_CASES = {}


def cases(pkg, tables, orc):
    """The cases of tests/test_gpu_lockstep.py by name, made once per process."""
    if _CASES:
        return _CASES
    x_ref = pkg.X0_REFERENCE[None]
    add = lambda c: _CASES.__setitem__(c.name, c)
    add(Case("a", np.vstack([x_ref, pkg.sample_x0(tables, 14, seed=61), [RESTORATION_STATE]]), 10, 30))
    add(Case("b", np.vstack([x_ref, pkg.sample_x0(tables, 15, seed=61)]), 40, 10))
    add(Case("c", pkg.sample_x0(tables, 12, seed=83), 3, 18))   # (every instance has converged by k = 16)
    add(Case("d", pkg.sample_x0(tables, 70, seed=61), 10, 10))
    add(Case("e", _CASES["a"].x0, 10, 12, groups=THETA_GROUPS))
    # f: as test_guess_matches_oracle - the guess is the oracle's cold solution at x0, the solve is at x1 = plant(x0, u0)
    N, x0 = 10, pkg.sample_x0(tables, 16, seed=21)
    o = orc.Oracle(tables.packed())
    cold = o.solve(x0, N, nthreads=8)
    add(Case("f", o.plant_step(x0, cold["u0"]), N, 12, guess=dict(X=cold["X"], C=cold["C"], U=cold["U"], u_prev=cold["u0"])))
    # g: the elastic phase - the state that needs the restoration phase, and one off the track, at N = 8 and 10
    add(Case("g8", np.array([RESTORATION_STATE, OFF_TRACK_STATE]), 8, 30))
    add(Case("g10", np.array([RESTORATION_STATE, OFF_TRACK_STATE]), 10, 30))
    return _CASES
