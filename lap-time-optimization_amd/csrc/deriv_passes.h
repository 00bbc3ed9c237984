// deriv_passes.h — host drivers and C entry points of the derivative passes on the final iterate of a solve:
// sensitivities w.r.t. (x0, u_prev) and theta, the adjoint of a trajectory loss (w.r.t. those and w.r.t. the track tables), their
// product with one direction, the plant-step sensitivities and the closed loop.
// Part of ltompc.hip's translation unit, after ltompc_solver and its helpers; the passes' state is ltompc_solver::dv (DerivState).
#pragma once

// Solve records.  SolveView: the fields of the handle through which the passes below address "the solve".  A record
// holds one that points into its own buffers; while an entry point runs on a selected record the two are exchanged (RecScope), so
// the drivers below are the same code on the same kernels either way.  The passes' buffers (QP, RC, RS, LS, the PV / AJ / JV / TJ
// planes, the results) stay the handle's.
struct SolveView {
  Consts K;
  Consts* d_K = nullptr;
  Work W{}, *d_W = nullptr, Ws{}, *d_Ws = nullptr;
  WorkPI Wpi{}, *d_Wpi = nullptr, Wspi{}, *d_Wspi = nullptr;
  double* d_psens_uprev = nullptr;
  bool pi_solve = false, ts_solve = false, ref_eval = false, eval8 = true;
  int n_sets = 0;
  Sens sens = Sens::no_solve;  // ... and how far the passes have got on it (DerivState)
  Psens psens = Psens::none;
  bool fact = false, pv_valid = false, kept_uprev = false;
};
struct ltompc_record_s {
  bool in_use = false;  // else on the handle's free list
  char* base = nullptr;  // the one device buffer, and the arrays in it
  double *X = nullptr, *C = nullptr, *U = nullptr, *L1 = nullptr, *L2 = nullptr, *T = nullptr, *NU = nullptr, *st = nullptr, *x0 = nullptr,
         *uprev = nullptr, *TH = nullptr, *tab = nullptr;
  int* si = nullptr;
  SolveView v;
};

namespace {

int ws_alloc(ltompc_solver* h);  // (warm_state_host.h)
const int* ws_inverse(ltompc_solver* h);

void view_exchange(ltompc_solver* h, SolveView& v) {
  DerivState& D = h->dv;
  std::swap(h->K, v.K), std::swap(h->d_K, v.d_K), std::swap(h->W, v.W), std::swap(h->d_W, v.d_W), std::swap(D.Ws, v.Ws), std::swap(D.d_Ws, v.d_Ws);
  std::swap(h->Wpi, v.Wpi), std::swap(h->d_Wpi, v.d_Wpi), std::swap(D.Wspi, v.Wspi), std::swap(D.d_Wspi, v.d_Wspi);
  std::swap(D.d_psens_uprev, v.d_psens_uprev), std::swap(h->pi_solve, v.pi_solve), std::swap(h->ts_solve, v.ts_solve);
  std::swap(h->ref_eval, v.ref_eval), std::swap(h->eval8, v.eval8), std::swap(h->n_sets, v.n_sets);
  std::swap(D.sens, v.sens), std::swap(D.psens, v.psens), std::swap(D.fact, v.fact), std::swap(D.pv_valid, v.pv_valid);
  std::swap(D.kept_uprev, v.kept_uprev);
}
// For the duration of a derivative entry point: the selected record in the handle's place (nothing when none is selected).
struct RecScope {
  ltompc_solver* h;
  explicit RecScope(ltompc_solver* h_) : h(h_) {
    if (h->rec_sel) view_exchange(h, h->rec_sel->v);
  }
  ~RecScope() {
    if (h->rec_sel) view_exchange(h, h->rec_sel->v);
  }
  RecScope(const RecScope&) = delete;
  RecScope& operator=(const RecScope&) = delete;
};
int no_record(ltompc_solver* h, const char* who) {
  if (h->rec_sel) return fail(std::string(who) + ": not available while a solve record is selected (ltompc_record_select(h, NULL) first)");
  return 0;
}

constexpr hipMemcpyKind D2H = hipMemcpyDeviceToHost, D2D = hipMemcpyDeviceToDevice;

// n elements to an output of a C entry point, host or device by `kind`; dst may be null (an output the caller does not ask for)
template <typename T>
int copy_out(ltompc_solver* h, const hipMemcpyKind kind, T* dst, const T* src, const size_t n) {
  if (dst) HIPCHECK(hipMemcpyAsync(dst, src, n * sizeof(T), kind, h->stream));
  return 0;
}

// The re-linearisation and head-less sweep of the sensitivity passes (sensitivity.h), shared by all of them: run once per solve,
// and again only when the instances have moved since (same blocks, same bits, at their new slots).  The uniform kernels on Ws or
// the _pi ones on its WorkPI form (at each instance's rows of that solve, TH); the evaluation kernels the solve used.
void sens_factorise(ltompc_solver* h) {
  DerivState& D = h->dv;
  if (D.fact) return;
  const int N = h->N, Bp = h->Bp;
  const bool ref = h->ref_eval, ell = h->K.bd.nel > 0;
  const auto run = [&](auto eval8, auto eval, auto riccati8, auto* d_W, const auto& W) {
    if (h->eval8 && !h->ts_solve) hipLaunchKernelGGL(eval8, dim3(N * (Bp / 8)), dim3(64), 0, h->stream, (const Consts*)h->d_K, d_W);
    else hipLaunchKernelGGL(eval, dim3((N * Bp + 63) / 64), dim3(64), 0, h->stream, (const Consts*)h->d_K, d_W);
    hipLaunchKernelGGL(riccati8, dim3(Bp / 8), dim3(64), 0, h->stream, h->K, W, (const int*)h->W.si, D.d_sens_inertia);
  };
  if (h->ts_solve)  // (with table sets: thread-per-slot as the solve; the head-less sweep reads no table, the _pi one on the WorkPI part)
    run(k_sens_eval8_pi, ref ? k_sens_eval_ts<BoundsRef> : k_sens_eval_ts<BoundsAny>, k_sens_riccati8_pi, (const WorkTS*)D.d_Wsts, D.Wspi);
  else if (h->pi_solve)
    run(k_sens_eval8_pi, ref ? k_sens_eval_pi<BoundsRef> : k_sens_eval_pi<BoundsAny>, k_sens_riccati8_pi, (const WorkPI*)D.d_Wspi, D.Wspi);
  else
    run(k_sens_eval8, ell ? (ref ? k_sens_eval<BoundsRef, true> : k_sens_eval<BoundsAny, true>)
                          : (ref ? k_sens_eval<BoundsRef, false> : k_sens_eval<BoundsAny, false>),
        k_sens_riccati8, (const Work*)D.d_Ws, D.Ws);
  D.fact = true;
}

// The buffers of the (x0, u_prev) pass, which every pass shares, on the first request (one synchronisation).  On the live handle
// only: a record brings a Ws of its own that points at them.
int sens_buffers(ltompc_solver* h) {
  DerivState& D = h->dv;
  const int B = h->B, N = h->N, Bp = h->Bp;
  if (!D.d_Ws) {
    Work& Ws = D.Ws = h->W;
    int rc = 0;
    rc |= h->dalloc(&Ws.QP, (size_t)QP_NF * (N + 1) * Bp, true), rc |= h->dalloc(&Ws.RC, (size_t)RC_NF * (N + 1) * Bp, true);
    rc |= h->dalloc(&Ws.RS, (size_t)RS_NF * N * Bp, true), rc |= h->dalloc(&Ws.LS, (size_t)3 * N * Bp, true);
    rc |= h->dalloc(&Ws.si, (size_t)SI_NF * Bp);  // zeros, never written
    rc |= h->dalloc(&D.d_sens_inertia, Bp), rc |= h->dalloc(&D.d_sens_ok, Bp);
    rc |= h->dalloc(&D.d_sens_du0, (size_t)2 * SENS_NP * B), rc |= h->dalloc(&D.d_sens_margin, B);
    rc |= h->dalloc(&D.d_Ws, 1);
    if (rc) return -1;
    HIPCHECK(hipMemcpyAsync(D.d_Ws, &D.Ws, sizeof(Work), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (h->d_th_solve && sync_pi_work(h)) return -1;
  }
  return 0;
}

// The sensitivity pass of the last solve (sensitivity.h), enqueued on the handle's stream: linearisation and head-less sweep
// when not done since that solve (or when the instances have moved since), the forward pass for du0 / ok / margin, and the
// trajectories when asked for.  Results in the caller's order, cached until the next solve or initial guess.
int sens_compute(ltompc_solver* h, const bool traj, const char* who) {
  DerivState& D = h->dv;
  if (D.sens == Sens::no_solve) return fail(std::string(who) + ": no solve to differentiate (make_step, make_step_dev or rollout_dev first; set_initial_guess, set_table_values and set_table_sets discard the last solve)");
  const int B = h->B, N = h->N, Bp = h->Bp;
  if (sens_buffers(h)) return -1;
  if (D.sens == Sens::solved) {
    sens_factorise(h);
    hipLaunchKernelGGL(k_sens_forward, dim3(Bp / 8), dim3(64), 0, h->stream, D.Ws, (const int*)D.d_sens_inertia, h->K.bd.ni, D.d_sens_du0,
                       D.d_sens_ok, D.d_sens_margin, (double*)nullptr, (double*)nullptr, (const int*)nullptr);
    D.sens = Sens::du0;
  }
  if (traj && D.sens == Sens::du0) {
    if (!D.d_sens_dX && (h->dalloc(&D.d_sens_dX, (size_t)(N + 1) * 8 * SENS_NP * B) || h->dalloc(&D.d_sens_dU, (size_t)N * 2 * SENS_NP * B)))
      return -1;
    sens_factorise(h);
    hipLaunchKernelGGL(k_sens_forward, dim3(Bp / 8), dim3(64), 0, h->stream, D.Ws, (const int*)D.d_sens_inertia, h->K.bd.ni, (double*)nullptr,
                       (int*)nullptr, (double*)nullptr, D.d_sens_dX, D.d_sens_dU, (const int*)D.d_sens_ok);
    D.sens = Sens::traj;
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

// The passes that per-instance table sets do not cover: a worded usage error.
int no_table_sets(ltompc_solver* h, const char* who, const char* what) {
  if (h->n_sets)
    return fail(std::string(who) + ": " + what + " not available on a handle with per-instance table sets (ltompc_set_table_sets; n_sets = 0 and a new solve bring it back)");
  return 0;
}

// What both passes over theta need: a problem that theta covers, a solve to differentiate whose u_prev was kept, the PV buffers.
int psens_prepare(ltompc_solver* h, const char* who) {
  DerivState& D = h->dv;
  if (no_table_sets(h, who, "the derivatives w.r.t. the vehicle and cost parameters are")) return -1;
  if (h->K.p.ell_penalty > 0.0) return fail(std::string(who) + ": not available with the friction-ellipse constraints (ell_penalty > 0)");
  if (h->K.p.ptv != 0.0) return fail(std::string(who) + ": not available with torque vectoring (ptv != 0)");
  if (sens_compute(h, false, who)) return -1;  // (the usage error before a solve comes from here)
  if (!D.kept_uprev) return fail(std::string(who) + ": not available after a rollout (it does not keep the u_prev of each instance's last solve, which the r_du columns need)");
  const int B = h->B, N = h->N, Bp = h->Bp;
  if (!D.d_psens_pv && (h->dalloc(&D.d_psens_pv, (size_t)PV_NF * N * Bp, true) || h->dalloc(&D.d_psens_kf, (size_t)N * 2 * PS_NT * Bp, true) ||
                        h->dalloc(&D.d_psens_du0, (size_t)2 * PS_NT * B)))
    return -1;
  return 0;
}

// The factorisation and k_psens_cond's PV planes at the instances' current slots, each only when not there already (both passes
// that read the planes come through here).
void psens_condense(ltompc_solver* h) {
  DerivState& D = h->dv;
  sens_factorise(h);
  if (D.pv_valid) return;
  const int N = h->N, Bp = h->Bp;
  if (h->pi_solve)
    hipLaunchKernelGGL(h->ref_eval ? k_psens_cond_pi<BoundsRef> : k_psens_cond_pi<BoundsAny>, dim3((N * Bp + 63) / 64), dim3(64), 0, h->stream,
                       (const Consts*)h->d_K, (const WorkPI*)h->d_Wpi, D.d_psens_pv);
  else
    hipLaunchKernelGGL(h->ref_eval ? k_psens_cond<BoundsRef> : k_psens_cond<BoundsAny>, dim3((N * Bp + 63) / 64), dim3(64), 0, h->stream,
                       (const Consts*)h->d_K, (const Work*)h->d_W, D.d_psens_pv);
  D.pv_valid = true;
}

// The parameter-sensitivity pass of the last solve (param_sensitivity.h): ok (and du0 / margin) of the pass above, whose
// factorisation it shares, then the condensed right-hand sides of the 16 columns and their recursion.  Cached like the above.
int psens_compute(ltompc_solver* h, const bool traj, const char* who) {
  DerivState& D = h->dv;
  if (psens_prepare(h, who)) return -1;
  const int B = h->B, N = h->N, Bp = h->Bp;
  if (traj && !D.d_psens_dX && (h->dalloc(&D.d_psens_dX, (size_t)(N + 1) * 8 * PS_NT * B) || h->dalloc(&D.d_psens_dU, (size_t)N * 2 * PS_NT * B)))
    return -1;
  if (D.psens == Psens::none || (traj && D.psens == Psens::du0)) {
    psens_condense(h);
    double *const dX = traj ? D.d_psens_dX : nullptr, *const dU = traj ? D.d_psens_dU : nullptr;
    if (h->pi_solve)
      hipLaunchKernelGGL(k_psens_sweep_pi, dim3(Bp / 8, 2), dim3(64), 0, h->stream, D.Wspi, (const double*)D.d_psens_uprev,
                         (const double*)D.d_psens_pv, (const int*)D.d_sens_ok, D.d_psens_kf, D.d_psens_du0, dX, dU);
    else
      hipLaunchKernelGGL(k_psens_sweep, dim3(Bp / 8, 2), dim3(64), 0, h->stream, D.Ws, h->K.p.r_du[0], h->K.p.r_du[1],
                         (const double*)D.d_psens_uprev, (const double*)D.d_psens_pv, (const int*)D.d_sens_ok, D.d_psens_kf, D.d_psens_du0, dX, dU);
    D.psens = traj ? Psens::traj : Psens::du0;
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

// The adjoint pass of the last solve (adjoint.h) for one cotangent (device pointers, caller's order; either may be null), into
// d_adj_gp and, with theta, d_adj_gth: the factorisation and the PV planes when not there, then one sweep.  Once its buffers
// exist it only enqueues.
int adj_compute(ltompc_solver* h, const double* gX_dev, const double* gU_dev, const bool theta, const char* who) {
  DerivState& D = h->dv;
  if (!gX_dev && !gU_dev) return fail(std::string(who) + ": gX and gU are both NULL (no cotangent)");
  if (theta ? psens_prepare(h, who) : sens_compute(h, false, who)) return -1;
  const int B = h->B, N = h->N, Bp = h->Bp;
  if (!D.d_adj_gp && (h->dalloc(&D.d_adj_gp, (size_t)ADJ_NP * B) || h->dalloc(&D.d_adj_gth, (size_t)PS_NT * B))) return -1;
  if (theta && !D.d_adj_aj && h->dalloc(&D.d_adj_aj, (size_t)AJ_NF * N * Bp, true)) return -1;
  theta ? psens_condense(h) : sens_factorise(h);
  double* const gth = theta ? D.d_adj_gth : nullptr;
  if (h->pi_solve)
    hipLaunchKernelGGL(k_adj_sweep_pi, dim3(Bp / 8), dim3(64), 0, h->stream, D.Wspi, (const double*)D.d_psens_uprev, (const double*)D.d_psens_pv,
                       (const int*)D.d_sens_ok, gX_dev, gU_dev, D.d_adj_aj, D.d_adj_gp, gth);
  else
    hipLaunchKernelGGL(k_adj_sweep, dim3(Bp / 8), dim3(64), 0, h->stream, D.Ws, h->K.p.r_du[0], h->K.p.r_du[1], (const double*)D.d_psens_uprev,
                       (const double*)D.d_psens_pv, (const int*)D.d_sens_ok, gX_dev, gU_dev, D.d_adj_aj, D.d_adj_gp, gth);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The table-gradient pass of the last solve (table_sensitivity.h) for one cotangent (device pointers, caller's order; either may
// be null), into d_tab_sg and d_tab_gt: the factorisation when not there, the sweep that keeps the adjoint trajectory, the
// per-slot contraction, then the scatter to the knots into the zeroed d_tab_gt.  It needs no u_prev, so it also runs after a
// rollout.  Once its buffers exist it only enqueues.
// `sets`: the caller is one of the per-set entry points (grad_sets in d_tab_gs, [n_sets][4][n_table]); each kind of handle has its own.
int tab_compute(ltompc_solver* h, const double* gX_dev, const double* gU_dev, const char* who, const bool sets = false) {
  DerivState& D = h->dv;
  if (!sets && h->n_sets)
    return fail(std::string(who) + ": this handle has per-instance table sets, its table gradient is one per set: ltompc_get_adjoint_table_sets / ltompc_adjoint_table_sets_dev");
  if (sets && !h->n_sets)
    return fail(std::string(who) + ": this handle has no table sets (ltompc_set_table_sets), its table gradient is ltompc_get_adjoint_tables / ltompc_adjoint_tables_dev");
  if (!gX_dev && !gU_dev) return fail(std::string(who) + ": gX and gU are both NULL (no cotangent)");
  if (h->K.p.ell_penalty > 0.0) return fail(std::string(who) + ": not available with the friction-ellipse constraints (ell_penalty > 0)");
  if (h->K.p.ptv != 0.0) return fail(std::string(who) + ": not available with torque vectoring (ptv != 0)");
  if (sens_compute(h, false, who)) return -1;  // (ok; the usage error before a solve comes from here)
  const int B = h->B, N = h->N, Bp = h->Bp;
  if (!D.d_tab_tj) {
    if (h->dalloc(&D.d_tab_tj, (size_t)TJ_NF * N * Bp, true) || h->dalloc(&D.d_tab_sg, (size_t)TS_NS * N * B) ||
        h->dalloc(&D.d_tab_gt, (size_t)TAB_ROWS * h->n_table))
      return -1;
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  if (sets && h->n_sets > D.tab_gs_cap) {  // (grows with the number of sets, as the value buffer)
    double* fresh = nullptr;
    if (h->dalloc(&fresh, (size_t)TAB_ROWS * h->n_table * h->n_sets)) return -1;
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->dfree(D.d_tab_gs);
    D.d_tab_gs = fresh, D.tab_gs_cap = h->n_sets;
  }
  sens_factorise(h);
  const dim3 slots((N * Bp + 63) / 64), block(64);
  const size_t nthreads = (size_t)3 * N * Bp;
  if (sets) {  // (the sweep reads no table: the _pi one; the contraction on each instance's rows; the scatter into the block of its set)
    hipLaunchKernelGGL(k_adj_sweep_tab_pi, dim3(Bp / 8), block, 0, h->stream, D.Wspi, gX_dev, gU_dev, D.d_tab_tj);
    hipLaunchKernelGGL(h->ref_eval ? k_tab_cond_ts<BoundsRef> : k_tab_cond_ts<BoundsAny>, slots, block, 0, h->stream, (const Consts*)h->d_K,
                       (const WorkTS*)h->d_Wts, (const double*)D.d_tab_tj, (const int*)D.d_sens_ok, D.d_tab_sg);
    HIPCHECK(hipMemsetAsync(D.d_tab_gs, 0, sizeof(double) * TAB_ROWS * h->n_table * h->n_sets, h->stream));
    hipLaunchKernelGGL(k_tab_scatter_ts, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, h->stream, (const Consts*)h->d_K, h->W,
                       (const int*)D.d_sens_ok, (const double*)D.d_tab_sg, D.d_tab_gs, (const int*)h->d_ts_idx);
    HIPCHECK(hipGetLastError());
    return 0;
  }
  if (h->pi_solve) {
    hipLaunchKernelGGL(k_adj_sweep_tab_pi, dim3(Bp / 8), block, 0, h->stream, D.Wspi, gX_dev, gU_dev, D.d_tab_tj);
    hipLaunchKernelGGL(h->ref_eval ? k_tab_cond_pi<BoundsRef> : k_tab_cond_pi<BoundsAny>, slots, block, 0, h->stream, (const Consts*)h->d_K,
                       (const WorkPI*)h->d_Wpi, (const double*)D.d_tab_tj, (const int*)D.d_sens_ok, D.d_tab_sg);
  } else {
    hipLaunchKernelGGL(k_adj_sweep_tab, dim3(Bp / 8), block, 0, h->stream, D.Ws, h->K.p.r_du[0], h->K.p.r_du[1], gX_dev, gU_dev, D.d_tab_tj);
    hipLaunchKernelGGL(h->ref_eval ? k_tab_cond<BoundsRef> : k_tab_cond<BoundsAny>, slots, block, 0, h->stream, (const Consts*)h->d_K,
                       (const Work*)h->d_W, (const double*)D.d_tab_tj, (const int*)D.d_sens_ok, D.d_tab_sg);
  }
  HIPCHECK(hipMemsetAsync(D.d_tab_gt, 0, sizeof(double) * TAB_ROWS * h->n_table, h->stream));
  hipLaunchKernelGGL(k_tab_scatter, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, h->stream, (const Consts*)h->d_K, h->W,
                     (const int*)D.d_sens_ok, (const double*)D.d_tab_sg, D.d_tab_gt);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The directional pass of the last solve (jvp.h) for one direction (device pointers, caller's order; either may be null), into
// tX_dev / tU_dev (either may be null): the factorisation and, with dtheta, the PV planes when not there, then one sweep.  Once
// its kff planes exist it only enqueues.
int jvp_compute(ltompc_solver* h, const double* dp_dev, const double* dth_dev, double* tX_dev, double* tU_dev, const char* who) {
  DerivState& D = h->dv;
  if (!dp_dev && !dth_dev) return fail(std::string(who) + ": dp and dtheta are both NULL (no direction)");
  if (dth_dev ? psens_prepare(h, who) : sens_compute(h, false, who)) return -1;
  const int N = h->N, Bp = h->Bp;
  if (dth_dev && !D.d_jvp_jv) {
    if (h->dalloc(&D.d_jvp_jv, (size_t)JV_NF * N * Bp, true)) return -1;
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  dth_dev ? psens_condense(h) : sens_factorise(h);
  if (h->pi_solve)
    hipLaunchKernelGGL(k_jvp_sweep_pi, dim3(Bp / 8), dim3(64), 0, h->stream, D.Wspi, (const double*)D.d_psens_uprev, (const double*)D.d_psens_pv,
                       (const int*)D.d_sens_ok, dp_dev, dth_dev, D.d_jvp_jv, tX_dev, tU_dev);
  else
    hipLaunchKernelGGL(k_jvp_sweep, dim3(Bp / 8), dim3(64), 0, h->stream, D.Ws, h->K.p.r_du[0], h->K.p.r_du[1], (const double*)D.d_psens_uprev,
                       (const double*)D.d_psens_pv, (const int*)D.d_sens_ok, dp_dev, dth_dev, D.d_jvp_jv, tX_dev, tU_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The directional pass in the track tables of the last solve (table_jvp.h) for one direction (device pointers, caller's order):
// dp (B x 10), dtables (4 x n_table; `sets`: n_sets x 4 x n_table) and dslot (B x N x 10), any of them null but not all, into
// tX_dev / tU_dev (either may be null): the factorisation when not there, the slots' stage vectors, then one sweep.  With dp alone
// it is jvp.h's dp-only sweep.  It needs no u_prev, so it also runs after a rollout.  Once its planes exist it only enqueues.
// `sets`: the caller is one of the per-set entry points; each kind of handle has its own.
int tjv_compute(ltompc_solver* h, const double* dp_dev, const double* dt_dev, const double* ds_dev, double* tX_dev, double* tU_dev,
                const char* who, const bool sets = false) {
  DerivState& D = h->dv;
  if (!sets && h->n_sets)
    return fail(std::string(who) + ": this handle has per-instance table sets, its table direction is one per set: ltompc_get_jvp_table_sets / ltompc_jvp_table_sets_dev");
  if (sets && !h->n_sets)
    return fail(std::string(who) + ": this handle has no table sets (ltompc_set_table_sets), its directional pass in the tables is ltompc_get_jvp_tables / ltompc_jvp_tables_dev");
  if (!dp_dev && !dt_dev && !ds_dev) return fail(std::string(who) + ": dp, dtables and dslot are all NULL (no direction)");
  if (h->K.p.ell_penalty > 0.0) return fail(std::string(who) + ": not available with the friction-ellipse constraints (ell_penalty > 0)");
  if (h->K.p.ptv != 0.0) return fail(std::string(who) + ": not available with torque vectoring (ptv != 0)");
  if (!dt_dev && !ds_dev) return jvp_compute(h, dp_dev, nullptr, tX_dev, tU_dev, who);  // (the existing dp-only instantiation)
  if (sens_compute(h, false, who)) return -1;  // (ok; the usage error before a solve comes from here)
  const int N = h->N, Bp = h->Bp;
  if (!D.d_tjv_tq) {
    if (h->dalloc(&D.d_tjv_tq, (size_t)TQ_NF * N * Bp, true) || h->dalloc(&D.d_tjv_jv, (size_t)JV_NF * N * Bp, true)) return -1;
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  sens_factorise(h);
  const dim3 slots((N * Bp + 63) / 64), block(64);
  const int* ok = D.d_sens_ok;
  if (sets) {  // (the stage vectors on each instance's rows and block of the direction; the sweep reads no table: the _pi one)
    hipLaunchKernelGGL(h->ref_eval ? k_tabjvp_cond_ts<BoundsRef> : k_tabjvp_cond_ts<BoundsAny>, slots, block, 0, h->stream, (const Consts*)h->d_K,
                       (const WorkTS*)h->d_Wts, ok, dt_dev, ds_dev, D.d_tjv_tq);
    hipLaunchKernelGGL(k_jvp_sweep_tab_pi, dim3(Bp / 8), block, 0, h->stream, D.Wspi, (const double*)D.d_tjv_tq, ok, dp_dev, D.d_tjv_jv, tX_dev,
                       tU_dev);
  } else if (h->pi_solve) {
    hipLaunchKernelGGL(h->ref_eval ? k_tabjvp_cond_pi<BoundsRef> : k_tabjvp_cond_pi<BoundsAny>, slots, block, 0, h->stream, (const Consts*)h->d_K,
                       (const WorkPI*)h->d_Wpi, ok, dt_dev, ds_dev, D.d_tjv_tq);
    hipLaunchKernelGGL(k_jvp_sweep_tab_pi, dim3(Bp / 8), block, 0, h->stream, D.Wspi, (const double*)D.d_tjv_tq, ok, dp_dev, D.d_tjv_jv, tX_dev,
                       tU_dev);
  } else {
    hipLaunchKernelGGL(h->ref_eval ? k_tabjvp_cond<BoundsRef> : k_tabjvp_cond<BoundsAny>, slots, block, 0, h->stream, (const Consts*)h->d_K,
                       (const Work*)h->d_W, ok, dt_dev, ds_dev, D.d_tjv_tq);
    hipLaunchKernelGGL(k_jvp_sweep_tab, dim3(Bp / 8), block, 0, h->stream, D.Ws, h->K.p.r_du[0], h->K.p.r_du[1], (const double*)D.d_tjv_tq, ok,
                       dp_dev, D.d_tjv_jv, tX_dev, tU_dev);
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

// The host form of the above: every direction checked finite, staged, the pass, the results copied back.
int tjv_host(ltompc_solver* h, const double* dp, const double* dtables, const double* dslot, double* tX, double* tU, int* ok, const char* who,
             const bool sets) {
  if (!dp && !dtables && !dslot) return fail(std::string(who) + ": dp, dtables and dslot are all NULL (no direction)");
  if (!sets && h->n_sets)
    return fail(std::string(who) + ": this handle has per-instance table sets, its table direction is one per set: ltompc_get_jvp_table_sets / ltompc_jvp_table_sets_dev");
  if (sets && !h->n_sets)
    return fail(std::string(who) + ": this handle has no table sets (ltompc_set_table_sets), its directional pass in the tables is ltompc_get_jvp_tables / ltompc_jvp_tables_dev");
  const size_t B = h->B, N = h->N, n = h->n_table, ns = sets ? h->n_sets : 1;
  static const char* const rows[TAB_ROWS] = {"kappa", "n_left", "n_right", "v_ref"};
  for (size_t e = 0; dtables && e < ns * TAB_ROWS * n; e++)
    if (!std::isfinite(dtables[e])) {
      const size_t r = e / n % TAB_ROWS;
      return fail(std::string(who) + ": non-finite dtables" + (sets ? " of set " + std::to_string(e / (TAB_ROWS * n)) + "," : "") + " row " +
                  std::to_string(r) + " (" + rows[r] + "), knot " + std::to_string(e % n));
    }
  for (size_t b = 0; b < B; b++) {
    bool fin = true;
    for (size_t e = 0; dp && e < JVP_NP; e++) fin = fin && std::isfinite(dp[b * JVP_NP + e]);
    for (size_t e = 0; dslot && e < N * TS_NS; e++) fin = fin && std::isfinite(dslot[b * N * TS_NS + e]);
    if (!fin) return fail(std::string(who) + ": non-finite direction of instance " + std::to_string(b));
  }
  HIPCHECK(hipSetDevice(h->device));
  DerivState& D = h->dv;
  if (!D.d_tjv_dp && (h->dalloc(&D.d_tjv_dp, JVP_NP * B) || h->dalloc(&D.d_tjv_ds, TS_NS * N * B) || h->dalloc(&D.d_tjv_tX, (N + 1) * 8 * B) ||
                      h->dalloc(&D.d_tjv_tU, N * 2 * B)))
    return -1;
  if (dtables && (int)ns > D.tjv_dt_cap) {  // (grows with the number of sets, as the value buffer)
    double* fresh = nullptr;
    if (h->dalloc(&fresh, TAB_ROWS * n * ns)) return -1;
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->dfree(D.d_tjv_dt);
    D.d_tjv_dt = fresh, D.tjv_dt_cap = (int)ns;
  }
  if (dp) HIPCHECK(hipMemcpyAsync(D.d_tjv_dp, dp, sizeof(double) * JVP_NP * B, hipMemcpyHostToDevice, h->stream));
  if (dtables) HIPCHECK(hipMemcpyAsync(D.d_tjv_dt, dtables, sizeof(double) * TAB_ROWS * n * ns, hipMemcpyHostToDevice, h->stream));
  if (dslot) HIPCHECK(hipMemcpyAsync(D.d_tjv_ds, dslot, sizeof(double) * TS_NS * N * B, hipMemcpyHostToDevice, h->stream));
  if (tjv_compute(h, dp ? D.d_tjv_dp : nullptr, dtables ? D.d_tjv_dt : nullptr, dslot ? D.d_tjv_ds : nullptr, tX ? D.d_tjv_tX : nullptr,
                  tU ? D.d_tjv_tU : nullptr, who, sets))
    return -1;
  if (copy_out(h, D2H, tX, D.d_tjv_tX, (N + 1) * 8 * B) || copy_out(h, D2H, tU, D.d_tjv_tU, N * 2 * B) || copy_out(h, D2H, ok, D.d_sens_ok, B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

// k_plant_sens' planes and the row-major staging of the host forms and, with `loop`, the closed loop's state: each on the first
// request, with one synchronisation.
int psn_prepare(ltompc_solver* h, const bool loop) {
  DerivState& D = h->dv;
  int rc = 0;
  bool fresh = false;
  if (!D.d_psn_planes) {
    rc |= h->dalloc(&D.d_psn_planes, (size_t)PSN_NF * h->Bp, true), rc |= h->dalloc(&D.d_psn_rm, (size_t)PSN_NF * h->B);
    fresh = true;
  }
  if (loop && !D.d_loop_Sx) {
    rc |= h->dalloc(&D.d_loop_Sx, (size_t)8 * LOOP_NQ * h->Bp), rc |= h->dalloc(&D.d_loop_Du, (size_t)2 * LOOP_NQ * h->Bp);
    rc |= h->dalloc(&D.d_loop_ok, h->Bp), rc |= h->dalloc(&D.d_loop_ticks, h->Bp);
    fresh = true;
  }
  if (rc) return -1;
  if (fresh) HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

// The plant-step sensitivities at (x_dev, u_dev) into the planes, with the rows in effect (those set last, as the plant step).
int psn_launch(ltompc_solver* h, const double* x_dev, const double* u_dev, const int n_sub, const bool theta) {
  const dim3 grid((h->B + 7) / 8), block(64);
  if (h->pi_pend)
    hipLaunchKernelGGL(k_plant_sens_pi, grid, block, 0, h->stream, h->K, (const double*)h->d_th_pend, h->B, h->Bp, x_dev, u_dev, h->K.o.t_step,
                       n_sub, theta ? 1 : 0, h->dv.d_psn_planes);
  else
    hipLaunchKernelGGL(k_plant_sens, grid, block, 0, h->stream, h->K, h->B, h->Bp, x_dev, u_dev, h->K.o.t_step, n_sub, theta ? 1 : 0,
                       h->dv.d_psn_planes);
  HIPCHECK(hipGetLastError());
  return 0;
}

// planes [f0 .. f0 + F)[Bp] -> row-major B x F at out_dev
int planes_to_rows(ltompc_solver* h, const double* planes, const int f0, const int F, double* out_dev) {
  const size_t n = (size_t)h->B * F;
  hipLaunchKernelGGL(k_planes_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, planes, f0, F, h->B, h->Bp, out_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The feedback policy of the last solve (policy.h): ok of the (x0, u_prev) pass and the factorisation, whose
// Riccati buffer holds the gains, at the instances' current slots (whichever pass runs first for a solve makes them).  `law`: the
// caller evaluates pi_k, which needs the u_prev that solve used (V_0).  Once the pass's buffers exist it only enqueues.
int pol_prepare(ltompc_solver* h, const bool law, const char* who) {
  DerivState& D = h->dv;
  if (law && D.sens != Sens::no_solve && !D.kept_uprev)
    return fail(std::string(who) + ": not available after a rollout (it does not keep the u_prev of each instance's last solve, V_0 of the policy; the gains are: ltompc_get_policy)");
  if (sens_compute(h, false, who)) return -1;  // (the usage error before a solve comes from here)
  sens_factorise(h);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The stage gains of all instances into K_dev (B x N x 2 x 8) / Kv_dev (B x N x 2 x 2), either may be null
int pol_gather(ltompc_solver* h, double* K_dev, double* Kv_dev) {
  if (!K_dev && !Kv_dev) return 0;
  hipLaunchKernelGGL(k_policy_gather, dim3(h->Bp / 8, (h->N + POL_KS - 1) / POL_KS), dim3(256), 0, h->stream, h->dv.Ws, (const int*)h->dv.d_sens_ok,
                     K_dev, Kv_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The staging of the policy's host forms, each on its first request with one synchronisation
int pol_staging(ltompc_solver* h, const bool gains) {
  DerivState& D = h->dv;
  const size_t B = h->B, N = h->N;
  int rc = 0;
  bool fresh = false;
  if (gains && !D.d_pol_K) rc |= h->dalloc(&D.d_pol_K, B * N * 16), rc |= h->dalloc(&D.d_pol_Kv, B * N * 4), fresh = true;
  if (!gains && !D.d_pol_io) rc |= h->dalloc(&D.d_pol_io, B * 12), fresh = true;
  if (rc) return -1;
  if (fresh) HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------ solve records
// The arrays of a record inside its one device buffer, each 256-byte aligned, in bytes from the start; `end`: the size.
struct RecLayout {
  size_t X, C, U, L1, L2, T, NU, st, x0, uprev, pup, TH, tab, si, orig, K, W, Ws, Wpi, Wspi, end;
};
RecLayout rec_layout(const ltompc_solver* h) {
  const size_t N = h->N, Bp = h->Bp, ni = h->K.bd.ni, nel = h->K.bd.nel, D = sizeof(double);
  RecLayout L{};
  size_t at = 0;
  const auto take = [&](size_t& field, const size_t bytes) { field = at, at += (bytes + 255) / 256 * 256; };
  take(L.X, 8 * (N + 1) * Bp * D), take(L.C, 8 * N * Bp * D), take(L.U, 2 * N * Bp * D), take(L.L1, 8 * N * Bp * D), take(L.L2, 8 * N * Bp * D);
  take(L.T, (ni + NNL + nel) * N * Bp * D), take(L.NU, ni * N * Bp * D), take(L.st, (size_t)ST_NF * Bp * D), take(L.x0, 8 * Bp * D);
  take(L.uprev, 2 * Bp * D), take(L.pup, 2 * Bp * D), take(L.TH, (size_t)LTOMPC_NTHETA * Bp * D);
  take(L.tab, (size_t)LTOMPC_TABLE_VALUE_ROWS * h->n_table * D), take(L.si, (size_t)SI_NF * Bp * sizeof(int)), take(L.orig, Bp * sizeof(int));
  take(L.K, sizeof(Consts)), take(L.W, sizeof(Work)), take(L.Ws, sizeof(Work)), take(L.Wpi, sizeof(WorkPI)), take(L.Wspi, sizeof(WorkPI));
  L.end = at;
  return L;
}

ltompc_record_s* rec_find(ltompc_solver* h, const ltompc_record_s* rec) {
  for (ltompc_record_s* r : h->recs)
    if (r == rec) return r;
  return nullptr;
}
int rec_check(ltompc_solver* h, const ltompc_record_s* rec, const char* who) {
  const ltompc_record_s* r = rec_find(h, rec);
  if (!r) return fail(std::string(who) + ": not a record of this handle (one of another handle, or freed by ltompc_record_trim)");
  if (!r->in_use) return fail(std::string(who) + ": the record has been released (ltompc_record_release)");
  return 0;
}

// A new record: its buffer, the Work / Consts copies that point into it, here and on the device (one synchronisation).  The
// pointers never change afterwards, so a record that is reused or overwritten uploads nothing.
int rec_create(ltompc_solver* h, ltompc_record_s** out) {
  if (sens_buffers(h)) return -1;  // (QP, RC, RS, LS and the zeroed si of the record's Ws are the handle's)
  const RecLayout L = rec_layout(h);
  ltompc_record_s* r = new ltompc_record_s;
  if (h->dalloc(&r->base, L.end)) {
    delete r;
    return -1;
  }
  char* const p = r->base;
  const auto dbl = [&](const size_t at) { return reinterpret_cast<double*>(p + at); };
  r->X = dbl(L.X), r->C = dbl(L.C), r->U = dbl(L.U), r->L1 = dbl(L.L1), r->L2 = dbl(L.L2), r->T = dbl(L.T), r->NU = dbl(L.NU), r->st = dbl(L.st);
  r->x0 = dbl(L.x0), r->uprev = dbl(L.uprev), r->TH = dbl(L.TH), r->tab = dbl(L.tab), r->si = reinterpret_cast<int*>(p + L.si);
  SolveView& v = r->v;
  v.d_psens_uprev = dbl(L.pup);
  v.K = h->K;  // (grids, g0_*, inv_*, period, params, options and the bounds pattern are the handle's and immutable; the value rows the record's)
  using tp = gptr<const double>;
  const size_t n = h->n_table;
  v.K.T.kappa = (tp)r->tab, v.K.T.n_left = (tp)(r->tab + n), v.K.T.n_right = (tp)(r->tab + 2 * n), v.K.T.v_ref = (tp)(r->tab + 3 * n);
  Work& W = v.W = h->W;
  using dp = gptr<double>;
  W.X = (dp)r->X, W.C = (dp)r->C, W.U = (dp)r->U, W.L1 = (dp)r->L1, W.L2 = (dp)r->L2, W.T = (dp)r->T, W.NU = (dp)r->NU, W.st = (dp)r->st;
  W.x0 = (dp)r->x0, W.uprev = (dp)r->uprev, W.si = (gptr<int>)r->si, W.orig = (gptr<const int>)reinterpret_cast<int*>(p + L.orig);
  Work& Ws = v.Ws = W;
  const Work& hs = h->dv.Ws;
  Ws.QP = hs.QP, Ws.RC = hs.RC, Ws.RS = hs.RS, Ws.LS = hs.LS, Ws.si = hs.si;
  static_cast<Work&>(v.Wpi) = W, v.Wpi.TH = (tp)r->TH;
  static_cast<Work&>(v.Wspi) = Ws, v.Wspi.TH = (tp)r->TH;
  v.d_K = reinterpret_cast<Consts*>(p + L.K), v.d_W = reinterpret_cast<Work*>(p + L.W), v.d_Ws = reinterpret_cast<Work*>(p + L.Ws);
  v.d_Wpi = reinterpret_cast<WorkPI*>(p + L.Wpi), v.d_Wspi = reinterpret_cast<WorkPI*>(p + L.Wspi);
  std::vector<int> ident(h->Bp);
  for (int b = 0; b < h->Bp; b++) ident[b] = b;
  hipError_t e = hipMemcpyAsync(p + L.orig, ident.data(), sizeof(int) * h->Bp, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(v.d_K, &v.K, sizeof(Consts), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(v.d_W, &v.W, sizeof(Work), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(v.d_Ws, &v.Ws, sizeof(Work), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(v.d_Wpi, &v.Wpi, sizeof(WorkPI), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(v.d_Wspi, &v.Wspi, sizeof(WorkPI), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    h->dfree(r->base);
    delete r;
    return fail(std::string("ltompc_record_save: upload of the record's constants failed: ") + hipGetErrorString(e));
  }
  h->recs.push_back(r);
  *out = r;
  return 0;
}

// The gather of the solve that the live passes would refer to now into r (enqueued only), and its flags.
int rec_fill(ltompc_solver* h, ltompc_record_s* r) {
  const int N = h->N, Bp = h->Bp, ni = h->K.bd.ni, nel = h->K.bd.nel;
  const Work& W = h->W;
  RecPlanes P{};
  const auto add = [&](const void* src, void* dst, const int rows, const int flags) {
    P.p[P.n++] = RecPlane{(gptr<const void>)src, (gptr<void>)dst, rows, flags}, P.rows += rows;
  };
  add((const double*)W.NU, r->NU, ni * N, 0), add((const double*)W.T, r->T, (ni + NNL + nel) * N, 0), add((const double*)W.X, r->X, 8 * (N + 1), 0);
  add((const double*)W.C, r->C, 8 * N, 0), add((const double*)W.L1, r->L1, 8 * N, 0), add((const double*)W.L2, r->L2, 8 * N, 0);
  add((const double*)W.U, r->U, 2 * N, 0), add((const double*)W.st, r->st, ST_NF, 0), add((const double*)W.x0, r->x0, 8, 0);
  add((const double*)W.uprev, r->uprev, 2, 0);
  for (const int f : {SI_STATUS, SI_NODE0, SI_REINIT})  // (the words d_sens_riccati8 looks at; the other rows stay zero)
    add((const int*)W.si + (size_t)f * Bp, r->si + (size_t)f * Bp, 1, REC_W32);
  add(h->dv.d_psens_uprev, r->v.d_psens_uprev, 2, REC_DIRECT);  // (B x 2 in the caller's order: 2 Bp words as they are)
  if (h->pi_solve) add(h->d_th_solve, r->TH, LTOMPC_NTHETA, REC_DIRECT);
  static_assert(15 <= REC_MAX_PLANES, "k_rec_save's descriptor table");
  const int* inv = nullptr;
  if (h->packed) {
    if (ws_alloc(h)) return -1;
    inv = ws_inverse(h);
  }
  hipLaunchKernelGGL(k_rec_save, dim3((Bp + 255) / 256, (P.rows + REC_ROWS - 1) / REC_ROWS), dim3(256), 0, h->stream, P, inv, h->B, Bp);
  HIPCHECK(hipGetLastError());
  const size_t n = h->n_table, D = sizeof(double);  // value rows: kappa; n_left, n_right, v_ref (rows 1; 3, 4, 5 of d_tables)
  HIPCHECK(hipMemcpyAsync(r->tab, h->d_tables + n, n * D, hipMemcpyDeviceToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(r->tab + n, h->d_tables + 3 * n, 3 * n * D, hipMemcpyDeviceToDevice, h->stream));
  SolveView& v = r->v;
  v.pi_solve = h->pi_solve, v.ts_solve = false, v.n_sets = 0, v.ref_eval = h->ref_eval, v.eval8 = h->eval8, v.kept_uprev = h->dv.kept_uprev;
  v.sens = Sens::solved, v.psens = Psens::none, v.fact = v.pv_valid = false;
  return 0;
}

// A change of selection: what the passes have cached (the factorisation, the PV planes, the results) belongs to the solve they ran on last.
void rec_invalidate(Sens& sens, Psens& psens, bool& fact, bool& pv_valid) {
  if (sens != Sens::no_solve) sens = Sens::solved;
  psens = Psens::none, fact = pv_valid = false;
}
void rec_set_selection(ltompc_solver* h, ltompc_record_s* rec) {
  if (h->rec_sel == rec) return;
  DerivState& D = h->dv;
  rec_invalidate(D.sens, D.psens, D.fact, D.pv_valid);
  if (rec) rec_invalidate(rec->v.sens, rec->v.psens, rec->v.fact, rec->v.pv_valid);
  h->rec_sel = rec;
}

}  // namespace

extern "C" {

long long ltompc_record_size(ltompc_handle h) {
  if (!h) return fail("null handle");
  return (long long)rec_layout(h).end;
}

int ltompc_record_save(ltompc_handle h, ltompc_record* rec) {
  const char* who = "ltompc_record_save";
  if (!h) return fail("null handle");
  if (!rec) return fail(std::string(who) + ": null argument");
  if (*rec && rec_check(h, *rec, who)) return -1;
  if (h->dv.sens == Sens::no_solve) return fail(std::string(who) + ": no solve to differentiate (make_step, make_step_dev or rollout_dev first; set_initial_guess, set_table_values and set_table_sets discard the last solve)");
  if (h->n_sets || h->ts_solve)
    return fail(std::string(who) + ": records of solves with per-instance table sets are out of scope (ltompc_set_table_sets; n_sets = 0 and a new solve bring them back)");
  HIPCHECK(hipSetDevice(h->device));
  ltompc_record_s* r = *rec;
  if (!r) {
    for (ltompc_record_s* f : h->recs)
      if (!f->in_use) r = f;
    if (!r && rec_create(h, &r)) return -1;
  }
  if (rec_fill(h, r)) return -1;
  r->in_use = true;
  *rec = r;
  return 0;
}

int ltompc_record_select(ltompc_handle h, ltompc_record rec) {
  const char* who = "ltompc_record_select";
  if (!h) return fail("null handle");
  if (h->dv.loop_mode) return fail(std::string(who) + ": not available inside an open loop (ltompc_loop_end first)");
  if (rec && rec_check(h, rec, who)) return -1;
  rec_set_selection(h, rec);
  return 0;
}

int ltompc_record_release(ltompc_handle h, ltompc_record rec) {
  const char* who = "ltompc_record_release";
  if (!h) return fail("null handle");
  if (!rec) return fail(std::string(who) + ": null argument");
  if (rec_check(h, rec, who)) return -1;
  if (h->rec_sel == rec) rec_set_selection(h, nullptr);
  rec->in_use = false;
  return 0;
}

int ltompc_record_trim(ltompc_handle h) {
  if (!h) return fail("null handle");
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipStreamSynchronize(h->stream));  // (nothing in flight reads a buffer when it goes)
  std::vector<ltompc_record_s*> kept;
  for (ltompc_record_s* r : h->recs) {
    if (r->in_use) {
      kept.push_back(r);
      continue;
    }
    h->dfree(r->base);
    delete r;
  }
  h->recs.swap(kept);
  return 0;
}

int ltompc_record_stats(ltompc_handle h, int* in_use, int* free_) {
  if (!h) return fail("null handle");
  int n_use = 0;
  for (const ltompc_record_s* r : h->recs) n_use += r->in_use ? 1 : 0;
  if (in_use) *in_use = n_use;
  if (free_) *free_ = (int)h->recs.size() - n_use;
  return 0;
}

int ltompc_get_sensitivities(ltompc_handle h, double* du0_dp, double* dX_dp, double* dU_dp, int* ok, double* margin) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (sens_compute(h, dX_dp || dU_dp, "ltompc_get_sensitivities")) return -1;
  const DerivState& D = h->dv;
  const size_t B = h->B, N = h->N;
  if (copy_out(h, D2H, du0_dp, D.d_sens_du0, 2 * SENS_NP * B) || copy_out(h, D2H, ok, D.d_sens_ok, B) ||
      copy_out(h, D2H, margin, D.d_sens_margin, B) || copy_out(h, D2H, dX_dp, D.d_sens_dX, (N + 1) * 8 * SENS_NP * B) ||
      copy_out(h, D2H, dU_dp, D.d_sens_dU, N * 2 * SENS_NP * B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_sensitivities_dev(ltompc_handle h, double* du0_dp_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (sens_compute(h, false, "ltompc_sensitivities_dev")) return -1;
  if (copy_out(h, D2D, du0_dp_dev, h->dv.d_sens_du0, (size_t)2 * SENS_NP * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_param_sensitivities(ltompc_handle h, double* du0_dth, double* dX_dth, double* dU_dth, int* ok) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (psens_compute(h, dX_dth || dU_dth, "ltompc_get_param_sensitivities")) return -1;
  const DerivState& D = h->dv;
  const size_t B = h->B, N = h->N;
  if (copy_out(h, D2H, du0_dth, D.d_psens_du0, 2 * PS_NT * B) || copy_out(h, D2H, ok, D.d_sens_ok, B) ||
      copy_out(h, D2H, dX_dth, D.d_psens_dX, (N + 1) * 8 * PS_NT * B) || copy_out(h, D2H, dU_dth, D.d_psens_dU, N * 2 * PS_NT * B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_param_sensitivities_dev(ltompc_handle h, double* du0_dth_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (psens_compute(h, false, "ltompc_param_sensitivities_dev")) return -1;
  if (copy_out(h, D2D, du0_dth_dev, h->dv.d_psens_du0, (size_t)2 * PS_NT * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_adjoint_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_p_dev, double* grad_theta_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (adj_compute(h, gX_dev, gU_dev, grad_theta_dev != nullptr, "ltompc_adjoint_dev")) return -1;
  if (copy_out(h, D2D, grad_p_dev, h->dv.d_adj_gp, (size_t)ADJ_NP * h->B)) return -1;
  if (copy_out(h, D2D, grad_theta_dev, h->dv.d_adj_gth, (size_t)PS_NT * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_adjoint(ltompc_handle h, const double* gX, const double* gU, double* grad_p, double* grad_theta, int* ok) {
  const char* who = "ltompc_get_adjoint";
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  if (!gX && !gU) return fail(std::string(who) + ": gX and gU are both NULL (no cotangent)");
  const size_t B = h->B, N = h->N;
  for (size_t b = 0; b < B; b++) {
    bool fin = true;
    for (size_t e = 0; gX && e < (N + 1) * 8; e++) fin = fin && std::isfinite(gX[b * (N + 1) * 8 + e]);
    for (size_t e = 0; gU && e < N * 2; e++) fin = fin && std::isfinite(gU[b * N * 2 + e]);
    if (!fin) return fail(std::string(who) + ": non-finite cotangent of instance " + std::to_string(b));
  }
  HIPCHECK(hipSetDevice(h->device));
  DerivState& D = h->dv;
  if (gX && !D.d_adj_gX && h->dalloc(&D.d_adj_gX, (N + 1) * 8 * B)) return -1;
  if (gU && !D.d_adj_gU && h->dalloc(&D.d_adj_gU, N * 2 * B)) return -1;
  if (gX) HIPCHECK(hipMemcpyAsync(D.d_adj_gX, gX, sizeof(double) * (N + 1) * 8 * B, hipMemcpyHostToDevice, h->stream));
  if (gU) HIPCHECK(hipMemcpyAsync(D.d_adj_gU, gU, sizeof(double) * N * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (adj_compute(h, gX ? D.d_adj_gX : nullptr, gU ? D.d_adj_gU : nullptr, grad_theta != nullptr, who)) return -1;
  if (copy_out(h, D2H, grad_p, D.d_adj_gp, ADJ_NP * B) || copy_out(h, D2H, grad_theta, D.d_adj_gth, PS_NT * B) ||
      copy_out(h, D2H, ok, D.d_sens_ok, B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_adjoint_tables_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_tables_dev, double* slot_grad_dev,
                              int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (tab_compute(h, gX_dev, gU_dev, "ltompc_adjoint_tables_dev")) return -1;
  if (copy_out(h, D2D, grad_tables_dev, h->dv.d_tab_gt, (size_t)TAB_ROWS * h->n_table)) return -1;
  if (copy_out(h, D2D, slot_grad_dev, h->dv.d_tab_sg, (size_t)TS_NS * h->N * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_adjoint_tables_add_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_tables_dev, double* slot_grad_dev,
                                  int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (tab_compute(h, gX_dev, gU_dev, "ltompc_adjoint_tables_add_dev")) return -1;
  if (grad_tables_dev) {
    const int n = TAB_ROWS * h->n_table;
    hipLaunchKernelGGL(k_tab_add, dim3((n + 255) / 256), dim3(256), 0, h->stream, grad_tables_dev, (const double*)h->dv.d_tab_gt, n);
    HIPCHECK(hipGetLastError());
  }
  if (copy_out(h, D2D, slot_grad_dev, h->dv.d_tab_sg, (size_t)TS_NS * h->N * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_adjoint_tables(ltompc_handle h, const double* gX, const double* gU, double* grad_tables, double* slot_grad, int* ok) {
  const char* who = "ltompc_get_adjoint_tables";
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  if (!gX && !gU) return fail(std::string(who) + ": gX and gU are both NULL (no cotangent)");
  const size_t B = h->B, N = h->N;
  for (size_t b = 0; b < B; b++) {
    bool fin = true;
    for (size_t e = 0; gX && e < (N + 1) * 8; e++) fin = fin && std::isfinite(gX[b * (N + 1) * 8 + e]);
    for (size_t e = 0; gU && e < N * 2; e++) fin = fin && std::isfinite(gU[b * N * 2 + e]);
    if (!fin) return fail(std::string(who) + ": non-finite cotangent of instance " + std::to_string(b));
  }
  HIPCHECK(hipSetDevice(h->device));
  DerivState& D = h->dv;
  if (gX && !D.d_adj_gX && h->dalloc(&D.d_adj_gX, (N + 1) * 8 * B)) return -1;
  if (gU && !D.d_adj_gU && h->dalloc(&D.d_adj_gU, N * 2 * B)) return -1;
  if (gX) HIPCHECK(hipMemcpyAsync(D.d_adj_gX, gX, sizeof(double) * (N + 1) * 8 * B, hipMemcpyHostToDevice, h->stream));
  if (gU) HIPCHECK(hipMemcpyAsync(D.d_adj_gU, gU, sizeof(double) * N * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (tab_compute(h, gX ? D.d_adj_gX : nullptr, gU ? D.d_adj_gU : nullptr, who)) return -1;
  if (copy_out(h, D2H, grad_tables, D.d_tab_gt, (size_t)TAB_ROWS * h->n_table) || copy_out(h, D2H, slot_grad, D.d_tab_sg, TS_NS * N * B) ||
      copy_out(h, D2H, ok, D.d_sens_ok, B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

// The same three calls on a handle with per-instance table sets: grad_sets [n_sets][4][n_table], each set's block
// summed over the ok instances of that set; slot_grad and ok as above.
int ltompc_adjoint_table_sets_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_sets_dev, double* slot_grad_dev,
                                  int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (tab_compute(h, gX_dev, gU_dev, "ltompc_adjoint_table_sets_dev", true)) return -1;
  if (copy_out(h, D2D, grad_sets_dev, h->dv.d_tab_gs, (size_t)TAB_ROWS * h->n_table * h->n_sets)) return -1;
  if (copy_out(h, D2D, slot_grad_dev, h->dv.d_tab_sg, (size_t)TS_NS * h->N * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_adjoint_table_sets_add_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_sets_dev, double* slot_grad_dev,
                                      int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (tab_compute(h, gX_dev, gU_dev, "ltompc_adjoint_table_sets_add_dev", true)) return -1;
  if (grad_sets_dev) {
    const int n = TAB_ROWS * h->n_table * h->n_sets;
    hipLaunchKernelGGL(k_tab_add, dim3((n + 255) / 256), dim3(256), 0, h->stream, grad_sets_dev, (const double*)h->dv.d_tab_gs, n);
    HIPCHECK(hipGetLastError());
  }
  if (copy_out(h, D2D, slot_grad_dev, h->dv.d_tab_sg, (size_t)TS_NS * h->N * h->B)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_adjoint_table_sets(ltompc_handle h, const double* gX, const double* gU, double* grad_sets, double* slot_grad, int* ok) {
  const char* who = "ltompc_get_adjoint_table_sets";
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  if (!gX && !gU) return fail(std::string(who) + ": gX and gU are both NULL (no cotangent)");
  const size_t B = h->B, N = h->N;
  for (size_t b = 0; b < B; b++) {
    bool fin = true;
    for (size_t e = 0; gX && e < (N + 1) * 8; e++) fin = fin && std::isfinite(gX[b * (N + 1) * 8 + e]);
    for (size_t e = 0; gU && e < N * 2; e++) fin = fin && std::isfinite(gU[b * N * 2 + e]);
    if (!fin) return fail(std::string(who) + ": non-finite cotangent of instance " + std::to_string(b));
  }
  HIPCHECK(hipSetDevice(h->device));
  DerivState& D = h->dv;
  if (gX && !D.d_adj_gX && h->dalloc(&D.d_adj_gX, (N + 1) * 8 * B)) return -1;
  if (gU && !D.d_adj_gU && h->dalloc(&D.d_adj_gU, N * 2 * B)) return -1;
  if (gX) HIPCHECK(hipMemcpyAsync(D.d_adj_gX, gX, sizeof(double) * (N + 1) * 8 * B, hipMemcpyHostToDevice, h->stream));
  if (gU) HIPCHECK(hipMemcpyAsync(D.d_adj_gU, gU, sizeof(double) * N * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (tab_compute(h, gX ? D.d_adj_gX : nullptr, gU ? D.d_adj_gU : nullptr, who, true)) return -1;
  if (copy_out(h, D2H, grad_sets, D.d_tab_gs, (size_t)TAB_ROWS * h->n_table * h->n_sets) || copy_out(h, D2H, slot_grad, D.d_tab_sg, TS_NS * N * B) ||
      copy_out(h, D2H, ok, D.d_sens_ok, B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_jvp_dev(ltompc_handle h, const double* dp_dev, const double* dtheta_dev, double* tX_dev, double* tU_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (jvp_compute(h, dp_dev, dtheta_dev, tX_dev, tU_dev, "ltompc_jvp_dev")) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_jvp(ltompc_handle h, const double* dp, const double* dtheta, double* tX, double* tU, int* ok) {
  const char* who = "ltompc_get_jvp";
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  if (!dp && !dtheta) return fail(std::string(who) + ": dp and dtheta are both NULL (no direction)");
  const size_t B = h->B, N = h->N;
  for (size_t b = 0; b < B; b++) {
    bool fin = true;
    for (size_t e = 0; dp && e < JVP_NP; e++) fin = fin && std::isfinite(dp[b * JVP_NP + e]);
    for (size_t e = 0; dtheta && e < PS_NT; e++) fin = fin && std::isfinite(dtheta[b * PS_NT + e]);
    if (!fin) return fail(std::string(who) + ": non-finite direction of instance " + std::to_string(b));
  }
  HIPCHECK(hipSetDevice(h->device));
  DerivState& D = h->dv;
  if (!D.d_jvp_dp && (h->dalloc(&D.d_jvp_dp, JVP_NP * B) || h->dalloc(&D.d_jvp_dth, PS_NT * B) || h->dalloc(&D.d_jvp_tX, (N + 1) * 8 * B) ||
                      h->dalloc(&D.d_jvp_tU, N * 2 * B)))
    return -1;
  if (dp) HIPCHECK(hipMemcpyAsync(D.d_jvp_dp, dp, sizeof(double) * JVP_NP * B, hipMemcpyHostToDevice, h->stream));
  if (dtheta) HIPCHECK(hipMemcpyAsync(D.d_jvp_dth, dtheta, sizeof(double) * PS_NT * B, hipMemcpyHostToDevice, h->stream));
  if (jvp_compute(h, dp ? D.d_jvp_dp : nullptr, dtheta ? D.d_jvp_dth : nullptr, tX ? D.d_jvp_tX : nullptr, tU ? D.d_jvp_tU : nullptr, who))
    return -1;
  if (copy_out(h, D2H, tX, D.d_jvp_tX, (N + 1) * 8 * B) || copy_out(h, D2H, tU, D.d_jvp_tU, N * 2 * B) || copy_out(h, D2H, ok, D.d_sens_ok, B))
    return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_jvp_tables_dev(ltompc_handle h, const double* dp_dev, const double* dtables_dev, const double* dslot_dev, double* tX_dev,
                          double* tU_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (tjv_compute(h, dp_dev, dtables_dev, dslot_dev, tX_dev, tU_dev, "ltompc_jvp_tables_dev")) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_jvp_tables(ltompc_handle h, const double* dp, const double* dtables, const double* dslot, double* tX, double* tU, int* ok) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  return tjv_host(h, dp, dtables, dslot, tX, tU, ok, "ltompc_get_jvp_tables", false);
}

// The same two calls on a handle with per-instance table sets: dtables is [n_sets][4][n_table] and instance b
// moves along the block of its set, set_of_instance[b]; dp, dslot and the outputs as above.
int ltompc_jvp_table_sets_dev(ltompc_handle h, const double* dp_dev, const double* dtables_dev, const double* dslot_dev, double* tX_dev,
                              double* tU_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (tjv_compute(h, dp_dev, dtables_dev, dslot_dev, tX_dev, tU_dev, "ltompc_jvp_table_sets_dev", true)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_get_jvp_table_sets(ltompc_handle h, const double* dp, const double* dtables, const double* dslot, double* tX, double* tU, int* ok) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  return tjv_host(h, dp, dtables, dslot, tX, tU, ok, "ltompc_get_jvp_table_sets", true);
}

int ltompc_plant_sensitivities_dev(ltompc_handle h, const double* x_dev, const double* u_dev, int n_sub, double* x_next_dev, double* dxn_dx_dev,
                                   double* dxn_du_dev, double* dxn_dtheta_dev) {
  const char* who = "ltompc_plant_sensitivities";
  if (n_sub < 1) return fail(std::string(who) + ": n_sub must be >= 1");
  if (!h || !x_dev || !u_dev) return fail(std::string(who) + ": null argument");
  if (dxn_dtheta_dev && h->K.p.ptv != 0.0) return fail(std::string(who) + ": dxn_dtheta is not available with torque vectoring (ptv != 0)");
  if (no_table_sets(h, who, "the plant-step sensitivities are")) return -1;
  HIPCHECK(hipSetDevice(h->device));
  if (psn_prepare(h, false)) return -1;
  if (dxn_dx_dev || dxn_du_dev || dxn_dtheta_dev) {
    const double* planes = h->dv.d_psn_planes;
    if (psn_launch(h, x_dev, u_dev, n_sub, dxn_dtheta_dev != nullptr)) return -1;
    if (dxn_dx_dev && planes_to_rows(h, planes, PSN_DX, 64, dxn_dx_dev)) return -1;
    if (dxn_du_dev && planes_to_rows(h, planes, PSN_DU, 16, dxn_du_dev)) return -1;
    if (dxn_dtheta_dev && planes_to_rows(h, planes, PSN_DTH, 8 * PS_NT, dxn_dtheta_dev)) return -1;
  }
  if (x_next_dev) return ltompc_plant_step_dev(h, x_dev, u_dev, n_sub, x_next_dev);  // (k_plant itself: the plant's bits)
  return 0;
}

int ltompc_plant_sensitivities(ltompc_handle h, const double* x, const double* u, int n_sub, double* x_next, double* dxn_dx, double* dxn_du,
                               double* dxn_dtheta) {
  const char* who = "ltompc_plant_sensitivities";
  if (n_sub < 1) return fail(std::string(who) + ": n_sub must be >= 1");
  if (!h || !x || !u) return fail(std::string(who) + ": null argument");
  if (no_table_sets(h, who, "the plant-step sensitivities are")) return -1;
  HIPCHECK(hipSetDevice(h->device));
  if (psn_prepare(h, false)) return -1;
  const size_t B = h->B;
  double *rx = h->dv.d_psn_rm, *ru = rx + 64 * B, *rt = ru + 16 * B;
  return via_io(h, x, u, x_next, [&](double* dx, double* du, double* dn) {
    if (ltompc_plant_sensitivities_dev(h, dx, du, n_sub, dn, dxn_dx ? rx : nullptr, dxn_du ? ru : nullptr, dxn_dtheta ? rt : nullptr)) return -1;
    return copy_out(h, D2H, dxn_dx, rx, 64 * B) || copy_out(h, D2H, dxn_du, ru, 16 * B) || copy_out(h, D2H, dxn_dtheta, rt, 8 * PS_NT * B) ? -1 : 0;
  });
}

int ltompc_loop_begin(ltompc_handle h, int mode) {
  const char* who = "ltompc_loop_begin";
  if (!h) return fail("null handle");
  if (mode < 1 || mode > 3) return fail(std::string(who) + ": mode must be 1 (theta enters the controller), 2 (the plant) or 3 (both)");
  if (no_record(h, who) || no_table_sets(h, who, "the closed-loop sensitivities are")) return -1;
  if (h->K.p.ell_penalty > 0.0) return fail(std::string(who) + ": not available with the friction-ellipse constraints (ell_penalty > 0)");
  if (h->K.p.ptv != 0.0) return fail(std::string(who) + ": not available with torque vectoring (ptv != 0)");
  HIPCHECK(hipSetDevice(h->device));
  if (psn_prepare(h, true)) return -1;
  DerivState& D = h->dv;
  hipLaunchKernelGGL(k_loop_begin, dim3((LOOP_NQ * h->Bp + 255) / 256), dim3(256), 0, h->stream, h->B, h->Bp, D.d_loop_Sx, D.d_loop_Du,
                     D.d_loop_ok, D.d_loop_ticks);
  HIPCHECK(hipGetLastError());
  D.loop_mode = mode;
  return 0;
}

int ltompc_loop_tick_dev(ltompc_handle h, const double* x_dev, const double* u0_dev, int n_sub, double* x_next_dev) {
  const char* who = "ltompc_loop_tick";
  if (n_sub < 1) return fail(std::string(who) + ": n_sub must be >= 1");
  if (!h || !x_dev || !u0_dev || !x_next_dev) return fail(std::string(who) + ": null argument");
  DerivState& D = h->dv;
  if (no_record(h, who)) return -1;
  if (!D.loop_mode) return fail(std::string(who) + ": no loop (ltompc_loop_begin first)");
  if (no_table_sets(h, who, "the closed-loop sensitivities are")) return -1;
  HIPCHECK(hipSetDevice(h->device));
  if (sens_compute(h, false, who)) return -1;  // (the usage error after set_initial_guess comes from here)
  if (!D.kept_uprev) return fail(std::string(who) + ": not available after a rollout (it does not keep the u_prev of each instance's last solve, which the r_du columns need)");
  if (!D.loop_fresh) return fail(std::string(who) + ": no new solve since the last tick (make_step or make_step_dev first)");
  const int mode = D.loop_mode;
  if ((mode & 1) && psens_compute(h, false, who)) return -1;
  if (psn_launch(h, x_dev, u0_dev, n_sub, (mode & 2) != 0)) return -1;
  hipLaunchKernelGGL(k_loop_accum, dim3((LOOP_NQ * h->Bp + 255) / 256), dim3(256), 0, h->stream, h->B, h->Bp, mode, (const double*)D.d_sens_du0,
                     (const double*)((mode & 1) ? D.d_psens_du0 : nullptr), (const int*)D.d_sens_ok, (const double*)D.d_psn_planes, D.d_loop_Sx,
                     D.d_loop_Du, D.d_loop_ok, D.d_loop_ticks);
  HIPCHECK(hipGetLastError());
  D.ticked();
  return ltompc_plant_step_dev(h, x_dev, u0_dev, n_sub, x_next_dev);
}

int ltompc_loop_tick(ltompc_handle h, const double* x, const double* u0, int n_sub, double* x_next) {
  const char* who = "ltompc_loop_tick";
  if (n_sub < 1) return fail(std::string(who) + ": n_sub must be >= 1");
  if (!h || !x || !u0 || !x_next) return fail(std::string(who) + ": null argument");
  HIPCHECK(hipSetDevice(h->device));
  return via_io(h, x, u0, x_next, [&](double* dx, double* du, double* dn) { return ltompc_loop_tick_dev(h, dx, du, n_sub, dn); });
}

int ltompc_get_loop_sensitivities(ltompc_handle h, double* dx_dq, double* du_dq, int* ok, int* ticks) {
  if (!h) return fail("null handle");
  const DerivState& D = h->dv;
  if (!D.d_loop_Sx) return fail("ltompc_get_loop_sensitivities: no loop (ltompc_loop_begin first)");
  HIPCHECK(hipSetDevice(h->device));
  if (copy_out(h, D2H, ok, D.d_loop_ok, h->B) || copy_out(h, D2H, ticks, D.d_loop_ticks, h->B)) return -1;
  if (planes_to_host(h, D.d_loop_Sx, 8 * LOOP_NQ, 1, dx_dq)) return -1;
  if (planes_to_host(h, D.d_loop_Du, 2 * LOOP_NQ, 1, du_dq)) return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_loop_sensitivities_dev(ltompc_handle h, double* dx_dq_dev, double* du_dq_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  const DerivState& D = h->dv;
  if (!D.d_loop_Sx) return fail("ltompc_loop_sensitivities_dev: no loop (ltompc_loop_begin first)");
  HIPCHECK(hipSetDevice(h->device));
  if (dx_dq_dev && planes_to_rows(h, D.d_loop_Sx, 0, 8 * LOOP_NQ, dx_dq_dev)) return -1;
  if (du_dq_dev && planes_to_rows(h, D.d_loop_Du, 0, 2 * LOOP_NQ, du_dq_dev)) return -1;
  return copy_out(h, D2D, ok_dev, D.d_loop_ok, h->B);
}

int ltompc_loop_end(ltompc_handle h) {
  if (!h) return fail("null handle");
  h->dv.loop_mode = 0;
  return 0;
}

int ltompc_get_policy(ltompc_handle h, double* K, double* Kv, int* ok) {
  const char* who = "ltompc_get_policy";
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (pol_prepare(h, false, who)) return -1;
  const DerivState& D = h->dv;
  const size_t B = h->B, N = h->N;
  if (K || Kv) {
    if (pol_staging(h, true) || pol_gather(h, K ? D.d_pol_K : nullptr, Kv ? D.d_pol_Kv : nullptr)) return -1;
  }
  if (copy_out(h, D2H, K, D.d_pol_K, B * N * 16) || copy_out(h, D2H, Kv, D.d_pol_Kv, B * N * 4) || copy_out(h, D2H, ok, D.d_sens_ok, B)) return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_policy_dev(ltompc_handle h, double* K_dev, double* Kv_dev, int* ok_dev) {
  if (!h) return fail("null handle");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (pol_prepare(h, false, "ltompc_policy_dev") || pol_gather(h, K_dev, Kv_dev)) return -1;
  return copy_out(h, D2D, ok_dev, h->dv.d_sens_ok, h->B);
}

int ltompc_policy_step_dev(ltompc_handle h, int k, const double* x_dev, const double* v_dev, int clip, double* u_dev) {
  const char* who = "ltompc_policy_step";
  if (!h || !x_dev || !u_dev) return fail(std::string(who) + ": null argument");
  if (k < 0 || k >= h->N) return fail(std::string(who) + ": k must be in [0, N)");
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (pol_prepare(h, true, who)) return -1;
  const DerivState& D = h->dv;
  hipLaunchKernelGGL(k_policy_step, dim3((h->B + 63) / 64), dim3(64), 0, h->stream, h->K, D.Ws, (const int*)D.d_sens_ok,
                     (const double*)D.d_psens_uprev, k, x_dev, v_dev, clip ? 1 : 0, u_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

int ltompc_policy_step(ltompc_handle h, int k, const double* x, const double* v, int clip, double* u) {
  const char* who = "ltompc_policy_step";
  if (!h || !x || !u) return fail(std::string(who) + ": null argument");
  if (k < 0 || k >= h->N) return fail(std::string(who) + ": k must be in [0, N)");
  const size_t B = h->B;
  for (size_t b = 0; b < B; b++) {
    bool fin = true;
    for (size_t e = 0; e < 8; e++) fin = fin && std::isfinite(x[b * 8 + e]);
    if (!fin) return fail(std::string(who) + ": non-finite x of instance " + std::to_string(b));
    for (size_t e = 0; v && e < 2; e++) fin = fin && std::isfinite(v[b * 2 + e]);
    if (!fin) return fail(std::string(who) + ": non-finite v of instance " + std::to_string(b));
  }
  HIPCHECK(hipSetDevice(h->device));
  if (pol_staging(h, false)) return -1;
  double *dx = h->dv.d_pol_io, *dv = dx + 8 * B, *du = dx + 10 * B;
  HIPCHECK(hipMemcpyAsync(dx, x, sizeof(double) * 8 * B, hipMemcpyHostToDevice, h->stream));
  if (v) HIPCHECK(hipMemcpyAsync(dv, v, sizeof(double) * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (ltompc_policy_step_dev(h, k, dx, v ? dv : nullptr, clip, du)) return -1;
  HIPCHECK(hipMemcpyAsync(u, du, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_policy_run_dev(ltompc_handle h, int k0, int n, double* x_dev, const double* v_dev, int n_sub, int clip, double* u_log_dev,
                          double* x_log_dev) {
  const char* who = "ltompc_policy_run";
  if (!h || !x_dev) return fail(std::string(who) + ": null argument");
  if (k0 < 0 || k0 >= h->N) return fail(std::string(who) + ": k0 must be in [0, N)");
  if (n < 1) return fail(std::string(who) + ": n must be >= 1");
  if (k0 + n > h->N) return fail(std::string(who) + ": k0 + n must be <= N (the policy ends with the horizon)");
  if (n_sub < 1) return fail(std::string(who) + ": n_sub must be >= 1");
  // the plant is the handle's: its tables, rows and sets in effect, as ltompc_plant_step_dev, whatever record is selected
  const Consts K_live = h->K;
  const int n_sets_live = h->n_sets;
  RecScope on_record(h);  // (the selected record, if any, in the handle's place)
  HIPCHECK(hipSetDevice(h->device));
  if (pol_prepare(h, true, who)) return -1;
  const DerivState& D = h->dv;
  const dim3 grid((h->B + 63) / 64), block(64);
  const int* ok = D.d_sens_ok;
  const double* up = D.d_psens_uprev;
  const int c = clip ? 1 : 0;
  if (n_sets_live)
    hipLaunchKernelGGL(k_policy_run_ts, grid, block, 0, h->stream, K_live, D.Ws, ok, up, k0, n, x_dev, v_dev, n_sub, c, u_log_dev, x_log_dev,
                       (const double*)(h->pi_pend ? h->d_th_pend : h->d_th_unif), (const double*)h->d_ts_vals, (const int*)h->d_ts_idx);
  else if (h->pi_pend)
    hipLaunchKernelGGL(k_policy_run_pi, grid, block, 0, h->stream, K_live, D.Ws, ok, up, k0, n, x_dev, v_dev, n_sub, c, u_log_dev, x_log_dev,
                       (const double*)h->d_th_pend);
  else hipLaunchKernelGGL(k_policy_run, grid, block, 0, h->stream, K_live, D.Ws, ok, up, k0, n, x_dev, v_dev, n_sub, c, u_log_dev, x_log_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

int ltompc_policy_last_dev(ltompc_handle h, int n, const double* u_log_dev, double* u_dev) {
  const char* who = "ltompc_policy_last_dev";
  if (!h || !u_log_dev || !u_dev) return fail(std::string(who) + ": null argument");
  if (n < 1) return fail(std::string(who) + ": n must be >= 1");
  HIPCHECK(hipSetDevice(h->device));
  const size_t row = 2 * sizeof(double);  // rows of 16 bytes, n rows apart in the log
  HIPCHECK(hipMemcpy2DAsync(u_dev, row, u_log_dev + (size_t)2 * (n - 1), row * n, row, h->B, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

}  // extern "C"
