/*
 * ltompc.h — C ABI of the MI355X-native receding-horizon NLP solver (libltompc.so).
 *
 * Drop-in boundary for the one hot path of bruno-maruszczak/lap-time-optimization:
 *     u0 = controller.mpc.make_step(x0)                      reference src/mpc.py:142
 * i.e. do_mpc's MPC object as configured by src/mpc/controller.py:9-103 over the model of
 * src/mpc/model.py:130-185 and the look-up tables of src/path.py:96-101, src/mpc/track.py:30-42.
 * The reference has no FFI of its own (it is pure Python over do_mpc/CasADi/IPOPT); the entry points
 * below are what a ctypes binding for that path binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - all floating point is IEEE double; all arrays are plain C arrays, row-major, no torch types;
 *   - state  x = [s, n, mu, vx, vy, r, steering_angle, throttle]          (model.py:138-147)
 *     input  u = [steering_angle_change, throttle_change]                  (model.py:149-150)
 *   - a handle owns B independent MPC instances ("batch"); instance b is row b of every array;
 *   - every function returns 0 on success, <0 on a usage / HIP error (ltompc_last_error() has the text).
 *     Solver non-convergence is NOT an error (the reference returns IPOPT's last iterate silently,
 *     SURVEY.md §8b): it is reported per instance in `status`.
 *   - a handle is not thread-safe; distinct handles are independent.  Calls are synchronous unless the
 *     name ends in _async (those only enqueue on the handle's stream).
 */
#ifndef LTOMPC_H
#define LTOMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define LTOMPC_NX 8
#define LTOMPC_NU 2
#define LTOMPC_NO_BOUND 1.0e30 /* |bound| >= this means "not set" (controller.py:78 `not_set`) */
#define LTOMPC_TABLE_ROWS 6    /* s_kappa, kappa, s_arc, n_left, n_right, v_ref */
#define LTOMPC_NTHETA 16       /* columns of ltompc_get_param_sensitivities (order given there)   */
#define LTOMPC_NLOOP 24        /* columns of ltompc_get_loop_sensitivities: x_init[0..7], theta[0..15] */

/* per-instance solver status written by make_step */
#define LTOMPC_STATUS_SOLVED 0          /* scaled KKT error <= tol                                */
#define LTOMPC_STATUS_ACCEPTABLE 1      /* <= acceptable_tol for acceptable_iter iterations       */
#define LTOMPC_STATUS_MAX_ITER 2        /* iteration budget exhausted, last iterate returned      */
#define LTOMPC_STATUS_NUMERICAL 3       /* non-finite value / regularisation overflow             */
#define LTOMPC_STATUS_STALLED 4         /* no progress and the restoration phase could not help (or is
                                           switched off): IPOPT's 'restoration failed'              */
#define LTOMPC_STATUS_INFEASIBLE 5      /* the restoration phase converged, at its largest penalty
                                           (options.resto_rho_max), to a point where a track constraint stays
                                           violated by more than tol: a stationary point of the constraint
                                           violation up to 1 / resto_rho_max (IPOPT: 'converged to a point of
                                           local infeasibility'); that least-violation iterate is returned.
                                           Also: the measured state x0 itself violates a track constraint
                                           (options.node0_check: the reference's NLP has no feasible point) */

/* Vehicle + objective + bounds.  Defaults (ltompc_default_params) are the values the reference
 * actually uses, including its quirks: D_f = D_r = 1.0 because model.py:42-64
 * never reads them; car length in the boundary constraint is length_f + length_r (model.py:71). */
typedef struct ltompc_params {
  /* model.py:42-64, constructor defaults :16-29 */
  double mass, inertia_z, length_f, length_r, width;
  double B_f, C_f, D_f, B_r, C_r, D_r;
  double C_m, Cr_0, Cr_2, gravity;
  /* Torque vectoring (model.py:162-164, disabled in the reference: `Mtv = 0.0`, the line `Mtv = ptv * (rt - r)` with
   * rt = tan(delta) vx / (l_f + l_r) is commented out): yaw moment added to the r equation.  0 = the reference. */
  double ptv;
  /* controller.py:29,52-53: lterm = q_n n^2 + q_mu mu^2 + q_vy vy^2 + q_v (vx - vref_scale*v_ref(s))^2
   *                                 + q_B (atan(vy/vx) - atan(delta*l_r/(l_f+l_r)))^2 ; mterm = first three.
   * controller.py:40-41 + mpc.py:104: rterm = sum_i r_du[i] * (u_k[i] - u_{k-1}[i])^2                  */
  double q_n, q_mu, q_vy, q_v, vref_scale, q_B;
  double r_du[LTOMPC_NU];
  /* controller.py:79-103 (LTOMPC_NO_BOUND where the reference sets nothing) */
  double x_lb[LTOMPC_NX], x_ub[LTOMPC_NX];
  double u_lb[LTOMPC_NU], u_ub[LTOMPC_NU];
  /* Friction-ellipse constraints of the two axles (model.py:86-99 get_traction_ellipse_constraint; their registration as
   * soft nl constraints is commented out in the reference, controller.py:72-74: ell_penalty = 0 is the reference).
   *   long = ell_rho 0.5 C_m T ;  g_a = (long^2 + F_y,a^2) / ell_D_a^2 - 1 <= 0 at the nodes 1 .. N-1, a = front, rear,
   * always with an elastic variable that costs ell_penalty (do_mpc: soft_constraint=True, penalty_term_cons).  With
   * ell_D_f = ell_D_r = 1.0 (= alpha D with the reference's alpha = 1 and D = 1.0) and ell_rho = 1 this is the reference's
   * expression, which no tyre force in newtons can satisfy; a physical radius is the peak lateral force F_N D. */
  double ell_penalty, ell_rho, ell_D_f, ell_D_r;
} ltompc_params;

/* NLP transcription + interior-point options.  Defaults follow do_mpc 4.6.5 / IPOPT 3.14 defaults
 * as listed in SURVEY.md App. B (t_step, Radau-IIA deg 2, tol 1e-8, mu_init 0.1, monotone mu, ...). */
typedef struct ltompc_options {
  double t_step;          /* controller.py:9            0.1  */
  double tol;             /* ipopt tol                  1e-8 */
  double acceptable_tol;  /* ipopt acceptable_tol       1e-6 */
  double mu_init;         /* ipopt mu_init              0.1  */
  double mu_min;          /* tol/10                     1e-9 */
  double kappa_eps;       /* barrier_tol_factor         10   */
  double kappa_mu;        /* mu_linear_decrease_factor  0.2  */
  double theta_mu;        /* mu_superlinear_decrease_power 1.5 */
  double tau_min;         /* fraction-to-boundary       0.99 */
  double bound_push;      /* slack initialisation       1e-2 */
  double s_max;           /* dual-residual scaling cap  100  */
  double delta_w_first;   /* first Hessian regularisation 1e-4 */
  /* Smoothing of the reference NLP's kinks (|mu| in model.py:77-78, table knots): eps = max(smooth_eps_min,
   * smooth_scale * mu_barrier) in rad resp. metres; both 0 = the exact non-smooth functions. */
  double smooth_eps_min;  /* 1e-4 */
  double smooth_scale;    /* 1.0  */
  /* Barrier parameter at the start of a WARM-started solve (every make_step after the first).  0 = use mu_init, which
   * is what do_mpc/IPOPT do (IPOPT restarts at mu_init = 0.1 on every call); a smaller value (1e-3 .. 1e-2) keeps
   * the iterates close to the previous solution and saves iterations without changing the KKT point found. */
  double mu_init_warm;    /* 0 */
  /* Softened track constraints (do_mpc: set_nl_cons(..., soft_constraint=True, penalty_term_cons=soft_rho)).
   * 0 = hard constraints gL, gR <= 0 as in the reference (controller.py:69-70).  > 0: every track constraint of every
   * node gets an elastic variable e >= 0 (g - e <= 0) that costs soft_rho * e (exact L1 penalty: the solution is the
   * hard-constrained one wherever that exists and soft_rho exceeds its multipliers, a least-violation one otherwise).
   * It also is what keeps the closed loop going: from some states the lap reaches, the hard-constrained solve stalls
   * (no restoration phase here) or has no feasible point at all, and every later tick inherits the failure; with
   * soft_rho = 100 all 769 ticks of the buckmore lap converge.  The elastic variables are eliminated
   * with the slacks: same stage-QP sizes, same kernels, three more planes per interval. */
  double soft_rho;        /* 0 */
  /* Restoration phase (what IPOPT enters when its filter line search fails).  Here it is an ELASTIC mode:
   * the solve is continued on the same NLP with every track constraint relaxed by an elastic variable e >= 0 that
   * costs resto_rho * e (the machinery of soft_rho, with IPOPT's restoration penalty 1000), the barrier parameter and
   * the slacks re-centred.  When the elastic problem has converged with all e <= tol the iterate is a KKT point of the
   * hard-constrained NLP: the solve switches back to the hard constraints and terminates there (status SOLVED);
   * with some e > tol the problem is locally infeasible (status INFEASIBLE).  0 = no restoration: a failed line
   * search ends the solve with status STALLED after max_ls_fail attempts, as in round 1. */
  double resto_rho;       /* 1000 */
  /* Penalty escalation of the restoration phase.  An elastic problem that has converged with an elastic variable > tol has
   * only shown that, at its penalty, violating is cheaper than complying (the multiplier of that constraint sits at the
   * penalty); a feasible NLP whose multipliers exceed resto_rho ends there too.  So the penalty of THAT instance is
   * multiplied by resto_rho_factor (elastic variables, slacks, barrier re-centred at the current primal point, as at the
   * entry of the phase) and the elastic problem is solved again, until all elastic variables are <= tol (back to the hard
   * constraints, status SOLVED) or the penalty has reached resto_rho_max: only then the status is INFEASIBLE, a stationary
   * point of  objective / resto_rho_max + violation,  i.e. of the constraint violation itself up to 1 / resto_rho_max (IPOPT's
   * restoration phase minimises the violation alone; at 1e7 the escalated problems sit at the rounding floor and take 2 - 4
   * times the iterations, at 1e6 the least violation is reproduced to 2 % down to violations of 1e-5 m).  resto_rho_factor <= 1 or resto_rho_max <= resto_rho: no escalation,
   * INFEASIBLE means "at penalty resto_rho" (round 2's behaviour). */
  double resto_rho_max;    /* 1e6 */
  double resto_rho_factor; /* 1e3 (one step to resto_rho_max) */
  /* Early entry into the recovery steps (shifted restart, restoration phase): on the hard constraints, an iterate whose dual
   * infeasibility (max-norm of the Lagrangian's gradient, unscaled) exceeds this.  On this NLP a solve that converges stays
   * below 1e3 .. 1e4 after a warm start; the solves that exceed it are the ones whose multipliers diverge (1e5 -> 1e18) while
   * the filter keeps accepting steps of a percent - 100 to 250 iterations until the line search finally fails, the slowest
   * instances of every tick.  IPOPT has no such test (it would iterate on); it only changes WHEN the recovery starts, not
   * what the solve returns when it converges.  Warm-started solves only (from do_mpc's cold start, every node = x0, a
   * converging solve passes through dual infeasibilities of 1e7).  0 = off. */
  double dual_inf_max;     /* 1e4 */
  int max_iter;           /* controller.py:18 says 1000.  Per instance: iterations plus repeated Riccati sweeps (inertia correction) */
  int acceptable_iter;    /* ipopt acceptable_iter      15   */
  int n_linesearch;       /* step-size candidates alpha_max * 2^-l, l = 0..n_linesearch-1 */
  int stall_iter;         /* stop (status STALLED) after this many consecutive steps with alpha <= 1e-3; 0 = off */
  int max_ls_fail;        /* stop (status STALLED) after this many failed line searches in one solve; 0 = off.
                             IPOPT would enter its restoration phase at the first one and, on a locally infeasible
                             problem, end with 'restoration failed'                                       (8) */
  int warm_shift;         /* 0 (do_mpc: previous solution re-used as is) | 1: a warm start shifts the previous solution
                             by one interval (x_k <- x_{k+1}, ..., last interval repeated) before solving      (0) */
  int warm_reset_on_fail; /* 1: a warm start after a solve that did NOT converge keeps that solve's primal point but
                             restarts the equality multipliers at 0 and the barrier at mu_init (IPOPT's default
                             warm_start_init_point=no never re-uses multipliers; ours are re-used after a converged
                             solve only, the ones of a failed solve are what diverged) | 0: always re-use       (1) */
  int periodic_tables;    /* 0: tables extrapolate linearly beyond their ends (CasADi's interpolant, the reference) | 1: the track is a
                             closed loop, tables are evaluated at s modulo their span (buckmore: kappa, n_left, n_right
                             agree at both ends, v_ref to 0.2 %), so that the closed loop can run lap after lap; the kink
                             at the seam is not rounded.  One period serves both grids: ltompc_create
                             refuses tables whose s_arc and s_kappa grids differ in their first knot or in their span by
                             more than 1e-9 of the span (they would wrap n_left, n_right and v_ref at the wrong place) (0) */
  int max_soc;            /* second-order corrections per iteration (IPOPT's max_soc): when the full step is rejected and
                             does not reduce the constraint violation, the step is re-computed with the constraint
                             residuals of the trial point added (same KKT matrix, new right-hand side: a Riccati sweep
                             over the vectors only).  Implemented in the oracle, where it was measured not to change
                             the iteration counts of this NLP; the device library accepts 0 only    (0) */
  int resto_sticky;       /* > 0: an instance whose solve entered the restoration phase from the hard constraints, or ended
                             INFEASIBLE, starts its next resto_sticky warm-started solves directly in elastic mode (no
                             second jam on the hard constraints first: 10 - 15 iterations saved per solve, and these are
                             the instances that make the tail of a tick); the count is renewed while that keeps
                             happening.  A solve that starts in elastic mode ends like any restoration: back on the hard
                             constraints when every elastic variable is <= tol (status SOLVED), INFEASIBLE otherwise.
                             0: every solve starts on the hard constraints (IPOPT).                              (0) */
  int node0_check;        /* do_mpc registers the track constraints at the nodes 0 .. N-1 (controller.py:69-70); node 0 is the measured
                             state, so its two rows are constants: they cannot change the minimiser, but when x0 violates them
                             the reference's NLP has no feasible point whatever the solver does.  1: the solve runs as always
                             (the rows of node 0 left out), and a measured state with g(x0) > acceptable_tol turns a converged
                             status into INFEASIBLE (violation = g(x0)), one with tol < g(x0) <= acceptable_tol turns SOLVED into
                             ACCEPTABLE (IPOPT's error then cannot fall below g(x0)).  0: node 0 ignored (round 2).       (1) */
  int warm_fallback_iter; /* safeguard of options.mu_init_warm: a warm-started solve that began at mu_init_warm and has gone this
                             many iterations without a decrease of the barrier parameter (it is cycling: the small barrier
                             keeps it at a point that is not central) starts again from its current primal point with the
                             equality multipliers at 0 and the barrier at mu_init, once per solve.  0 = off.          (25) */
  int resto_shift_retry;  /* 1: before the restoration phase proper, a WARM-started solve whose line search has failed (or
                             stalled) starts once more on the hard constraints from its own starting point moved one interval
                             ahead (options.warm_shift's rule), multipliers 0, barrier at mu_init.  do_mpc re-uses the previous
                             solution un-shifted, one interval behind the new measured state, and that mismatch is what jams
                             many of these solves: from the shifted point they converge in ~15 iterations where the elastic
                             problem started at the jam point drifts into a local minimum of the violation.
                             0: straight to the restoration phase (round 2).  Ignored with warm_shift = 1.            (1) */
  int max_mu_stay;        /* warm-started solves: after this many iterations without a decrease of the barrier parameter the
                             iterates are wandering or cycling (the filter holds 16 pairs and forgets the oldest; a solve that
                             converges needs ~60 at most on this NLP; one cycling instance running to max_iter = 1000 costs a
                             tick of 8192 instances 200 ms).  On the hard constraints the recovery steps take over (shifted
                             restart, restoration phase), elsewhere the solve ends with status STALLED.  0 = off.        (100) */
  int infeasible_sticky;  /* 1: a warm-started solve that follows one the solver ended INFEASIBLE (its own verdict, at the largest
                             penalty - not the node-0 rule) starts where that one ended: in the escalated elastic problem, from
                             its primal point and multipliers, instead of going through hard attempt, shifted restart and the
                             elastic problem at resto_rho again (~100 passes; a car that cannot make the corner stays infeasible
                             for several ticks, and such chronic cases are the slowest instances of every tick).  It ends like
                             any restoration: back on the hard constraints when every elastic variable is <= tol (SOLVED),
                             INFEASIBLE otherwise.  0: every solve starts on the hard constraints (IPOPT).              (1) */
  int latency_mode;       /* which evaluation kernels a handle uses, fixed at create: 2 = thread per (interval, instance)
                             (fewest instructions per instance: throughput), 1 = 8 lanes per (interval, instance)
                             (k_eval8 / k_expand8: a third of the latency per launch, 3x the time at full load),
                             0 = 1 for batches of at most 64 instances, else 2.  The two agree to ~1e-12 per iteration;
                             bit-identical results across batches hold between handles of the same mode.     (0) */
} ltompc_options;

typedef struct ltompc_solver* ltompc_handle;

void ltompc_default_params(ltompc_params* p);
void ltompc_default_options(ltompc_options* o);
const char* ltompc_last_error(void);
const char* ltompc_version(void);

/* Replaces Controller(model, control_costs, n_horizon, t_step) + mpc.setup()   (controller.py:9-34).
 * tables: LTOMPC_TABLE_ROWS x n_table doubles, row-major (rows as named above; path.py:96-101,
 *         mpc/track.py:30-42).  n_horizon = N; batch = number of independent MPC instances;
 * device: HIP device ordinal.  Allocates every device workspace; no allocation happens per call later, except the workspaces
 * of the sensitivity pass (ltompc_get_sensitivities / ltompc_sensitivities_dev), allocated on the handle's first request for
 * sensitivities: a handle that never asks for them pays nothing. */
int ltompc_create(const ltompc_params* params, const ltompc_options* options, const double* tables,
                  int n_table, int n_horizon, int batch, int device, ltompc_handle* out);
int ltompc_destroy(ltompc_handle h);

/* Run on this HIP stream (hipStream_t as void*); NULL = the handle's own stream. */
int ltompc_set_stream(ltompc_handle h, void* hip_stream);

/* Replaces `mpc.x0 = x0; mpc.set_initial_guess()`  (mpc.py:117-118): every state slot of instance b := x0[b],
 * every input := 0, u_prev := 0, multipliers reset.  x0: batch x 8 (host). */
int ltompc_set_initial_guess(ltompc_handle h, const double* x0);

/* Replaces `u0 = mpc.make_step(x0)`  (mpc.py:142).  Solves the B NLPs warm-started from the handle's
 * previous solution (un-shifted, like do_mpc), u_prev := last returned u0.
 *   x0: batch x 8 (host, in)      u0: batch x 2 (host, out)
 *   status, iters: batch ints (host, out; may be NULL). */
int ltompc_make_step(ltompc_handle h, const double* x0, double* u0, int* status, int* iters);

/* Same, device pointers, enqueue only (x0_dev: batch x 8, u0_dev: batch x 2, row-major, on the handle's
 * device; u0_dev may be NULL).  Converged instances idle; the host stops launching iterations once a polled
 * device counter says every instance has terminated (ltompc_set_poll_every).  Kernels run on the handle's
 * stream; the call returns after the last poll, the final u0 store may still be in flight on that stream. */
int ltompc_make_step_dev(ltompc_handle h, const double* x0_dev, double* u0_dev);

/* Waits until everything the handle has enqueued on its stream (the _dev entry points only enqueue) has completed. */
int ltompc_synchronize(ltompc_handle h);

/* Closed-loop rollout with FREE-RUNNING instances: every instance does n_ticks of the reference's loop body (src/mpc.py:140-153:
 * u0 = make_step(x0); x0 = plant(x0, u0)), but an instance that has converged takes its plant step and starts its next tick
 * inside the running batch instead of waiting for the slowest instance of the tick (no coupling exists between instances;
 * with make_step 40 % of a tick is spent on the 4 % of instances that need many iterations).  Per instance the
 * sequence of solves is exactly the one of make_step + plant_step in a loop: controls, statuses and iteration counts are
 * bit-identical (tests/test_gpu_parity.py).  Starts from the handle's current guess / warm start like make_step.
 *   x_dev: batch x 8 (device, in: states at tick 0, out: states after n_ticks); n_sub: RK4 sub-steps of the plant;
 *   u_log_dev: batch x n_ticks x 2, status_log_dev, iters_log_dev: batch x n_ticks (device, out; any may be NULL).
 * Synchronous.  Afterwards the handle holds every instance's last solution (warm start of a following make_step / rollout). */
int ltompc_rollout_dev(ltompc_handle h, double* x_dev, int n_ticks, int n_sub, double* u_log_dev, int* status_log_dev,
                       int* iters_log_dev);
/* interior-point iterations launched and kernel launches of the last rollout */
int ltompc_rollout_info(ltompc_handle h, long long* iterations, long long* launches);

/* Predicted trajectories of the last solve (do_mpc: mpc.opt_x_num['_x', k, 0, -1], ['_u', k, 0]).
 *   X: batch x (N+1) x 8, U: batch x N x 2 (host, out; either may be NULL). */
int ltompc_get_prediction(ltompc_handle h, double* X, double* U);

/* Per-instance results of the last solve (host, out; any may be NULL):
 *   status, iters: ints;  kkt_error: scaled KKT error E_0;  objective: NLP objective J;  mu: last barrier. */
int ltompc_get_stats(ltompc_handle h, int* status, int* iters, double* kkt_error, double* objective,
                     double* mu);

/* Full primal/dual iterate of the last solve, for KKT checks (host, out; any may be NULL):
 *   X: B x (N+1) x 8, C: B x N x 8 (first Radau point), U: B x N x 2,
 *   L1, L2: B x N x 8 (collocation multipliers).                                   */
int ltompc_get_iterate(ltompc_handle h, double* X, double* C, double* U, double* L1, double* L2);

/* Slacks t and multipliers nu of the inequality constraints of the last solve (host, out; any may be NULL):
 * B x N x n_ineq, per interval k: input bounds (lower, upper per input), bounds on the Radau point, bounds on
 * node k+1 (per state lower then upper, only the bounds that are set), gL, gR+, gR- at node k+1. */
int ltompc_get_ineq(ltompc_handle h, double* T, double* NU, int* n_ineq);

/* Plant step: replaces sim.make_step(u0) (src/mpc/simulator.py:18-20, mpc.py:143): integrates the model ODE
 * over t_step under zero-order-hold u with n_sub classical RK4 sub-steps.  x, x_next: batch x 8; u: batch x 2
 * (host).  _dev variant: device pointers, enqueue only. */
int ltompc_plant_step(ltompc_handle h, const double* x, const double* u, int n_sub, double* x_next);
int ltompc_plant_step_dev(ltompc_handle h, const double* x_dev, const double* u_dev, int n_sub,
                          double* x_next_dev);

/* Slip angles and Pacejka lateral forces (model.py:101-114; called per tick at mpc.py:148-150).
 * x: batch x 8 -> alpha: batch x 2 (front, rear), Fy: batch x 2.  Host pointers, computed on the device. */
int ltompc_slip_forces(ltompc_handle h, const double* x, int batch, double* alpha, double* Fy);

/* Device-pointer form of ltompc_set_initial_guess (enqueue only). */
int ltompc_set_initial_guess_dev(ltompc_handle h, const double* x0_dev);

/* Per-instance counters of the last solve: Hessian-regularisation retries, failed line searches (host, out). */
int ltompc_get_counters(ltompc_handle h, int* n_reg, int* n_lsfail);

/* Restoration phase of the last solve (host, out; any may be NULL): how often an instance entered it (0 or 1), and the
 * largest elastic variable at termination, i.e. the remaining violation of the track constraints in metres (> tol for
 * status INFEASIBLE; 0 for instances that ended on the hard constraints). */
int ltompc_get_restoration(ltompc_handle h, int* n_resto, double* violation);

/* Recovery steps of the last solve (host, out; any may be NULL): n_shift - the solve started again from its shifted starting
 * point (options.resto_shift_retry; 0 or 1); n_fallback - a tuned warm start fell back to mu_init (options.warm_fallback_iter);
 * g0 - the largest track constraint at the measured state x0 (options.node0_check; > 0: x0 is outside the band);
 * solver_status - the solver's own termination status, before the node-0 rule; penalty - the elastic variables' penalty at
 * termination (0: hard constraints; resto_rho_max for status INFEASIBLE after an escalated restoration). */
int ltompc_get_recovery(ltompc_handle h, int* n_shift, int* n_fallback, double* g0, int* solver_status, double* penalty);

/* Parametric sensitivities of the last solve's solution w.r.t. p = (x0[0..7], u_prev[0..1]): 10 columns, in that order.
 * u_prev is the previous input of the Delta-u cost that solve used (0 after set_initial_guess, the u0 of the solve before otherwise).
 *
 * Definition.  For an instance whose last solve ended with the solver's own status SOLVED or ACCEPTABLE (solver_status of
 * ltompc_get_recovery, i.e. before the node-0 rule) these are the derivatives of the solution of the BARRIER problem at the
 * final iterate - the final barrier parameter and the final table smoothing - obtained from the KKT matrix at that iterate
 * with delta_w = 0 (implicit-function theorem, as in sIPOPT).  du0/dx0 = K_0 and du0/du_prev = Kv_0, the
 * stage-0 gains of the Riccati factorisation of that matrix.  An instance that the node-0 rule reports as INFEASIBLE is covered
 * the same way: its u0 is the control of the NLP without the constant node-0 rows, and these are that NLP's sensitivities.
 *   ok[b] = 1 when the status condition holds, the factorisation at delta_w = 0 passes the inertia test (every stage's Huu
 *   positive definite: the reduced Hessian is positive definite) and every output is finite.  Otherwise ok[b] = 0 and every
 *   output of the instance (margin included) is exactly 0 - not NaN: a caller that applies the feedback blindly gets u0.
 *   margin[b] = min over the (slack, multiplier) pairs of the inequalities of max(t, nu), unscaled.  In an interior-point
 *   solution t nu ~ mu; a small margin (<< 1) marks a weakly active constraint, where the true derivative is one-sided and
 *   the barrier derivative a smoothed value.
 *
 * ltompc_get_sensitivities: host outputs in the caller's instance order, any may be NULL:
 *   du0_dp  batch x 2 x 10;
 *   dX_dp   batch x (N+1) x 8 x 10, row block 0 is [I_8 | 0] (by definition);
 *   dU_dp   batch x N x 2 x 10, block 0 equals du0_dp;
 *   ok      batch ints;  margin  batch doubles.
 * ltompc_sensitivities_dev: enqueues only, on the handle's stream: du0_dp_dev (row-major batch x 2 x 10) and ok_dev (batch
 *   ints), device pointers, either may be NULL.  This is the feedback use (u = u0 + du0_dp (p - p_solved)): no host round trip.
 *   Exception: the FIRST request for sensitivities on a handle (either function) allocates the pass's workspaces and
 *   synchronises the handle's stream once; call one of them once after the first solve (e.g. with NULL outputs) to keep
 *   every later call asynchronous.
 *
 * The result refers to the last solve of each instance (make_step, make_step_dev or rollout_dev).  It is computed on the
 * first request after that solve (re-linearisation at the final iterate, a head-less Riccati sweep, the forward propagation
 * of the 10 directions; the trajectories only when dX_dp or dU_dp is asked for) and cached until the next solve,
 * set_initial_guess or set_initial_guess_dev.  Before any solve, and after set_initial_guess, a call is a usage error.  The
 * pass writes buffers of its own only: every later make_step or rollout gives the bits it would have given without it. */
int ltompc_get_sensitivities(ltompc_handle h, double* du0_dp, double* dX_dp, double* dU_dp, int* ok, double* margin);
int ltompc_sensitivities_dev(ltompc_handle h, double* du0_dp_dev, int* ok_dev);

/* Parametric sensitivities of the last solve's solution w.r.t. the vehicle and cost parameters theta: LTOMPC_NTHETA = 16
 * columns, in this order and in natural units (the fields of ltompc_params):
 *     mass, inertia_z, B_f, C_f, D_f, B_r, C_r, D_r, C_m, Cr_0, Cr_2, q_n, q_mu, q_B, r_du[0], r_du[1].
 * Not covered: the geometry (length_f, length_r, width, gravity: it also enters the track constraints), q_vy, q_v,
 * vref_scale, ptv and the friction-ellipse parameters.  A handle with ell_penalty > 0 or ptv != 0 is a usage error; soft
 * track constraints (soft_rho > 0) are covered (the track constraints do not depend on theta).
 *
 * Definition: that of ltompc_get_sensitivities - the barrier problem at the final iterate with the final barrier parameter
 * and table smoothing, the KKT matrix with delta_w = 0, the same instances (solver status SOLVED or ACCEPTABLE before the
 * node-0 rule), dz/dtheta = -F_z^-1 F_theta.  theta enters every stage (the dynamics in both collocation
 * equations and in the Lagrangian's mixed second derivatives, the weights in the cost gradient), so the initial state
 * and input do not move: dX block 0 is 0, and dU_k = K_k dX_k + Kv_k dV_k + kff_k with a right-hand side of its own per column.
 *   ok[b] equals ltompc_get_sensitivities' ok[b] bit for bit; every output of an instance with ok[b] = 0 is exactly 0.
 *
 * ltompc_get_param_sensitivities: host outputs in the caller's instance order, any may be NULL:
 *   du0_dth  batch x 2 x 16;   dX_dth  batch x (N+1) x 8 x 16 (block 0 is 0);   dU_dth  batch x N x 2 x 16;   ok  batch ints.
 * ltompc_param_sensitivities_dev: enqueues only, on the handle's stream: du0_dth_dev (batch x 2 x 16) and ok_dev (batch
 *   ints), device pointers, either may be NULL.  The first request for any sensitivities on a handle allocates and
 *   synchronises once, as for ltompc_sensitivities_dev; the first request for these allocates their own buffers the same way.
 *
 * Computed on the first request after a solve and cached until the next solve, set_initial_guess or set_initial_guess_dev;
 * before any solve, after set_initial_guess and after rollout_dev a call is a usage error (the r_du columns need u_0 - u_prev
 * of the solve: make_step keeps u_prev for them, the rollout does not).  The pass re-uses the re-linearisation and the
 * delta_w = 0 factorisation of ltompc_get_sensitivities when that ran for the same solve (and the other way round) and
 * writes buffers of its own only: neither pass changes the other's results, and every later make_step or rollout gives the
 * bits it would have given without it. */
int ltompc_get_param_sensitivities(ltompc_handle h, double* du0_dth, double* dX_dth, double* dU_dth, int* ok);
int ltompc_param_sensitivities_dev(ltompc_handle h, double* du0_dth_dev, int* ok_dev);

/* Adjoint sensitivities of the last solve: the gradient of a scalar loss L(X, U) of the predicted trajectory
 * w.r.t. p = (x0[0..7], u_prev[0..1]) and theta (the LTOMPC_NTHETA = 16 columns above), from its cotangents gX = dL/dX and
 * gU = dL/dU, without forming a Jacobian.  For instance b:
 *     grad_p[j]     = sum_{k,i} gX[k,i] dX_dp[k,i,j]  + sum_{k,c} gU[k,c] dU_dp[k,c,j],     j < 10
 *     grad_theta[j] = sum_{k,i} gX[k,i] dX_dth[k,i,j] + sum_{k,c} gU[k,c] dU_dth[k,c,j],    j < 16
 * with dX_dp, dU_dp, dX_dth, dU_dth exactly the outputs of ltompc_get_sensitivities and ltompc_get_param_sensitivities (same
 * definition, same instances).  Block 0 of dX_dp is [I_8 | 0]: gX[0] lands in grad_p[0..7] as it is; block 0 of dX_dth is 0.
 *   ok[b] equals ltompc_get_sensitivities' ok[b] bit for bit; every output of an instance with ok[b] = 0 is exactly 0.
 * The KKT matrix is symmetric, so this is ONE more solve on the delta_w = 0 factorisation with the cotangent as right-hand
 * side (a backward and a forward recursion of vectors), contracted with the condensed right-hand sides of the 16 columns.
 *
 * Inputs, in the caller's instance order:
 *   gX  batch x (N+1) x 8;   gU  batch x N x 2.   Either may be NULL (= zeros); both NULL is a usage error.
 * Outputs, in the caller's instance order, any may be NULL:
 *   grad_p  batch x 10 (x0[0..7], u_prev[0..1]);   grad_theta  batch x 16;   ok  batch ints.
 *   grad_theta = NULL skips the parameter part of the pass (no right-hand sides are condensed, no forward recursion).
 * ltompc_get_adjoint: host pointers.  A non-finite cotangent is a usage error that names the instance.
 * ltompc_adjoint_dev: device pointers, enqueues only, on the handle's stream.  The cotangents are NOT checked.  The first
 *   request on a handle allocates the pass's buffers and synchronises once (as for ltompc_sensitivities_dev; the first one
 *   with grad_theta allocates the parameter part's the same way).
 *
 * The result refers to the last solve of each instance; before any solve and after set_initial_guess(_dev) a call is a usage
 * error.  grad_theta has the limits of ltompc_get_param_sensitivities: a handle with ell_penalty > 0 or ptv != 0, and a call
 * after rollout_dev, are usage errors; grad_p alone is available there.  With per-instance rows the gradients are those at the
 * rows the solve used.  The re-linearisation, the factorisation and the condensed right-hand sides are shared with the two
 * forward passes (whichever runs first for a solve makes them); nothing is kept per cotangent.  The pass writes buffers of its
 * own only: every later make_step, rollout or forward pass gives the bits it would have given without it. */
int ltompc_get_adjoint(ltompc_handle h, const double* gX, const double* gU, double* grad_p, double* grad_theta, int* ok);
int ltompc_adjoint_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_p_dev, double* grad_theta_dev,
                       int* ok_dev);

/* Adjoint gradients w.r.t. the track tables: the gradient of a scalar loss L(X, U) of the predicted trajectory of
 * the last solve w.r.t. the knot values y[r][j] of the LTOMPC_TABLE_VALUE_ROWS = 4 value rows r = kappa, n_left, n_right, v_ref
 * (the rows of ltompc_set_table_values; the grids s_kappa and s_arc are not differentiated), from the cotangents gX, gU of
 * ltompc_get_adjoint, summed over the instances of the handle (they share the tables):
 *     grad_tables[r][j] = sum_b ( sum_{k,i} gX_b[k,i] dX_b[k,i]/dy[r][j] + sum_{k,c} gU_b[k,c] dU_b[k,c]/dy[r][j] )
 * Definition: that of ltompc_get_sensitivities - the barrier problem at the final iterate with the final barrier parameter and
 * table smoothing, the KKT matrix with delta_w = 0, the same instances.  ok[b] equals ltompc_get_sensitivities' ok[b] bit for bit;
 * an instance with ok[b] = 0 contributes exactly 0.  Block 0 of gX does not enter (x0 is data).  Knots that no look-up of any
 * predicted trajectory touches get exactly 0.
 *
 * The tables enter interval k of instance b through ten scalars, the value and the slope that the look-ups returned:
 *     slot_grad[b][k][0..9] = dL/d( kappa(s(c_k)), kappa'(s(c_k)), kappa(s(x_{k+1})), kappa'(s(x_{k+1})),
 *                                   n_left, n_left', n_right, n_right', v_ref, v_ref' at s(x_{k+1}) )
 * (c_k: the first Radau point of interval k; the last six are 0 for k = N - 1: node N has no track row and no v_ref term).
 * slot_grad is deterministic: the same solve and cotangent give the same bits, whatever the batch, the packing or the split
 * over handles.  It is what a caller with a table parametrisation of its own (a spline race line) chains through.  grad_tables
 * is slot_grad scattered to the knots with the weights of the piece-wise linear basis (with the rounding of the knots that the
 * solve used: at most four knots per look-up) and summed over the instances with fp64 atomic adds: its last bits depend on
 * the order in which the adds arrive and can differ between two calls.  With periodic_tables the first and the last knot of a
 * row are reported separately.
 *
 * Inputs, in the caller's instance order:  gX  batch x (N+1) x 8;  gU  batch x N x 2.  Either may be NULL (= zeros); both NULL is a
 * usage error.  Outputs, any may be NULL:  grad_tables  4 x n_table (overwritten, not accumulated);  slot_grad  batch x N x 10 in the
 * caller's instance order;  ok  batch ints.
 * ltompc_get_adjoint_tables: host pointers.  A non-finite cotangent is a usage error that names the instance.
 * ltompc_adjoint_tables_dev: device pointers, enqueues only, on the handle's stream.  The cotangents are NOT checked.  The first
 *   request on a handle allocates the pass's buffers and synchronises once (as for ltompc_sensitivities_dev).
 *
 * The result refers to the last solve of each instance; before any solve, after set_initial_guess(_dev) and after
 * ltompc_set_table_values(_dev) a call is a usage error.  A handle with ell_penalty > 0 or ptv != 0 is a usage error, as for
 * ltompc_get_param_sensitivities; unlike grad_theta the pass needs no u_prev, so a call after rollout_dev works.  With
 * per-instance rows the gradients are those at the rows the solve used.  The re-linearisation and the factorisation are shared
 * with the other passes (whichever runs first for a solve makes them); nothing is kept per cotangent.  The pass writes buffers of
 * its own only: every later make_step, rollout or other pass gives the bits it would have given without it. */
int ltompc_get_adjoint_tables(ltompc_handle h, const double* gX, const double* gU, double* grad_tables, double* slot_grad, int* ok);
int ltompc_adjoint_tables_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_tables_dev, double* slot_grad_dev,
                              int* ok_dev);
/* ltompc_adjoint_tables_dev, except that grad_tables_dev is ADDED TO instead of overwritten (slot_grad_dev and ok_dev are written
 * as there): the handles of a batch that is split over several handles with the same tables call the plain form on the first
 * part and this one on the others, one after the other, and get the sum over the whole batch in one 4 x n_table array. */
int ltompc_adjoint_tables_add_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_tables_dev,
                                  double* slot_grad_dev, int* ok_dev);

/* ltompc_get_prediction into device memory: X_dev (row-major batch x (N+1) x 8) and U_dev (batch x N x 2) in the caller's
 * instance order, either may be NULL.  Enqueues only, on the handle's stream.  Unlike ltompc_get_prediction it reads the
 * instances where they are and does not restore the caller's order inside the handle: a device-side loop (a loss on the
 * prediction, ltompc_adjoint_dev, the next make_step_dev) never pays for un-packing. */
int ltompc_get_prediction_dev(ltompc_handle h, double* X_dev, double* U_dev);

/* Directional sensitivities of the last solve: the product of the Jacobians of the predicted trajectory with ONE
 * direction dp of p = (x0[0..7], u_prev[0..1]) and dtheta of theta (the LTOMPC_NTHETA = 16 columns above, natural units), without
 * forming a Jacobian.  For instance b:
 *     tX[k,i] = sum_{j < 10} dX_dp[k,i,j] dp[j] + sum_{j < 16} dX_dth[k,i,j] dtheta[j]
 *     tU[k,c] = sum_{j < 10} dU_dp[k,c,j] dp[j] + sum_{j < 16} dU_dth[k,c,j] dtheta[j]
 * with dX_dp, dU_dp, dX_dth, dU_dth exactly the outputs of ltompc_get_sensitivities and ltompc_get_param_sensitivities (same
 * definition, same instances).  Block 0 of tX is dp[0..7] as it is; block 0 of tU is du0_dp dp + du0_dth dtheta.
 *   ok[b] equals ltompc_get_sensitivities' ok[b] bit for bit; every output of an instance with ok[b] = 0 is exactly 0.
 * The linearised KKT system is linear in its right-hand side: with dtheta, ONE backward recursion of the dtheta-weighted sum of
 * the condensed right-hand sides of the 16 columns on the delta_w = 0 factorisation, then ONE forward recursion from (dp[0..7],
 * dp[8..9]); without dtheta only the forward recursion.
 *
 * Inputs, in the caller's instance order:
 *   dp  batch x 10 (x0[0..7], u_prev[0..1]);   dtheta  batch x 16.   Either may be NULL (= zeros); both NULL is a usage error.
 * Outputs, in the caller's instance order, any may be NULL:
 *   tX  batch x (N+1) x 8;   tU  batch x N x 2;   ok  batch ints.
 * ltompc_get_jvp: host pointers.  A non-finite direction is a usage error that names the instance.
 * ltompc_jvp_dev: device pointers, enqueues only, on the handle's stream.  The directions are NOT checked.  The first request
 *   on a handle allocates the pass's buffers and synchronises once (as for ltompc_sensitivities_dev; the first one with dtheta
 *   allocates the parameter part's the same way).
 *
 * The result refers to the last solve of each instance; before any solve and after set_initial_guess(_dev) a call is a usage
 * error.  dtheta != NULL has the limits of ltompc_get_param_sensitivities: a handle with ell_penalty > 0 or ptv != 0, and a call
 * after rollout_dev, are usage errors; dp alone is available there.  With per-instance rows the result is that at the rows the
 * solve used.  The re-linearisation, the factorisation and the condensed right-hand sides are shared with the other passes
 * (whichever runs first for a solve makes them); nothing is kept per direction.  The pass writes buffers of its own only: every
 * later make_step, rollout or other pass gives the bits it would have given without it. */
int ltompc_get_jvp(ltompc_handle h, const double* dp, const double* dtheta, double* tX, double* tU, int* ok);
int ltompc_jvp_dev(ltompc_handle h, const double* dp_dev, const double* dtheta_dev, double* tX_dev, double* tU_dev, int* ok_dev);

/* Directional sensitivities along a direction in the track tables: the forward twin of ltompc_get_adjoint_tables.
 * For a direction dy[r][j] in the knot values of the 4 value rows r = kappa, n_left, n_right, v_ref (the rows of
 * ltompc_set_table_values; the grids are not differentiated), for instance b:
 *     tX[k,i] = sum_{r,j} dX_b[k,i]/dy[r][j] dy[r][j] (+ sum_{j < 10} dX_dp[k,i,j] dp[j]),     tU[k,c] likewise
 * with dX/dy, dU/dy exactly the sensitivities whose transpose ltompc_get_adjoint_tables applies: the barrier problem at the final
 * iterate with the final barrier parameter and table smoothing, the KKT matrix with delta_w = 0, the same instances.  ok[b] equals
 * ltompc_get_sensitivities' ok[b] bit for bit; every output of an instance with ok[b] = 0 is exactly 0.  Block 0 of tX is dp[0..7]
 * when dp is given, else 0.  dtheta is not part of this call: the map is linear, a caller adds ltompc_jvp_dev's result.
 *
 * The direction has two forms, summed when both are given:
 *   dtables  4 x n_table: ONE direction of the handle, shared by all instances as the tables are.  The look-ups are linear in the
 *            knot values, so it reaches interval k as the ten tangents below with the weights of the piece-wise linear basis
 *            (with the rounding of the knots that the solve used: at most four knots per look-up).  With periodic_tables the
 *            first and the last knot of a row are read separately, as grad_tables reports them separately.
 *   dslot    batch x N x 10, in slot_grad's order: the tangents of what each look-up returned,
 *                d( kappa(s(c_k)), kappa'(s(c_k)), kappa(s(x_{k+1})), kappa'(s(x_{k+1})),
 *                   n_left, n_left', n_right, n_right', v_ref, v_ref' at s(x_{k+1}) )
 *            (the last six do not enter for k = N - 1).  The forward twin of slot_grad, for a caller that owns its table
 *            parametrisation (a spline race line) and pushes tangents through it itself.
 * The pass is a gather without atomic adds: the same solve and direction give the same bits, whatever the batch, the packing or
 * the split over handles.
 *
 * Inputs:  dp  batch x 10 (x0[0..7], u_prev[0..1]), dslot in the caller's instance order; dtables as above.  Any may be NULL
 * (= zeros); all three NULL is a usage error.  With dp alone the call is ltompc_get_jvp's without dtheta.
 * Outputs, in the caller's instance order, any may be NULL:  tX  batch x (N+1) x 8;   tU  batch x N x 2;   ok  batch ints.
 * ltompc_get_jvp_tables: host pointers.  A non-finite direction is a usage error that names the row and knot (dtables) or the
 *   instance (dp, dslot).
 * ltompc_jvp_tables_dev: device pointers, enqueues only, on the handle's stream.  The directions are NOT checked.  The first
 *   request on a handle allocates the pass's buffers and synchronises once (as for ltompc_sensitivities_dev).
 *
 * The result refers to the last solve of each instance (under a selected solve record: to the record's); before any solve, after
 * set_initial_guess(_dev) and between ltompc_set_table_values(_dev) / ltompc_set_table_sets and the next solve a call is a usage
 * error.  A handle with ell_penalty > 0 or ptv != 0 is a usage error, as for ltompc_get_adjoint_tables; the pass needs no u_prev,
 * so a call after rollout_dev works.  With per-instance rows the result is that at the rows the solve used.  The
 * re-linearisation and the factorisation are shared with the other passes (whichever runs first for a solve makes them);
 * nothing is kept per direction.  The pass writes buffers of its own only: every later make_step, rollout or other pass gives
 * the bits it would have given without it.
 *
 * On a handle with per-instance table sets (ltompc_set_table_sets) the two calls above are usage errors that name the two below,
 * and the other way round: there dtables is n_sets x 4 x n_table and instance b moves along block set_of_instance[b], on the
 * rows of its own set; a non-finite entry names the set too. */
int ltompc_get_jvp_tables(ltompc_handle h, const double* dp, const double* dtables, const double* dslot, double* tX, double* tU, int* ok);
int ltompc_jvp_tables_dev(ltompc_handle h, const double* dp_dev, const double* dtables_dev, const double* dslot_dev, double* tX_dev,
                          double* tU_dev, int* ok_dev);
int ltompc_get_jvp_table_sets(ltompc_handle h, const double* dp, const double* dtables, const double* dslot, double* tX, double* tU,
                              int* ok);
int ltompc_jvp_table_sets_dev(ltompc_handle h, const double* dp_dev, const double* dtables_dev, const double* dslot_dev, double* tX_dev,
                              double* tU_dev, int* ok_dev);

/* The previous input u_prev of the NEXT solve's Delta-u cost r_du (u_0 - u_prev)^2, which the handle otherwise makes itself (0
 * after set_initial_guess, else the u0 the last make_step returned): with it the solve is a function of (x0, u_prev, theta) that
 * a caller can evaluate.
 *   u_prev  batch x 2, in the caller's instance order.
 * ltompc_set_u_prev: host pointer.  Every row is checked finite; a bad row is a usage error that names the instance and leaves
 *   the handle unchanged.  ltompc_set_u_prev_dev: a device pointer, enqueues only, on the handle's stream.  NOT checked.
 * A set takes effect at the next make_step, make_step_dev or rollout_dev (there: the first solve of every instance) and holds
 * for that solve only.  Made after set_initial_guess(_dev) it wins over the cold start's zero; a set_initial_guess(_dev) after it
 * discards it.  It does not touch the warm start and does not invalidate the cached derivatives of the last solve, which keep
 * referring to the u_prev that solve used. */
int ltompc_set_u_prev(ltompc_handle h, const double* u_prev);
int ltompc_set_u_prev_dev(ltompc_handle h, const double* u_prev_dev);

/* Settable table values: overwrite one of the LTOMPC_TABLE_VALUE_ROWS = 4 value rows of the handle's look-up tables, so that a
 * caller who tunes the race line or the reference-speed profile keeps the handle and the warm start of its instances.
 *   row     0 kappa, 1 n_left, 2 n_right, 3 v_ref;   values  n_table doubles (the n_table of ltompc_create).
 * The grids s_kappa and s_arc, n_table and what ltompc_create derived from the grids (the interval estimate of the look-ups,
 * the period of options.periodic_tables) stay; they cannot be set.  With periodic_tables the caller keeps
 * values[n_table - 1] == values[0] (the kink at the seam is not rounded, as at ltompc_create); this is not checked.
 * ltompc_set_table_values: host pointer.  Every entry is checked finite; a bad entry is a usage error that names the knot and
 *   leaves the handle unchanged.  Returns when the row is in place.
 * ltompc_set_table_values_dev: a device pointer, enqueues only, on the handle's stream.  NOT checked.
 * ltompc_get_table_values: the row in effect (host, out), after everything enqueued on the handle's stream before it.
 * A set takes effect for everything enqueued after it: the next make_step, make_step_dev and rollout_dev solve with the new
 * row (bit for bit what a handle created with it gives from the same starting point), and ltompc_plant_step(_dev),
 * ltompc_plant_sensitivities(_dev) and the rollout's plant steps read the new kappa.  It does not touch the warm start (the
 * iterate, the multipliers, u_prev, the per-instance rows).  It discards the derivative state of the last solve - the cached
 * factorisation belongs to the old tables: until the next solve every derivative request (ltompc_get_sensitivities,
 * ltompc_get_param_sensitivities, ltompc_get_adjoint, ltompc_get_jvp, ltompc_loop_tick and their _dev forms) is the usage
 * error of a handle that has not solved yet. */
#define LTOMPC_TABLE_VALUE_ROWS 4
int ltompc_set_table_values(ltompc_handle h, int row, const double* values);
int ltompc_set_table_values_dev(ltompc_handle h, int row, const double* values_dev);
int ltompc_get_table_values(ltompc_handle h, int row, double* values);

/* Per-instance table sets.  A handle may hold n_sets >= 1 table sets - each the LTOMPC_TABLE_VALUE_ROWS value
 * rows (kappa, n_left, n_right, v_ref, n_table doubles each) on the handle's own two grids - and an index set_of_instance[batch]
 * in the caller's instance order.  Instance b's solve, plant step, rollout and supported derivative passes are then bit for bit
 * those of a handle created with the handle's tables, options and params and set set_of_instance[b] written into the value rows
 * (a twin in thread-per-slot evaluation mode, latency_mode = 2: handles with sets run the thread-per-slot evaluation kernels
 * whatever latency_mode says, as friction-ellipse handles do).  The grids, n_table, the period and the interval estimates stay
 * the handle's.  While sets are in effect no instance reads the handle's own value rows; ltompc_set_table_values keeps writing
 * them, and they take effect again once the sets are dropped.
 *
 * ltompc_set_table_sets: host pointers.  values is n_sets x 4 x n_table, set_of_instance is batch ints.
 *   values == NULL with n_sets unchanged changes the index only (the common move of a population method);
 *   set_of_instance == NULL keeps the index (all zeros before the first one; a usage error when it was written for more sets);
 *   n_sets == 0 goes back to the handle's tables (both pointers are ignored).
 *   A non-finite value is a usage error that names the set, an index outside [0, n_sets) one that names the instance; either
 *   leaves the handle unchanged.  A handle with ell_penalty > 0 or ptv != 0 and the debug path LTOMPC_RICCATI=serial refuse sets.
 * ltompc_set_table_sets_dev: the same from device arrays, enqueued on the handle's stream.  The values are NOT checked; the index
 *   is clamped into [0, n_sets) by the kernel that copies it, so no look-up can leave the value buffer.  The first set of either
 *   kind, and every set with more sets than the handle ever held, allocates and synchronises once.
 * ltompc_get_table_sets: n_sets in effect (0: none; then nothing else is written), and the values and the index in effect (host,
 *   out; either may be NULL), after everything enqueued on the handle's stream before it.
 *
 * Timing is ltompc_set_table_values' contract: a set takes effect from the next solve, plant step and rollout; the warm start is
 * kept (so are the per-instance rows); the derivative state of the last solve is discarded until the next solve.  One device
 * buffer each for the values and the index.  The warm-state blobs (ltompc_export_warm_state) do not carry the set index.
 *
 * With sets in effect these run: make_step(_dev), plant_step(_dev), rollout_dev, the prediction and iterate accessors,
 * ltompc_get_sensitivities / ltompc_sensitivities_dev, ltompc_get_adjoint(_dev) without grad_theta, ltompc_get_jvp(_dev) with dp
 * only, the per-set table gradient below, and the calls of the warm-start control.  These are usage errors: the derivatives
 * w.r.t. theta (ltompc_get_param_sensitivities, grad_theta, dtheta), ltompc_plant_sensitivities, the ltompc_loop_* calls and
 * the handle-wide ltompc_get_adjoint_tables / ltompc_adjoint_tables(_add)_dev (which point to the calls below).
 *
 * ltompc_get_adjoint_table_sets, ltompc_adjoint_table_sets_dev, ltompc_adjoint_table_sets_add_dev: ltompc_get_adjoint_tables and
 * its two _dev forms with grad_sets [n_sets][4][n_table] in place of grad_tables: block g is summed over the ok instances of
 * set g (a set without instances gets zeros).  slot_grad and ok are as there.  On a handle without sets they are a usage error
 * that points to the handle-wide calls. */
int ltompc_set_table_sets(ltompc_handle h, int n_sets, const double* values, const int* set_of_instance);
int ltompc_set_table_sets_dev(ltompc_handle h, int n_sets, const double* values_dev, const int* set_of_instance_dev);
int ltompc_get_table_sets(ltompc_handle h, int* n_sets, double* values, int* set_of_instance);
int ltompc_get_adjoint_table_sets(ltompc_handle h, const double* gX, const double* gU, double* grad_sets, double* slot_grad, int* ok);
int ltompc_adjoint_table_sets_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_sets_dev, double* slot_grad_dev,
                                  int* ok_dev);
int ltompc_adjoint_table_sets_add_dev(ltompc_handle h, const double* gX_dev, const double* gU_dev, double* grad_sets_dev,
                                      double* slot_grad_dev, int* ok_dev);

/* Per-instance vehicle and cost parameters.  Instance b may have its own row theta_b: the LTOMPC_NTHETA = 16
 * values of ltompc_get_param_sensitivities' columns, in that order and in natural units.  Every other field of ltompc_params
 * stays the handle's.  Instance b's NLP, plant step and sensitivities are then bit for bit those of a handle created with
 * theta_b written into its params (handles of the same latency mode).
 *
 * ltompc_set_instance_params: theta is batch x 16 (host, caller's instance order); NULL goes back to the handle's params.
 *   Every row is checked: all entries finite, mass > 0, inertia_z > 0, q_n, q_mu, q_B, r_du >= 0; a bad row is a usage error
 *   that names the row and the column and leaves the handle unchanged.  A handle with ell_penalty > 0 or ptv != 0 (those terms
 *   read the tyre and mass fields too) and the debug path LTOMPC_RICCATI=serial refuse rows with a usage error.
 * ltompc_set_instance_params_dev: the same from a device array (batch x 16), enqueued on the handle's stream.  NOT checked.
 *   The first set of either kind allocates two batch x 16 planes and synchronises once.
 * ltompc_get_instance_params: the rows in effect (batch x 16): the handle's values in every row when none are set.
 *
 * A set takes effect at the next make_step, make_step_dev, rollout_dev or plant_step(_dev) and does not touch the warm start.
 * The sensitivities (ltompc_get_sensitivities, ltompc_get_param_sensitivities) are those of the last solve, at the rows that
 * solve used, also when rows were set after it.  ltompc_plant_step(_dev) and the rollout's plant steps use the rows;
 * ltompc_slip_forces and the ltompc_test_* entry points always use the handle's params. */
int ltompc_set_instance_params(ltompc_handle h, const double* theta);
int ltompc_set_instance_params_dev(ltompc_handle h, const double* theta_dev);
int ltompc_get_instance_params(ltompc_handle h, double* theta);

/* Sensitivities of the plant step: the derivative of the discrete map that ltompc_plant_step computes - the
 * tangent of the same 4 x n_sub RK4 stage evaluations, the curvature table as the plant takes it (exact, slope of the current
 * interval) - at (x, u), with the rows in effect when per-instance rows are set (as ltompc_plant_step).
 *   x_next      batch x 8: the plant step itself, bit for bit ltompc_plant_step's;
 *   dxn_dx      batch x 8 x 8;     dxn_du  batch x 8 x 2;
 *   dxn_dtheta  batch x 8 x 16, the columns of ltompc_get_param_sensitivities in natural units: the 11 dynamics columns (rows
 *               vx, vy, r of the model), the five cost columns exactly 0.
 * Outputs may be NULL.  A handle with ptv != 0 refuses dxn_dtheta (usage error); dxn_dx and dxn_du are available there.
 * ltompc_plant_sensitivities: host pointers.  ltompc_plant_sensitivities_dev: device pointers, enqueues only, on the handle's
 * stream; the first request on a handle allocates the pass's buffers and synchronises once.  n_sub < 1 is a usage error. */
int ltompc_plant_sensitivities(ltompc_handle h, const double* x, const double* u, int n_sub, double* x_next, double* dxn_dx,
                               double* dxn_du, double* dxn_dtheta);
int ltompc_plant_sensitivities_dev(ltompc_handle h, const double* x_dev, const double* u_dev, int n_sub, double* x_next_dev,
                                   double* dxn_dx_dev, double* dxn_du_dev, double* dxn_dtheta_dev);

/* Closed-loop sensitivities: the derivative of where the loop  u0_t = make_step(x_t); x_{t+1} = plant(x_t, u0_t)
 * actually is after T ticks, w.r.t. q = (x_init[0..7], theta[0..15]): LTOMPC_NLOOP = 24 columns, theta in the order and units of
 * ltompc_get_param_sensitivities.  Per instance the handle keeps Sx = dx_t/dq (8 x 24) and Du = du_{t-1}/dq (2 x 24) on the device.
 *   ltompc_loop_begin(mode): Sx = [I_8 | 0], Du = 0, ok = 1, ticks = 0.  mode is a bit mask, 1 .. 3: bit 1 - theta enters the
 *     controller, bit 2 - theta enters the plant (1: tune the controller's model against a fixed car, 2: the car changes under a
 *     fixed controller, 3: both).  A handle with ell_penalty > 0 or ptv != 0 is a usage error (ltompc_get_param_sensitivities'
 *     limits).  The first call allocates the buffers and synchronises once; a handle that never asks pays nothing.
 *   ltompc_loop_tick_dev(x_dev, u0_dev, n_sub, x_next_dev): after make_step(_dev) at x_dev that returned u0_dev.  With K0, Kv0
 *     (ltompc_sensitivities_dev) and Tth (ltompc_param_sensitivities_dev) of that solve and Phi_x, Phi_u, Phi_th of the plant step
 *     at (x_t, u0_t):
 *         Du <- K0 Sx + Kv0 Du + [mode & 1] (Tth into the theta columns)
 *         Sx <- Phi_x Sx + Phi_u Du + [mode & 2] (Phi_th into the theta columns)
 *     and x_next_dev = the plant step (bit for bit ltompc_plant_step_dev's).  Enqueues only, on the handle's stream.  An instance
 *     whose solve has ok = 0 (ltompc_get_sensitivities') leaves the loop: its loop ok becomes 0, its Sx and Du are exactly 0 from
 *     that tick on, its tick counter stops; x_next is still the plant's.  Usage errors: no ltompc_loop_begin; no new make_step
 *     since the last tick; the last solve discarded by set_initial_guess or made by rollout_dev (it does not keep u_prev);
 *     n_sub < 1; a null argument.  The plant step uses the rows in effect (ltompc_plant_step's rule), the solve's derivatives the
 *     rows the solve used.
 *   ltompc_loop_tick: the same with host pointers (x, u0: in, x_next: out), synchronous.
 *   ltompc_get_loop_sensitivities: host outputs, any may be NULL: dx_dq batch x 8 x 24, du_dq batch x 2 x 24, ok and ticks batch ints
 *     (ticks: the ticks accumulated while ok).  ltompc_loop_sensitivities_dev: device pointers (dx_dq, du_dq, ok), enqueues only.
 *   ltompc_loop_end: ends the loop (a tick is a usage error until the next ltompc_loop_begin); the last values stay readable.
 * The passes write buffers of their own only: every later make_step, rollout, sensitivity or adjoint call gives the bits it would
 * have given without them. */
int ltompc_loop_begin(ltompc_handle h, int mode);
int ltompc_loop_tick_dev(ltompc_handle h, const double* x_dev, const double* u0_dev, int n_sub, double* x_next_dev);
int ltompc_loop_tick(ltompc_handle h, const double* x, const double* u0, int n_sub, double* x_next);
int ltompc_get_loop_sensitivities(ltompc_handle h, double* dx_dq, double* du_dq, int* ok, int* ticks);
int ltompc_loop_sensitivities_dev(ltompc_handle h, double* dx_dq_dev, double* du_dq_dev, int* ok_dev);
int ltompc_loop_end(ltompc_handle h);

/* ---------------------------------------------------------------------------------------------------------------------
 * Per-instance control of the warm start.  A handle carries a warm start per instance from solve to solve;
 * ltompc_set_initial_guess throws away that of the whole batch.  The calls below act on chosen instances: every other
 * instance keeps its warm start to the bit, and a handle on which none of them is made runs exactly as before.
 * Instance indices, masks and rows are in the CALLER's order whatever order the handle keeps its instances in.
 * Every call has a host form (host pointers, checked, returns when done; a usage error leaves the handle unchanged) and a
 * _dev form (device pointers, enqueues only, on the handle's stream, NOT checked).
 * A call that changes an instance discards the cached derivatives of the last solve (as ltompc_set_initial_guess: a derivative
 * request before the next solve is a usage error).  Between ltompc_loop_begin and ltompc_loop_end the changing calls
 * (reset_instances, set_guess, import_state) are usage errors: the loop's chain of an instance would be broken.
 *
 * ltompc_reset_instances: a cold start of the instances b with mask[b] != 0, from x0[b] (mask: batch ints, x0: batch x 8; rows
 *   with mask 0 are ignored, also by the checks).  The iterate of a reset instance is filled as ltompc_set_initial_guess fills
 *   it (ltompc_get_iterate shows it), its u_prev becomes 0, its previous status, node-0 flag and sticky / restoration counters
 *   are cleared, and its next solve (make_step, make_step_dev, or its first one in rollout_dev) is a cold solve, bit for bit the
 *   first solve of a fresh handle.  A ltompc_set_u_prev after the reset overrides the zero for that solve; one before it is
 *   zeroed for the reset instances.  With options.warm_shift a reset instance is simply cold.  An all-ones mask is
 *   ltompc_set_initial_guess; an all-zeros mask changes nothing.
 *
 * ltompc_set_guess: a primal starting point for the instances with mask[b] != 0, in the layouts of ltompc_get_iterate:
 *   X batch x (N+1) x 8, C batch x N x 8 (the collocation states; e.g. x_k + (x_{k+1} - x_k) / 3, the Radau point at tau = 1/3),
 *   U batch x N x 2, u_prev batch x 2 or NULL (= 0).  The guess stands in for a previous solution that did not converge:
 *   planes := guess, L1 = L2 = 0, previous status := LTOMPC_STATUS_MAX_ITER, node-0 flag and sticky counters cleared, NOT
 *   cold.  Everything else is what the start of a solve does after a failed one: node 0 := the measured x0, barrier at mu_init
 *   (options.warm_reset_on_fail), slacks from the point; every warm-start option applies to the guess as to a previous solution.
 *   The host form refuses non-finite entries in the rows it uses.
 *
 * ltompc_warm_state_size: doubles per instance of a blob row (34 N + 18).
 * ltompc_export_state / ltompc_import_state: blob is n x size doubles, row j = instance idx[j] (idx NULL: instance j, n <= batch).
 *   A row holds everything the instance's next solve depends on: a header word (magic, layout version, N), the previous
 *   status, node-0 flag, restoration / sticky counters and the pending-cold flag, u_prev, and the planes X, C, U, L1, L2.
 *   NOT part of it: per-instance parameter rows (ltompc_set_instance_params) and the tables, which the caller sets on the
 *   target as on the source.  A blob is valid between handles of equal N, options and library build (only N and the layout
 *   version are checked).  After an import the iterate and prediction accessors show the imported point (T and NU of
 *   ltompc_get_ineq are rebuilt by the next solve); ltompc_get_stats shows the imported status; the other per-solve statistics
 *   (iters, kkt_error, counters, restoration, recovery) stay what they were until the next solve.
 *   Host-form usage errors: an index out of range, an index twice in an import, a wrong header, a non-finite payload (the
 *   planes of a row that starts cold are not looked at).  Export changes nothing and is allowed inside an open loop.
 * Returns 0 (ltompc_warm_state_size: the size), or < 0 with ltompc_last_error(). */
int ltompc_reset_instances(ltompc_handle h, const int* mask, const double* x0);
int ltompc_reset_instances_dev(ltompc_handle h, const int* mask_dev, const double* x0_dev);
int ltompc_set_guess(ltompc_handle h, const int* mask, const double* X, const double* C, const double* U, const double* u_prev);
int ltompc_set_guess_dev(ltompc_handle h, const int* mask_dev, const double* X_dev, const double* C_dev, const double* U_dev,
                         const double* u_prev_dev);
int ltompc_warm_state_size(ltompc_handle h);
int ltompc_export_state(ltompc_handle h, const int* idx, int n, double* blob);
int ltompc_export_state_dev(ltompc_handle h, const int* idx_dev, int n, double* blob_dev);
int ltompc_import_state(ltompc_handle h, const int* idx, int n, const double* blob);
int ltompc_import_state_dev(ltompc_handle h, const int* idx_dev, int n, const double* blob_dev);

/* Solve records: differentiate any earlier solve of a handle.  The derivative passes (ltompc_get_sensitivities,
 * ltompc_get_param_sensitivities, ltompc_get_adjoint, ltompc_get_adjoint_tables, ltompc_get_jvp and their _dev / _add_dev forms)
 * read the handle's last solve in place, so the next solve, guess, reset, import or table set takes it away.  A record is a
 * device copy of everything those passes read of one solve (about 83 N + 50 doubles per instance), in the caller's instance
 * order; while one is selected the passes run on it instead of the live solve, on the same kernels.
 *   ltompc_record_size     device bytes of one record of this handle.
 *   ltompc_record_save     captures the solve the live passes would refer to now.  *rec == NULL: a record from the handle's free
 *                          list, else a new one (allocates and synchronises once); *rec != NULL: that record is overwritten.  Reuse
 *                          and overwrite only enqueue one gather kernel and two copies on the handle's stream.  Read-only on the
 *                          handle, allowed inside an open loop.  Fails when there is no solve to differentiate, and on a handle
 *                          with per-instance table sets in effect (records of such solves are out of scope).
 *   ltompc_record_select   rec: the passes run on it from now on; NULL: back to the live solve.  A change of selection drops the
 *                          cached factorisation and results: the first pass after it re-linearises and re-factorises (about one
 *                          iteration).  Everything else - solves, plant steps, rollouts, setters, reset / import, the accessors of
 *                          the iterate and the statistics - keeps working on the live handle and touches neither record nor
 *                          selection.  Refused inside an open loop; ltompc_loop_begin / ltompc_loop_tick are refused while a record
 *                          is selected.  A pass the recorded solve itself could not run (theta passes after a rollout, ...) is
 *                          refused with the message of the live call.
 *   ltompc_record_release  back to the handle's free list (deselects it first when selected).  Never frees device memory.
 *   ltompc_record_trim     frees the records of the free list (synchronises).
 *   ltompc_record_stats    records in use and on the free list; either output may be NULL.
 * Whatever happens on the handle between save and select, a pass on a record returns the bits it would have returned right after
 * the recorded solve (grad_tables: up to the order of its atomic adds, as on the live solve).  A record of another handle, a
 * released or trimmed one is refused.  ltompc_destroy frees every record of the handle.
 * Return 0 (ltompc_record_size: the size), or < 0 with ltompc_last_error(). */
typedef struct ltompc_record_s* ltompc_record;
long long ltompc_record_size(ltompc_handle h);
int ltompc_record_save(ltompc_handle h, ltompc_record* rec);
int ltompc_record_select(ltompc_handle h, ltompc_record rec);
int ltompc_record_release(ltompc_handle h, ltompc_record rec);
int ltompc_record_trim(ltompc_handle h);
int ltompc_record_stats(ltompc_handle h, int* in_use, int* free_);

/* The feedback policy of the last solve: the time-varying local law of the whole horizon, to close the loop
 * between solves.  With X, U the prediction of that solve, V_0 the u_prev it used and V_k = U_{k-1}, for instance b
 *     pi_k(x, v) = U_k + K_k (x - X_k) + Kv_k (v - V_k),      k = 0 .. N-1.
 * K_k (2 x 8) and Kv_k (2 x 2) are the stage gains of the delta_w = 0 Riccati factorisation at the final iterate, the words the
 * forward pass of ltompc_get_sensitivities propagates (dU_k = K_k dX_k + Kv_k dV_k): K_k is the derivative of the first control
 * of the BARRIER problem of the tail (nodes k .. N) w.r.t. its initial state, Kv_k w.r.t. its previous input.  K_0 = du0/dx0 and
 * Kv_0 = du0/du_prev bit for bit.  They are not the gains of a solve started at node k with a new barrier parameter or warm start.
 *   ok[b] equals ltompc_get_sensitivities' ok[b] bit for bit.  Where ok[b] = 0, K and Kv are exactly 0 and pi_k = U_k - not NaN:
 *   a caller that applies the policy blindly gets the open-loop plan.
 *   clip = 1 saturates the result; delta and T (states 6, 7) integrate the inputs exactly over one t_step under a held input, so
 *   for i = 0, 1 first u_i <- min(max(u_i, (x_lb[6+i] - x[6+i]) / t_step), (x_ub[6+i] - x[6+i]) / t_step), then
 *   u_i <- min(max(u_i, u_lb[i]), u_ub[i]) (the input bounds win); a bound at LTOMPC_NO_BOUND is skipped.  clip = 0: the formula.
 *
 * All arrays are row-major in the caller's instance order.
 * ltompc_get_policy: host outputs, any may be NULL:  K  batch x N x 2 x 8;   Kv  batch x N x 2 x 2;   ok  batch ints.
 * ltompc_policy_dev: the same into device arrays, any may be NULL.  Enqueues only, on the handle's stream.
 * ltompc_policy_step: u (batch x 2) = pi_k(x, v) for host arrays x (batch x 8) and v (batch x 2; NULL means V_k: no correction
 *   in that direction).  A non-finite x or v is a usage error that names the instance.
 * ltompc_policy_step_dev: device pointers, enqueues only.  x and v are NOT checked.  It reads the prediction and the gains where
 *   they are: no gather first, and the instances stay where the solve left them.
 * ltompc_policy_run_dev: n ticks of the loop in ONE launch, for j = 0 .. n-1:
 *       u_j = pi_{k0+j}(x, v);   x <- plant(x, u_j, t_step, n_sub);   v <- u_j,
 *   the plant step that of ltompc_plant_step_dev bit for bit (the handle's tables, per-instance rows and table sets in effect -
 *   also while a record is selected).  x_dev (batch x 8) holds the states, in and out; v_dev (batch x 2) the input before tick 0
 *   or NULL (V_k0);  u_log_dev (batch x n x 2) the controls and x_log_dev (batch x n x 8) the state AFTER each tick, either may
 *   be NULL.  Enqueues only.  With n = 1, u_log_dev may be v_dev itself (an instance's row is read before it is written).
 * ltompc_policy_last_dev: the controls of the last tick of such a log (batch x n x 2) as an array u_dev (batch x 2) - what
 *   ltompc_set_u_prev_dev and ltompc_plant_step_dev take.  One strided device copy, enqueued on the handle's stream.
 * Exception: the first request on a handle (any of the five) allocates the pass's workspaces and synchronises the handle's stream
 *   once (as for ltompc_sensitivities_dev, whose workspaces they are); the first host form also its staging.
 *
 * The result refers to the last solve of each instance, or to the selected record, exactly like ltompc_get_sensitivities; the
 * re-linearisation and the factorisation are shared with the other passes (whichever runs first for a solve makes them).  Usage
 * errors, which leave the handle unchanged: a call before any solve or after set_initial_guess(_dev); k (k0) outside [0, N);
 * n < 1; k0 + n > N; n_sub < 1; policy_step / policy_run after rollout_dev (it does not keep the u_prev of each instance's last
 * solve, V_0) - the gains alone stay available there, like the sensitivities.  Handles with ell_penalty > 0 or ptv != 0 are
 * accepted.  The calls write buffers of their own and the caller's arrays only: every later make_step, rollout or pass gives the
 * bits it would have given without them. */
int ltompc_get_policy(ltompc_handle h, double* K, double* Kv, int* ok);
int ltompc_policy_dev(ltompc_handle h, double* K_dev, double* Kv_dev, int* ok_dev);
int ltompc_policy_step(ltompc_handle h, int k, const double* x, const double* v, int clip, double* u);
int ltompc_policy_step_dev(ltompc_handle h, int k, const double* x_dev, const double* v_dev, int clip, double* u_dev);
int ltompc_policy_run_dev(ltompc_handle h, int k0, int n, double* x_dev, const double* v_dev, int n_sub, int clip, double* u_log_dev,
                          double* x_log_dev);
int ltompc_policy_last_dev(ltompc_handle h, int n, const double* u_log_dev, double* u_dev);

/* Profiling: when on, every kernel launch of make_step is bracketed by HIP events on the handle's stream and
 * ltompc_get_timing returns the accumulated device time per kernel class since profiling was switched on:
 * index 0 eval (k_eval or k_eval8), 1 riccati (8 instances per wavefront), 2 expand (k_expand or k_expand8), 3 linesearch,
 * 4 pick, 5 update, 6 riccati1 (the one-instance-per-workgroup sweeps of the narrow launches: k_riccati1, one wavefront, and k_riccati1q, four), 7 step1 (their fused
 * line-search / pick / update kernel).  launches / ip_iterations (iterations launched) refer to the last make_step.
 * Arrays have 8 entries.  Any output may be NULL.
 * on = 0 off, 1 every launch, 2 + c: only the launches of kernel class c (two events per iteration instead of seven:
 * at 120 k solves/s bracketing every launch costs 4 % of the throughput, bracketing one class 1 %). */
int ltompc_set_profiling(ltompc_handle h, int on);
int ltompc_get_timing(ltompc_handle h, double* ms_by_kernel8, int* launches_by_kernel8, int* launches,
                      int* ip_iterations);
/* Per-launch log of the profiled make_steps since profiling was switched on: kernel class (index as above), launch
 * width (instances the launch was sized for: the whole batch until the first re-packing of the unfinished instances)
 * and device time in ms.  Returns the number of log entries (copies at most `capacity`); negative on error. */
int ltompc_get_launch_log(ltompc_handle h, int* kind, int* width, double* ms, int capacity);

/* Interior-point iteration (0-based, within its make_step) of every entry of the launch log; returns the number of entries. */
int ltompc_get_launch_log_iterations(ltompc_handle h, int* iteration, int capacity);

/* Number of unfinished instances after every iteration of the last make_step (entry i: instances that passed the
 * termination test of iteration i and went on); returns the number of iterations launched (0 after a rollout, which keeps
 * no per-iteration counts). */
int ltompc_get_active_history(ltompc_handle h, int* active, int capacity);

/* Histogram of the per-instance statuses of the last solve (counts8[s], s = LTOMPC_STATUS_*; entry 7 collects anything
 * else) and the sum of the instances' iteration counts, reduced on the device: cheaper than ltompc_get_stats and does
 * not disturb the packed order of the instances.  Either output may be NULL. */
int ltompc_get_status_counts(ltompc_handle h, int* counts8, long long* iterations_sum);
/* ... and the histogram of the solver's own statuses (before the node-0 rule of options.node0_check) that the last
 * ltompc_get_status_counts call reduced along with it. */
int ltompc_get_solver_status_counts(ltompc_handle h, int* counts8);

/* Poll history of the last make_step: up to `capacity` triples (iteration, unfinished instances, launch width);
 * returns the number of polls (>= 0). */
int ltompc_get_history(ltompc_handle h, int* triples, int capacity);

/* make_step polls the device's count of unfinished instances every n interior-point iterations (default 4). */
int ltompc_set_poll_every(ltompc_handle h, int n);

/* Launches of at most `width` unfinished instances use the one-instance-per-workgroup kernels (k_riccati1 / k_riccati1q,
 * k_step1), wider ones the full-width kernels; default 512, 0 = never, at most 512.  Scheduling only: an instance's result does
 * not depend on it (tests/test_gpu_parity.py).  With several handles ticking beside each other on one GPU a lower switch-over
 * is faster (their one-instance workgroups queue for the same CUs): four handles of 2048, 128 instead of 512: +2 %. */
int ltompc_set_narrow_width(ltompc_handle h, int width);

/* Debug hook: raw copy of a device work array in its device layout (see csrc/kernels.h); returns its size in bytes.
 * Work arrays are indexed by the physical slot of an instance; a solve that re-packed its unfinished instances
 * (more than 4 iterations) uses the step buffers as temporaries when it restores the caller's order,
 * so their content is meaningful after solves capped at a few iterations only (which is what the tests do). */
long long ltompc_debug_fetch(ltompc_handle h, int which, void* out, long long nbytes);

/* Test hook (not part of the reference surface): model derivatives at n points, computed by the same device
 * functions the solver kernels use.  x, lam: n x 8 -> f: n x 8; J (df/dx), H (sum_i lam_i d2f_i): n x 8 x 8;
 * cost value / gradient / Hessian of lterm and mterm: n x 2 [x 8 [x 8]]; constraints gL, gR+, gR-:
 * n x 3 [x 8 [x 8]].  eps = table smoothing length. */
int ltompc_test_model(ltompc_handle h, int n, double eps, const double* x, const double* lam, double* f,
                      double* J, double* H, double* cval, double* cgrad, double* cH, double* gval,
                      double* ggrad, double* gH);

/* Test hook: the five table look-ups of a horizon slot at n arc lengths: kappa at s[t]; kappa, v_ref, n_left, n_right at
 * s[n - 1 - t]; value, slope and second derivative each (n x 5 x 3).  `direct`: one look-up after the other, as the plant and the
 * derivative passes do; `batched`: fetched in one batch and finished afterwards, as the evaluation kernels do.  Equal bit for bit. */
int ltompc_test_lut(ltompc_handle h, int n, double eps, const double* s, double* direct, double* batched);

/* Test hook: the friction-ellipse constraints (front, rear; params.ell_*) at n points: val n x 2, grad n x 2 x 8, H n x 2 x 8 x 8. */
int ltompc_test_ellipse(ltompc_handle h, int n, const double* x, double* val, double* grad, double* H);

/* ---------------------------------------------------------------------------------------------------------------------
 * Velocity-profile generator: the producer of velocities.json, the v_ref table of the hot path.
 * Replaces VelocityProfile(vehicle, s, k, s_max) of the reference (src/velocity.py:14-76, called from
 * src/trajectory.py:47-52): local limit sqrt(mu g / k), forward pass limited by engine force and remaining traction,
 * backward pass limited by the remaining traction, v = min of the two; a batch of independent profiles per call (the
 * race-line optimisers evaluate one profile per candidate line).  One GPU thread per profile (the passes are sequential
 * scans over the samples). */
typedef struct ltompc_vp_vehicle {
  int kind;                     /* 0: engine map + friction circle (src/vehicle.py:11-35), 1: MX-5 (src/vehicleMX5.py:11-79) */
  int n_map;                    /* kind 0: points of the engine map (<= 16) */
  double mass, friction_coef;   /* friction_coef: `frictionCoefficient` / `control.lambda` (local limit; kind 0: traction too) */
  double lam, D;                /* kind 1: traction(v, k, lam=2.0): F_max = lam * D * mass * g with D = (D_f + D_r) / 2 */
  double T, C_m, Cr_0, Cr_2;    /* kind 1: engine_force(v) = T C_m - Cr_0 - Cr_2 v^2 */
  double map_v[16], map_f[16];  /* kind 0: engine_force(v) = np.interp(v, map_v, map_f) */
} ltompc_vp_vehicle;

/* s, k: batch x n (arc length and curvature > 0 of the samples, WITHOUT the overlapping end point of a closed path);
 * s_max: batch (length of the closed path; < 0: open path, `s_max=None` in the reference).  Outputs batch x n, host
 * pointers, any of v_local / v_acclim / v_declim may be NULL.  Returns 0, or < 0 with ltompc_last_error(). */
int ltompc_velocity_profile(int device, const ltompc_vp_vehicle* vehicle, int n, int batch, const double* s, const double* k,
                            const double* s_max, double* v, double* v_local, double* v_acclim, double* v_declim);

#ifdef __cplusplus
}
#endif
#endif /* LTOMPC_H */
