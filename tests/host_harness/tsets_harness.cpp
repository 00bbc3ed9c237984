// tsets_harness.cpp — TEST INFRASTRUCTURE: the kernels of the per-instance table sets (the _ts family) compiled as
// host C++ and run under AddressSanitizer + UndefinedBehaviorSanitizer: whole interior-point solves with the launch sequence of
// ltompc_make_step_dev (k_init_ts, k_eval_ts, k_riccati8_ts, k_expand_ts, k_linesearch_ts, k_pick_ts, k_update), the plant step
// k_plant_ts between two ticks, then the per-set table-gradient pass (k_sens_eval_ts, the head-less sweep, k_adj_sweep_tab_pi,
// k_tab_cond_ts, k_tab_scatter_ts).  The thread-per-slot kernels run lane after lane, the wave kernels on the lock-step
// wavefront of hip_shim.h.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
//   tsets_harness <problem file>
// The instances sit in permuted slots (orig is not the identity for B > 1) from the first launch on; every work buffer has exactly
// the size the kernels may touch and is NaN-filled; the set values are one buffer of exactly n_sets x 4 x n_table doubles and the
// index one of exactly B ints (the library pads it to Bp: no kernel may read a pad); the handle's own four value rows are NaN
// (with sets in effect no instance reads them).
// Problem file (text): `n_table N B n_sets ticks`, the tables (6 x n_table), the sets (n_sets x 4 x n_table), the index (B), x0
// (B x 8), gX (B x (N+1) x 8), gU (B x N x 2).  Output per tick: `tick t`, per instance `r status iters u0 u1`, then `x` and the
// next states (B x 8); after the last tick `ok`, the s coordinates of c_k and x_{k+1} (B x N each), eps (B), slot_grad, grad_sets.
// tests/test_host_harness_table_sets.py compares with the oracle per set.  Nothing in the package uses this file.
#include "layout.h"

inline double atomicAdd(double* p, double v) {  // (one thread at a time here; hip_shim.h's atomicAdd is for integers)
  const double old = *p;
  *p = old + v;
  return old;
}

#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"
#include "eval8.h"
#include "sensitivity.h"
#include "table_sensitivity.h"

#include <cstdio>
#include <type_traits>
#include <vector>

using namespace ltompc;

static double* poisoned(size_t n) {
  double* p = (double*)malloc((n ? n : 1) * sizeof(double));
  memset(p, 0xFF, (n ? n : 1) * sizeof(double));
  return p;
}
static double* zeros(size_t n) { return (double*)calloc(n ? n : 1, sizeof(double)); }
static int* ints(size_t n, int fill) {
  int* p = (int*)malloc((n ? n : 1) * sizeof(int));
  for (size_t i = 0; i < n; i++) p[i] = fill;
  return p;
}
static void default_params(ltompc_params* p) {  // = ltompc_default_params (ltompc.hip)
  memset(p, 0, sizeof *p);
  p->mass = 1000.0, p->inertia_z = 1000.0, p->length_f = 1.5, p->length_r = 1.5, p->width = 2.3;
  p->B_f = 10.0, p->C_f = 1.3, p->D_f = 1.0, p->B_r = 12.0, p->C_r = 1.2, p->D_r = 1.0;
  p->C_m = 1000.0, p->Cr_0 = 0.01, p->Cr_2 = 0.0003, p->gravity = 9.81;
  p->q_n = 0.5, p->q_mu = 3.0, p->q_vy = 1.0, p->q_v = 1.0, p->vref_scale = 0.6, p->q_B = 1e-2;
  p->r_du[0] = p->r_du[1] = 1e-2;
  for (int i = 0; i < NX; i++) p->x_lb[i] = -LTOMPC_NO_BOUND, p->x_ub[i] = LTOMPC_NO_BOUND;
  const double pi = 3.14159265358979323846;
  p->x_lb[0] = 0.0, p->x_lb[2] = -pi * 0.5, p->x_ub[2] = pi * 0.5, p->x_lb[3] = 0.0;
  p->x_lb[6] = -pi / 4, p->x_ub[6] = pi / 4, p->x_lb[7] = -1.0, p->x_ub[7] = 1.0;
  p->u_lb[0] = -2 * pi / 4, p->u_ub[0] = 2 * pi / 4, p->u_lb[1] = -1.0, p->u_ub[1] = 1.0;
}
static void default_options(ltompc_options* o) {  // = ltompc_default_options
  memset(o, 0, sizeof *o);
  o->t_step = 0.1, o->tol = 1e-8, o->acceptable_tol = 1e-6, o->mu_init = 0.1, o->mu_min = 1e-9;
  o->kappa_eps = 10, o->kappa_mu = 0.2, o->theta_mu = 1.5, o->tau_min = 0.99, o->bound_push = 1e-2;
  o->s_max = 100, o->delta_w_first = 1e-4, o->smooth_eps_min = 1e-4, o->smooth_scale = 1.0;
  o->max_iter = 1000, o->acceptable_iter = 15, o->n_linesearch = 8, o->stall_iter = 15, o->max_ls_fail = 8;
  o->warm_reset_on_fail = 1, o->resto_rho = 1000.0;
  o->resto_rho_max = 1e6, o->resto_rho_factor = 1e3, o->dual_inf_max = 1e4, o->max_mu_stay = 100, o->infeasible_sticky = 1, o->node0_check = 1,
  o->warm_fallback_iter = 25, o->resto_shift_retry = 1;
}
static void build_bounds(const ltompc_params& p, Bounds& b) {  // = build_bounds (ltompc.hip), no friction ellipse
  memset(&b, 0, sizeof b);
  for (int i = 0; i < NX; i++) {
    if (p.x_lb[i] > -LTOMPC_NO_BOUND) b.xb_idx[b.n_xb] = i, b.xb_sgn[b.n_xb] = -1.0, b.xb_val[b.n_xb] = p.x_lb[i], b.n_xb++;
    if (p.x_ub[i] < LTOMPC_NO_BOUND) b.xb_idx[b.n_xb] = i, b.xb_sgn[b.n_xb] = +1.0, b.xb_val[b.n_xb] = p.x_ub[i], b.n_xb++;
  }
  for (int i = 0; i < NU; i++) {
    if (p.u_lb[i] > -LTOMPC_NO_BOUND) b.ub_idx[b.n_ub] = i, b.ub_sgn[b.n_ub] = -1.0, b.ub_val[b.n_ub] = p.u_lb[i], b.n_ub++;
    if (p.u_ub[i] < LTOMPC_NO_BOUND) b.ub_idx[b.n_ub] = i, b.ub_sgn[b.n_ub] = +1.0, b.ub_val[b.n_ub] = p.u_ub[i], b.n_ub++;
  }
  b.nel = 0;
  b.ni = b.n_ub + 2 * b.n_xb + NNL;
}
template <typename F>
static void grid_bs(size_t threads, unsigned bs, F&& body) {  // a thread-per-element kernel, lane after lane
  blockDim.x = bs, gridDim.x = (unsigned)((threads + bs - 1) / bs);
  for (unsigned blk = 0; blk < gridDim.x; blk++)
    for (unsigned t = 0; t < bs; t++) blockIdx.x = blk, threadIdx.x = t, body();
  blockDim.x = 64;
}
template <typename F>
static void wave64(const char* name, int blocks, F&& body) {  // a wave kernel on the lock-step wavefront, block after block
  blockDim.x = 64, gridDim.x = blocks;
  for (int blk = 0; blk < blocks; blk++) {
    blockIdx.x = blk;
    LtWave::self().run(name, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, &body);
  }
}
static bool read(FILE* f, double* dst, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (fscanf(f, "%lf", dst + i) != 1) return false;
  return true;
}
static void put(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%.17g%c", v[i], i + 1 == n ? '\n' : ' ');
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: tsets_harness <problem file>\n"), 2;
  FILE* f = fopen(argv[1], "r");
  int n_table, N, B, n_sets, ticks;
  if (!f || fscanf(f, "%d %d %d %d %d", &n_table, &N, &B, &n_sets, &ticks) != 5) return fprintf(stderr, "bad problem file\n"), 2;
  const int Bp = (B + 63) / 64 * 64;
  const size_t n = N, bp = Bp, nt = n_table;
  Consts K{};
  default_params(&K.p), default_options(&K.o);
  build_bounds(K.p, K.bd);
  const int ni = K.bd.ni;
  // ---- the handle's tables: the two grids; its own value rows are NaN at their exact size (no instance may read them)
  std::vector<double> tab(6 * nt), x((size_t)8 * B), gX((n + 1) * 8 * B), gU(n * 2 * B), idx_in(B);
  double* const sets = poisoned((size_t)n_sets * LTOMPC_TABLE_VALUE_ROWS * nt);
  bool good = read(f, tab.data(), tab.size()) && read(f, sets, (size_t)n_sets * LTOMPC_TABLE_VALUE_ROWS * nt) && read(f, idx_in.data(), B) &&
              read(f, x.data(), x.size()) && read(f, gX.data(), gX.size()) && read(f, gU.data(), gU.size());
  fclose(f);
  if (!good) return fprintf(stderr, "short problem file\n"), 2;
  double* rows[6];
  for (int r = 0; r < 6; r++) {
    rows[r] = poisoned(nt);
    if (r == 0 || r == 2) memcpy(rows[r], tab.data() + r * nt, sizeof(double) * nt);
  }
  Tables& T = K.T;
  T.n = n_table, T.s_kappa = rows[0], T.kappa = rows[1], T.s_arc = rows[2], T.n_left = rows[3], T.n_right = rows[4], T.v_ref = rows[5];
  T.g0_kappa = rows[0][0], T.inv_kappa = (double)(n_table - 1) / (rows[0][nt - 1] - rows[0][0]);
  T.g0_arc = rows[2][0], T.inv_arc = (double)(n_table - 1) / (rows[2][nt - 1] - rows[2][0]);
  T.period = 0.0;
  int* const tsi = ints(B, 0);  // exactly B entries, in the caller's order
  for (int b = 0; b < B; b++) tsi[b] = (int)idx_in[b];
  // ---- slot b holds the caller's instance orig[b]: a permutation that is not the identity (B > 1)
  int* const orig = ints(B, 0);
  {
    auto gcd = [](int a, int c) { while (c) { const int t = a % c; a = c, c = t; } return a; };
    int step = 2;
    while (gcd(step, B) != 1) step++;
    for (int b = 0; b < B; b++) orig[b] = (int)(((long long)step * b + B / 2) % B);
  }
  // ---- the solver's Work at exact sizes, NaN-filled (ltompc_create), TH = the handle's own params in every column
  WorkTS W{};
  W.N = N, W.B = B, W.Bp = Bp;
  W.X = poisoned(8 * (n + 1) * bp), W.C = poisoned(8 * n * bp), W.U = poisoned(2 * n * bp), W.L1 = poisoned(8 * n * bp), W.L2 = poisoned(8 * n * bp);
  W.T = poisoned((ni + NNL) * n * bp), W.NU = poisoned(ni * n * bp);
  W.dX = poisoned(8 * (n + 1) * bp), W.dC = poisoned(8 * n * bp), W.dU = poisoned(2 * n * bp), W.nL1 = poisoned(8 * n * bp), W.nL2 = poisoned(8 * n * bp);
  W.dT = poisoned((ni + NNL) * n * bp), W.dNU = poisoned(ni * n * bp);
  W.QP = poisoned((size_t)QP_NF * (n + 1) * bp), W.RC = poisoned((size_t)RC_NF * (n + 1) * bp);
  W.RS = poisoned((size_t)RS_NF * n * bp), W.SP = poisoned((size_t)SP_NF * n * bp), W.LS = poisoned((size_t)3 * (K.o.n_linesearch + 1) * n * bp);
  W.x0 = poisoned(8 * bp), W.uprev = poisoned(2 * bp), W.st = poisoned((size_t)ST_NF * bp), W.filt = poisoned((size_t)2 * FILTER_MAX * bp);
  W.si = ints((size_t)SI_NF * bp, 0), W.active = ints(K.o.max_iter + 2, 0), W.ls_list = ints(bp, -1), W.ls_count = ints(4, 0);
  W.BK = poisoned(18 * n * bp);
  W.orig = orig;
  double* const TH = poisoned((size_t)LTOMPC_NTHETA * bp);
  {
    const ltompc_params& p = K.p;
    const double t[LTOMPC_NTHETA] = {p.mass, p.inertia_z, p.B_f, p.C_f, p.D_f, p.B_r, p.C_r, p.D_r, p.C_m, p.Cr_0, p.Cr_2, p.q_n, p.q_mu, p.q_B, p.r_du[0], p.r_du[1]};
    for (int j = 0; j < LTOMPC_NTHETA; j++)
      for (size_t b = 0; b < bp; b++) TH[j * bp + b] = t[j];
  }
  W.TH = TH, W.TSV = sets, W.TSI = tsi;
  const Work& Wu = W;
  int* const act = ints(bp, -1);
  int* const nact = ints(1, B);
  for (int b = 0; b < B; b++) act[b] = b;
  Launch la{act, nact, Bp, 0};
  std::vector<double> u0((size_t)2 * B, 0.0), xn((size_t)8 * B);
  const Consts Kc = K;
  for (int tick = 0; tick < ticks; tick++) {
    const int cold = tick == 0;
    grid_bs(B, 64, [&] { k_load_x0(Wu, x.data(), orig, K.o.resto_sticky, cold ? 0 : 1); });
    if (cold) grid_bs(B, 64, [&] { k_zero_uprev(Wu); });
    grid_bs(n * bp, 64, [&] { k_init_ts(&K, &W, cold); });
    memset(W.active, 0, sizeof(int) * (K.o.max_iter + 2)), W.ls_count[0] = W.ls_count[1] = 0;
    for (int it = 0;; it++) {
      grid_bs(n * bp, 64, [&] { k_eval_ts<BoundsRef>(&K, &W, la); });
      wave64("k_riccati8_ts", Bp / 8, [&] { k_riccati8_ts(Kc, W, la, it, 1); });
      if (it >= K.o.max_iter) break;
      grid_bs(n * bp, 64, [&] { k_expand_ts<BoundsRef>(&K, &W, la); });
      grid_bs(n * bp, 64, [&] { k_linesearch_ts<BoundsRef>(&K, &W, la, 0, Bp); });
      wave64("k_pick_ts", (Bp * 8 + 63) / 64, [&] { k_pick_ts(&K, &W, la, 0); });
      if (K.o.n_linesearch > 1 && W.ls_count[0] > 0) {
        const int jw = W.ls_count[0];
        grid_bs((size_t)(K.o.n_linesearch - 1) * n * jw, 64, [&] { k_linesearch_ts<BoundsRef>(&K, &W, la, 1, jw); });
        wave64("k_pick_ts", (jw * 8 + 63) / 64, [&] { k_pick_ts(&K, &W, la, 1); });
      }
      grid_bs(n * bp, 64, [&] { k_update(&K, &Wu, la); });
      int left = 0;
      for (int b = 0; b < B; b++) left += !W.si[(size_t)SI_DONE * Bp + b];
      if (!left) break;
    }
    grid_bs(B, 64, [&] { k_store_u0(Wu, u0.data(), orig); });
    printf("tick %d\n", tick);
    std::vector<int> slot_of(B);
    for (int b = 0; b < B; b++) slot_of[orig[b]] = b;
    for (int r = 0; r < B; r++) {
      const int b = slot_of[r];
      printf("%d %d %d %.17g %.17g\n", r, W.si[(size_t)SI_STATUS * Bp + b], W.si[(size_t)SI_ITERS * Bp + b], u0[2 * r], u0[2 * r + 1]);
    }
    // the plant step on each instance's kappa row (the caller's order), 100 sub-steps
    grid_bs(B, 64, [&] { k_plant_ts(Kc, TH, sets, tsi, Bp, B, x.data(), u0.data(), K.o.t_step, 100, xn.data()); });
    printf("x\n");
    put(xn.data(), xn.size());
    if (tick + 1 < ticks) x = xn;
  }
  // ---- the per-set table gradient of the last solve (sens_compute + tab_compute of deriv_passes.h)
  WorkTS Ws = W;
  Ws.QP = poisoned((size_t)QP_NF * (n + 1) * bp), Ws.RC = poisoned((size_t)RC_NF * (n + 1) * bp);
  Ws.RS = poisoned((size_t)RS_NF * n * bp), Ws.LS = poisoned((size_t)3 * n * bp);
  Ws.si = ints((size_t)SI_NF * bp, 0);
  const Work& Wsu = Ws;
  const WorkPI& Wspi = Ws;
  int *inertia = ints(bp, 0), *ok = ints(bp, 0);
  double *du0 = poisoned((size_t)2 * SENS_NP * B), *margin = poisoned(B);
  grid_bs(n * bp, 64, [&] { k_sens_eval_ts<BoundsRef>(&K, &Ws); });
  wave64("k_sens_riccati8_pi", Bp / 8, [&] { k_sens_riccati8_pi(Kc, Wspi, W.si, inertia); });
  wave64("k_sens_forward", Bp / 8, [&] { k_sens_forward(Wsu, inertia, ni, du0, ok, margin, nullptr, nullptr, nullptr); });
  double *TJ = poisoned((size_t)TJ_NF * n * bp), *sg = poisoned((size_t)TS_NS * n * B), *gs = zeros((size_t)n_sets * TAB_ROWS * nt);
  double *gXd = poisoned(gX.size()), *gUd = poisoned(gU.size());
  memcpy(gXd, gX.data(), sizeof(double) * gX.size()), memcpy(gUd, gU.data(), sizeof(double) * gU.size());
  wave64("k_adj_sweep_tab_pi", Bp / 8, [&] { k_adj_sweep_tab_pi(Wspi, gXd, gUd, TJ); });
  grid_bs(n * bp, 64, [&] { k_tab_cond_ts<BoundsRef>(&K, &W, TJ, ok, sg); });
  grid_bs(3 * n * bp, 256, [&] { k_tab_scatter_ts(&K, Wu, ok, sg, gs, tsi); });
  printf("ok");
  for (int b = 0; b < B; b++) printf(" %d", ok[b]);
  printf("\n");
  std::vector<double> sc(n * B), sx(n * B);  // s of c_k and of x_{k+1}, the caller's order
  for (int b = 0; b < B; b++)
    for (int k = 0; k < N; k++) sc[orig[b] * n + k] = W.C[(size_t)k * Bp + b], sx[orig[b] * n + k] = W.X[(size_t)(k + 1) * Bp + b];
  put(sc.data(), sc.size()), put(sx.data(), sx.size());
  std::vector<double> eps(B);  // the smoothing of each instance's look-ups at its final iterate
  for (int b = 0; b < B; b++) eps[orig[b]] = W.st[(size_t)ST_EPS * Bp + b];
  put(eps.data(), eps.size());
  put(sg, (size_t)TS_NS * n * B);
  put(gs, (size_t)n_sets * TAB_ROWS * nt);
  return 0;
}
