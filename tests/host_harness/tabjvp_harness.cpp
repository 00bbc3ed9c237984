// tabjvp_harness.cpp — TEST INFRASTRUCTURE: the directional pass in the track tables (csrc/table_jvp.h: k_tabjvp_cond,
// k_jvp_sweep_tab and the _pi / _ts forms) compiled as host C++ and run on the lock-step 64-lane wavefront of hip_shim.h under
// AddressSanitizer + UndefinedBehaviorSanitizer, after the re-linearisation and the head-less sweep of sensitivity.h.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
//   tabjvp_harness <problem file>
// The problem file holds a converged primal-dual iterate (the oracle's), the tables and one direction; the program puts the
// instances into permuted slots (orig is not the identity), every buffer at exactly the size the kernels may touch, NaN bit
// patterns wherever a kernel has no business reading (the tables and the direction at their exact size too: a look-up or a gather
// past either end is an ASan error), and prints ok, tX and tU, which tests/test_host_harness_tabjvp.py compares with the dense
// reference (tests/table_jvp_reference.py).
// Problem file (text): `n_table N B eps periodic mode n_sets has_dp has_dt has_ds` (mode 0: uniform, 1: _pi, 2: _ts), then the
// tables (6 x n_table; mode 2: only the grids are used) and, mode 2, the sets (n_sets x 4 x n_table) and the set of every instance
// (B), x0 (B x 8), X (B x (N+1) x 8), C, L1, L2 (B x N x 8), U (B x N x 2), ni, T, NU (B x N x ni), mu (B), with mode >= 1 theta rows
// (B x 16), then the directions that the flags announce: dp (B x 10), dtables (max(n_sets, 1) x 4 x n_table), dslot (B x N x 10).
// Nothing in the package uses this file.
#include "layout.h"

inline double atomicAdd(double* p, double v) {  // (table_sensitivity.h's scatter, not run here; hip_shim.h's atomicAdd is for integers)
  const double old = *p;
  *p = old + v;
  return old;
}

#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"
#include "eval8.h"
#include "table_jvp.h"

#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

using namespace ltompc;

static double* poisoned(size_t n) {
  double* p = (double*)malloc((n ? n : 1) * sizeof(double));
  memset(p, 0xFF, (n ? n : 1) * sizeof(double));
  return p;
}
static double* zeros(size_t n) { return (double*)calloc(n ? n : 1, sizeof(double)); }
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
static void build_bounds(const ltompc_params& p, Bounds& b) {  // = build_bounds (ltompc.hip)
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

// The tables of a problem file at their exact size, and Tables over them
struct TableSet {
  int n = 0;
  double* rows[6] = {};
  Tables T{};
  bool load(FILE* f, int n_table, int periodic) {
    n = n_table;
    for (int r = 0; r < 6; r++) {
      rows[r] = poisoned(n);
      if (!read(f, rows[r], n)) return false;
    }
    T.n = n, T.s_kappa = rows[0], T.kappa = rows[1], T.s_arc = rows[2], T.n_left = rows[3], T.n_right = rows[4], T.v_ref = rows[5];
    T.g0_kappa = rows[0][0], T.inv_kappa = (double)(n - 1) / (rows[0][n - 1] - rows[0][0]);
    T.g0_arc = rows[2][0], T.inv_arc = (double)(n - 1) / (rows[2][n - 1] - rows[2][0]);
    T.period = periodic ? rows[0][n - 1] - rows[0][0] : 0.0;
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: tabjvp_harness <problem file>\n"), 2;
  FILE* f = fopen(argv[1], "r");
  int n_table, N, B, periodic, mode, n_sets, has_dp, has_dt, has_ds;
  double eps;
  if (!f || fscanf(f, "%d %d %d %lf %d %d %d %d %d %d", &n_table, &N, &B, &eps, &periodic, &mode, &n_sets, &has_dp, &has_dt, &has_ds) != 10)
    return fprintf(stderr, "bad problem file\n"), 2;
  const bool PI = mode >= 1, TSM = mode == 2;
  if (TSM != (n_sets > 0)) return fprintf(stderr, "n_sets and mode disagree\n"), 2;
  const int Bp = (B + 63) / 64 * 64;
  const size_t n = N, bp = Bp, nt = n_table;
  Consts K{};
  default_params(&K.p);
  memset(&K.o, 0, sizeof K.o);
  K.o.t_step = 0.1, K.o.periodic_tables = periodic, K.o.smooth_eps_min = eps;
  build_bounds(K.p, K.bd);
  TableSet ts;
  if (!ts.load(f, n_table, periodic)) return fprintf(stderr, "short problem file (tables)\n"), 2;
  K.T = ts.T;
  double* sets = nullptr;
  int* tsi = nullptr;
  if (TSM) {  // the handle's own value rows: NaN at their exact size (no instance may read them)
    for (int r : {1, 3, 4, 5}) memset(ts.rows[r], 0xFF, sizeof(double) * nt);
    sets = poisoned((size_t)n_sets * TAB_ROWS * nt);
    std::vector<double> idx_in(B);
    if (!read(f, sets, (size_t)n_sets * TAB_ROWS * nt) || !read(f, idx_in.data(), B)) return fprintf(stderr, "short problem file (sets)\n"), 2;
    tsi = (int*)malloc(sizeof(int) * B);  // exactly B entries, in the caller's order
    for (int b = 0; b < B; b++) tsi[b] = (int)idx_in[b];
  }
  const int ni = K.bd.ni;
  std::vector<double> x0((size_t)8 * B), X((n + 1) * 8 * B), C(n * 8 * B), L1(n * 8 * B), L2(n * 8 * B), U(n * 2 * B), mu(B);
  std::vector<double> rows((size_t)LTOMPC_NTHETA * B);
  int ni_file = 0;
  bool good = read(f, x0.data(), x0.size()) && read(f, X.data(), X.size()) && read(f, C.data(), C.size()) && read(f, L1.data(), L1.size()) &&
              read(f, L2.data(), L2.size()) && read(f, U.data(), U.size()) && fscanf(f, "%d", &ni_file) == 1 && ni_file == ni;
  std::vector<double> Tt(n * ni * B), NUt(n * ni * B);
  good = good && read(f, Tt.data(), Tt.size()) && read(f, NUt.data(), NUt.size()) && read(f, mu.data(), mu.size()) &&
         (!PI || read(f, rows.data(), rows.size()));
  // the directions, each at its exact size
  const size_t n_dt = (size_t)(TSM ? n_sets : 1) * TAB_ROWS * nt;
  double *dp = has_dp ? poisoned((size_t)JVP_NP * B) : nullptr, *dt = has_dt ? poisoned(n_dt) : nullptr, *ds = has_ds ? poisoned(TS_NS * n * B) : nullptr;
  good = good && (!dp || read(f, dp, (size_t)JVP_NP * B)) && (!dt || read(f, dt, n_dt)) && (!ds || read(f, ds, TS_NS * n * B));
  fclose(f);
  if (!good) return fprintf(stderr, "short problem file\n"), 2;
  // ---- slot b holds the caller's instance orig[b]: a permutation that is not the identity (B > 1)
  int* orig = (int*)malloc(sizeof(int) * B);
  {
    auto gcd = [](int a, int c) { while (c) { const int t = a % c; a = c, c = t; } return a; };
    int step = 2;
    while (gcd(step, B) != 1) step++;
    for (int b = 0; b < B; b++) orig[b] = (int)(((long long)step * b + B / 2) % B);
  }
  // ---- the solver's Work: the iterate and st / si; everything else the pass must not touch stays null
  WorkTS W{};
  W.N = N, W.B = B, W.Bp = Bp;
  W.X = poisoned(8 * (n + 1) * bp), W.C = poisoned(8 * n * bp), W.U = poisoned(2 * n * bp), W.L1 = poisoned(8 * n * bp), W.L2 = poisoned(8 * n * bp);
  W.T = poisoned((ni + NNL) * n * bp), W.NU = poisoned(ni * n * bp);
  W.x0 = poisoned(8 * bp), W.uprev = zeros(2 * bp), W.st = zeros((size_t)ST_NF * bp);
  W.si = (int*)calloc((size_t)SI_NF * bp, sizeof(int));
  W.orig = orig;
  double* TH = poisoned((size_t)LTOMPC_NTHETA * bp);
  W.TH = TH, W.TSV = sets, W.TSI = tsi;
  for (int b = 0; b < B; b++) {
    const size_t o = orig[b];
#define PUT(plane, F, NK, src) \
  for (int k = 0; k < (NK); k++) \
    for (int q = 0; q < (F); q++) plane[((size_t)q * (NK) + k) * Bp + b] = src[(o * (NK) + k) * (F) + q];
    PUT(W.X, 8, N + 1, X) PUT(W.C, 8, N, C) PUT(W.U, 2, N, U) PUT(W.L1, 8, N, L1) PUT(W.L2, 8, N, L2) PUT(W.T, ni, N, Tt) PUT(W.NU, ni, N, NUt)
#undef PUT
    for (int q = 0; q < 8; q++) W.x0[(size_t)q * Bp + b] = x0[o * 8 + q], W.X[((size_t)q * (N + 1)) * Bp + b] = x0[o * 8 + q];
    W.st[(size_t)ST_MU * Bp + b] = mu[o], W.st[(size_t)ST_EPS * Bp + b] = eps, W.st[(size_t)ST_TAU * Bp + b] = 0.99;
    for (int q = 0; q < LTOMPC_NTHETA; q++) TH[(size_t)q * Bp + o] = rows[o * LTOMPC_NTHETA + q];  // (the caller's order)
  }
  // ---- the pass's Work (sens_compute): QP, RC, RS, LS of its own, si zeros
  WorkTS Ws = W;
  Ws.QP = poisoned((size_t)QP_NF * (n + 1) * bp), Ws.RC = poisoned((size_t)RC_NF * (n + 1) * bp);
  Ws.RS = poisoned((size_t)RS_NF * n * bp), Ws.LS = poisoned((size_t)3 * n * bp);
  Ws.si = (int*)calloc((size_t)SI_NF * bp, sizeof(int));
  int *inertia = (int*)calloc(bp, sizeof(int)), *ok = (int*)calloc(bp, sizeof(int));
  double *du0 = poisoned((size_t)2 * SENS_NP * B), *margin = poisoned(B);
  const Work& Wu = W;
  const WorkPI& Wpi = W;
  const Work& Wsu = Ws;
  const WorkPI& Wspi = Ws;
  if (TSM) grid_bs(n * bp, 64, [&] { k_sens_eval_ts<BoundsRef>(&K, &Ws); });
  else if (PI) grid_bs(n * bp, 64, [&] { k_sens_eval_pi<BoundsRef>(&K, &Wspi); });
  else grid_bs(n * bp, 64, [&] { k_sens_eval<BoundsRef, false>(&K, &Wsu); });
  if (PI) wave64("k_sens_riccati8_pi", Bp / 8, [&] { k_sens_riccati8_pi(K, Wspi, W.si, inertia); });
  else wave64("k_sens_riccati8", Bp / 8, [&] { k_sens_riccati8(K, Wsu, W.si, inertia); });
  wave64("k_sens_forward", Bp / 8, [&] { k_sens_forward(Wsu, inertia, ni, du0, ok, margin, nullptr, nullptr, nullptr); });
  // ---- tjv_compute (deriv_passes.h): the slots' stage vectors, then the sweep
  double *TQ = poisoned((size_t)TQ_NF * n * bp), *JV = poisoned((size_t)JV_NF * n * bp);
  double *tX = poisoned((n + 1) * 8 * B), *tU = poisoned(n * 2 * B);
  if (TSM) grid_bs(n * bp, 64, [&] { k_tabjvp_cond_ts<BoundsRef>(&K, &W, ok, dt, ds, TQ); });
  else if (PI) grid_bs(n * bp, 64, [&] { k_tabjvp_cond_pi<BoundsRef>(&K, &Wpi, ok, dt, ds, TQ); });
  else grid_bs(n * bp, 64, [&] { k_tabjvp_cond<BoundsRef>(&K, &Wu, ok, dt, ds, TQ); });
  if (PI) wave64("k_jvp_sweep_tab_pi", Bp / 8, [&] { k_jvp_sweep_tab_pi(Wspi, TQ, ok, dp, JV, tX, tU); });
  else wave64("k_jvp_sweep_tab", Bp / 8, [&] { k_jvp_sweep_tab(Wsu, K.p.r_du[0], K.p.r_du[1], TQ, ok, dp, JV, tX, tU); });
  printf("ok");
  for (int b = 0; b < B; b++) printf(" %d", ok[b]);
  printf("\n");
  put(tX, (n + 1) * 8 * B);
  put(tU, n * 2 * B);
  return 0;
}
