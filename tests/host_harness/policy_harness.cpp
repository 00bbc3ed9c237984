// policy_harness.cpp — TEST INFRASTRUCTURE: the kernels of the feedback policy (csrc/policy.h) compiled as host C++
// and run under AddressSanitizer + UndefinedBehaviorSanitizer: k_policy_gather on hip_shim.h's lock-step workgroup (4 wavefronts,
// one __syncthreads), k_policy_step and k_policy_run / k_policy_run_pi lane after lane (thread per instance, no collective).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// No solve: the prediction X, U, the gains in the Riccati buffer, u_prev, ok and a non-identity orig are seeded data in buffers of
// exactly the size the kernels may touch - the Riccati buffer ends with stage N-1, orig, ok and every row-major array with
// instance B-1 - filled with NaN bit patterns wherever the kernels have no business reading.  Cases: B = 13 and 61 (padding
// lanes), N = 2 and 10, uniform and per-instance rows, every stage for the step (with and without v, with and without clip) and
// k0 + n = N for the run.  Each is compared BIT FOR BIT with a serial restatement on natural arrays in this program (the same
// fma order; the plant step of the restatement is k_plant / k_plant_pi itself), and checked for exact zeros / U_k where ok = 0.
// The restatement follows the kernels' formulas: it checks the mechanics (the tile transpose, the field and stage indices,
// padding lanes, orig, the ok mask, every address), not the mathematics, which tests/test_gpu_policy.py checks against the dense
// reference.  Prints one line per case; exit status 1 when a check fails.  Nothing in the package uses this file.
#include "hip_shim.h"

#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "aux_kernels.h"
#include "eval8.h"
#include "sensitivity.h"
#include "policy.h"

#include <cmath>
#include <random>
#include <type_traits>
#include <vector>

using namespace ltompc;

static double* poisoned(size_t n) {
  double* p = (double*)malloc((n ? n : 1) * sizeof(double));
  memset(p, 0xFF, (n ? n : 1) * sizeof(double));
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
template <typename F>
static void grid_bs(size_t threads, unsigned bs, F&& body) {  // a thread-per-element kernel, lane after lane
  blockDim.x = bs, gridDim.x = (unsigned)((threads + bs - 1) / bs);
  for (unsigned blk = 0; blk < gridDim.x; blk++)
    for (unsigned t = 0; t < bs; t++) blockIdx.x = blk, threadIdx.x = t, body();
}
template <typename F>
static void wg256_2d(const char* name, int bx, int by, F&& body) {  // workgroups of 4 wavefronts on the lock-step workgroup
  blockDim.x = 256, gridDim.x = bx, gridDim.y = by;
  for (int y = 0; y < by; y++)
    for (int x = 0; x < bx; x++) {
      blockIdx.x = x, blockIdx.y = y;
      LtWave::self().run(name, 4, LtWave::STACK_SMALL, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, &body);
    }
  blockIdx.y = 0, gridDim.y = 1;
}
static bool same(const double a, const double b) { return memcmp(&a, &b, sizeof a) == 0 || (a == 0.0 && b == 0.0); }

// the clip rule of include/ltompc.h, restated
static double clipped(const ltompc_params& p, const double dt, const int c, const double xc, double u) {
  if (p.x_lb[6 + c] > -LTOMPC_NO_BOUND) u = fmax(u, (p.x_lb[6 + c] - xc) / dt);
  if (p.x_ub[6 + c] < LTOMPC_NO_BOUND) u = fmin(u, (p.x_ub[6 + c] - xc) / dt);
  if (p.u_lb[c] > -LTOMPC_NO_BOUND) u = fmax(u, p.u_lb[c]);
  if (p.u_ub[c] < LTOMPC_NO_BOUND) u = fmin(u, p.u_ub[c]);
  return u;
}

struct Stage {  // one instance, one stage: natural arrays
  double X[8], U[2], K[2][8], Kv[2][2];
};

static int run_case(const int B, const int N, const bool PI, std::mt19937_64& rng) {
  const int Bp = (B + 63) / 64 * 64, n_table = 33, n_sub = 3;
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  Consts K{};
  default_params(&K.p);
  K.o.t_step = 0.1;
  K.p.x_ub[7] = LTOMPC_NO_BOUND;  // (one bound of the clip rule absent)
  // ---- tables: uniform grids over [0, 120] m, a gentle curvature
  double* rows[6];
  for (int r = 0; r < 6; r++) rows[r] = poisoned(n_table);
  for (int j = 0; j < n_table; j++) {
    const double s = 120.0 * j / (n_table - 1);
    rows[0][j] = rows[2][j] = s, rows[1][j] = 0.02 * sin(0.1 * s), rows[3][j] = 3.0, rows[4][j] = -3.0, rows[5][j] = 12.0;
  }
  Tables& T = K.T;
  T.n = n_table, T.s_kappa = rows[0], T.kappa = rows[1], T.s_arc = rows[2], T.n_left = rows[3], T.n_right = rows[4], T.v_ref = rows[5];
  T.g0_kappa = rows[0][0], T.inv_kappa = (double)(n_table - 1) / (rows[0][n_table - 1] - rows[0][0]);
  T.g0_arc = rows[2][0], T.inv_arc = (double)(n_table - 1) / (rows[2][n_table - 1] - rows[2][0]);
  T.period = 0.0;
  // ---- the data, per slot b and stage k
  std::vector<std::vector<Stage>> S(B, std::vector<Stage>(N + 1));
  for (int b = 0; b < B; b++)
    for (int k = 0; k <= N; k++) {
      Stage& s = S[b][k];
      const double x[8] = {10.0 + 0.8 * k + 5.0 * uni(rng), 0.3 * uni(rng), 0.05 * uni(rng), 8.0 + uni(rng), 0.1 * uni(rng), 0.1 * uni(rng),
                           0.1 * uni(rng), 0.3 + 0.2 * uni(rng)};
      memcpy(s.X, x, sizeof x);
      s.U[0] = 0.3 * uni(rng), s.U[1] = 0.5 * uni(rng);
      for (int c = 0; c < 2; c++) {
        for (int i = 0; i < 8; i++) s.K[c][i] = 0.2 * uni(rng);
        for (int e = 0; e < 2; e++) s.Kv[c][e] = 0.3 * uni(rng);
      }
    }
  std::vector<int> orig(B);  // slot -> caller's index: a permutation that is not the identity
  for (int b = 0; b < B; b++) orig[b] = (5 * b + 3) % B;  // (5 is coprime to 13 and 61)
  // ---- the kernels' buffers: exact sizes, NaN wherever nothing was put
  Work W{};
  W.N = N, W.B = B, W.Bp = Bp;
  double *RC = poisoned((size_t)RC_NF * N * Bp), *Xp = poisoned((size_t)8 * (N + 1) * Bp), *Up = poisoned((size_t)2 * N * Bp);
  double *uprev = poisoned(2 * (size_t)B), *TH = poisoned((size_t)LTOMPC_NTHETA * Bp);
  int *orig_x = (int*)malloc(sizeof(int) * B), *ok = (int*)malloc(sizeof(int) * B);
  memcpy(orig_x, orig.data(), sizeof(int) * B);
  for (int o = 0; o < B; o++) {
    ok[o] = o % 5 != 2;
    uprev[2 * o] = 0.3 * uni(rng), uprev[2 * o + 1] = 0.5 * uni(rng);
    const double th[LTOMPC_NTHETA] = {K.p.mass * (1.0 + 0.1 * uni(rng)), K.p.inertia_z * (1.0 + 0.1 * uni(rng)), K.p.B_f, K.p.C_f, K.p.D_f * (1.0 + 0.05 * uni(rng)),
                                      K.p.B_r, K.p.C_r, K.p.D_r, K.p.C_m * (1.0 + 0.1 * uni(rng)), K.p.Cr_0, K.p.Cr_2, K.p.q_n, K.p.q_mu, K.p.q_B,
                                      K.p.r_du[0], K.p.r_du[1]};
    for (int j = 0; j < LTOMPC_NTHETA; j++) TH[(size_t)j * Bp + o] = th[j];
  }
  for (int b = 0; b < B; b++)
    for (int k = 0; k <= N; k++) {
      const Stage& s = S[b][k];
      for (int i = 0; i < 8; i++) PL(Xp, i, k, N + 1) = s.X[i];
      if (k == N) continue;
      PL(Up, 0, k, N) = s.U[0], PL(Up, 1, k, N) = s.U[1];
      if (!ok[orig[b]]) continue;  // (the gains of a rejected instance stay NaN: nothing of them may reach an output)
      for (int c = 0; c < 2; c++) {
        for (int i = 0; i < 8; i++) PG(RC, RC_K + c * 8 + i, k, RC_NF) = s.K[c][i];
        for (int e = 0; e < 2; e++) PG(RC, RC_Kv + c * 2 + e, k, RC_NF) = s.Kv[c][e];
      }
    }
  W.RC = RC, W.X = Xp, W.U = Up, W.orig = orig_x;
  int bad = 0;
  // ---- the gather
  double *Ko = poisoned((size_t)B * N * 16), *Kvo = poisoned((size_t)B * N * 4);
  wg256_2d("k_policy_gather", Bp / 8, (N + POL_KS - 1) / POL_KS, [&] { k_policy_gather(W, ok, Ko, Kvo); });
  for (int b = 0; b < B; b++) {
    const size_t o = orig[b];
    for (int k = 0; k < N; k++)
      for (int c = 0; c < 2; c++) {
        for (int i = 0; i < 8; i++) bad += !same(Ko[((o * N + k) * 2 + c) * 8 + i], ok[o] ? S[b][k].K[c][i] : 0.0);
        for (int e = 0; e < 2; e++) bad += !same(Kvo[((o * N + k) * 2 + c) * 2 + e], ok[o] ? S[b][k].Kv[c][e] : 0.0);
      }
  }
  // one output alone (the other NULL) writes the same words
  double* Ko2 = poisoned((size_t)B * N * 16);
  wg256_2d("k_policy_gather", Bp / 8, (N + POL_KS - 1) / POL_KS, [&] { k_policy_gather(W, ok, Ko2, (double*)nullptr); });
  bad += memcmp(Ko, Ko2, sizeof(double) * B * N * 16) != 0;
  // ---- the law, restated: pi_k of the instance in slot b
  const auto law = [&](const int b, const int k, const double* x, const double* v, const int clip, double* u) {
    const size_t o = orig[b];
    const Stage& s = S[b][k];
    for (int c = 0; c < 2; c++) {
      double acc = 0.0;
      if (ok[o]) {
        for (int i = 0; i < 8; i++) acc = std::fma(s.K[c][i], x[i] - s.X[i], acc);
        for (int e = 0; e < 2; e++) acc = std::fma(s.Kv[c][e], v ? v[e] - (k ? S[b][k - 1].U[e] : uprev[2 * o + e]) : 0.0, acc);
      }
      u[c] = ok[o] ? s.U[c] + acc : s.U[c];
      if (clip) u[c] = clipped(K.p, K.o.t_step, c, x[6 + c], u[c]);
    }
  };
  // ---- the step: every stage, with and without v, with and without clip (x near the prediction, some rows far enough to saturate)
  std::vector<double> x((size_t)B * 8), v((size_t)B * 2);
  double* u = poisoned((size_t)B * 2);
  int n_clip = 0;
  for (int k = 0; k < N; k++)
    for (int with_v = 0; with_v < 2; with_v++)
      for (int clip = 0; clip < 2; clip++) {
        for (int b = 0; b < B; b++) {
          const size_t o = orig[b];
          const double far = (b + k) % 3 == 0 ? 30.0 : 1.0;
          for (int i = 0; i < 8; i++) x[o * 8 + i] = S[b][k].X[i] + 0.05 * far * uni(rng);
          for (int e = 0; e < 2; e++) v[o * 2 + e] = 0.5 * far * uni(rng);
        }
        memset(u, 0xFF, sizeof(double) * B * 2);
        const double* vp = with_v ? v.data() : nullptr;
        grid_bs(Bp, 64, [&] { k_policy_step(K, W, ok, uprev, k, x.data(), vp, clip, u); });
        for (int b = 0; b < B; b++) {
          const size_t o = orig[b];
          double ref[2], raw[2];
          law(b, k, &x[o * 8], with_v ? &v[o * 2] : nullptr, clip, ref);
          law(b, k, &x[o * 8], with_v ? &v[o * 2] : nullptr, 0, raw);
          for (int c = 0; c < 2; c++) bad += !(std::isfinite(u[o * 2 + c]) && same(u[o * 2 + c], ref[c])), n_clip += clip && ref[c] != raw[c];
          if (!ok[o] && !clip) bad += !same(u[o * 2], S[b][k].U[0]) || !same(u[o * 2 + 1], S[b][k].U[1]);
        }
      }
  if (!n_clip) bad++, printf("FAIL: no row of the step saturated\n");
  // ---- the run: k0 + n = N from k0 = N / 2, logs on; then from k0 = 0 without v and without logs, against the same loop of
  // the restated law and the plant kernel itself
  for (int pass = 0; pass < 2; pass++) {
    const int k0 = pass == 0 ? N / 2 : 0, n = N - k0, clip = pass == 0 ? 1 : 0;
    const bool with_v = pass == 0, logs = pass == 0;
    double *xr = poisoned((size_t)B * 8), *ul = poisoned((size_t)B * n * 2), *xl = poisoned((size_t)B * n * 8);
    for (int b = 0; b < B; b++) {
      const size_t o = orig[b];
      for (int i = 0; i < 8; i++) x[o * 8 + i] = xr[o * 8 + i] = S[b][k0].X[i] + 0.05 * uni(rng);
      for (int e = 0; e < 2; e++) v[o * 2 + e] = 0.3 * uni(rng);
    }
    const double* vp = with_v ? v.data() : nullptr;
    double *ulp = logs ? ul : nullptr, *xlp = logs ? xl : nullptr;
    if (PI) grid_bs(Bp, 64, [&] { k_policy_run_pi(K, W, ok, uprev, k0, n, xr, vp, n_sub, clip, ulp, xlp, TH); });
    else grid_bs(Bp, 64, [&] { k_policy_run(K, W, ok, uprev, k0, n, xr, vp, n_sub, clip, ulp, xlp); });
    std::vector<double> xs(x), vs(v), us((size_t)B * 2), xn((size_t)B * 8);
    for (int j = 0; j < n; j++) {
      for (int b = 0; b < B; b++) {
        const size_t o = orig[b];
        law(b, k0 + j, &xs[o * 8], (with_v || j) ? &vs[o * 2] : nullptr, clip, &us[o * 2]);
      }
      if (PI) grid_bs(B, 64, [&] { k_plant_pi(K, TH, Bp, B, xs.data(), us.data(), K.o.t_step, n_sub, xn.data()); });
      else grid_bs(B, 64, [&] { k_plant(K, B, xs.data(), us.data(), K.o.t_step, n_sub, xn.data()); });
      for (size_t o = 0; o < (size_t)B; o++) {
        for (int c = 0; c < 2 && logs; c++) bad += !same(ul[(o * n + j) * 2 + c], us[o * 2 + c]);
        for (int i = 0; i < 8 && logs; i++) bad += !same(xl[(o * n + j) * 8 + i], xn[o * 8 + i]);
        for (int i = 0; i < 8; i++) bad += !std::isfinite(xn[o * 8 + i]);
      }
      xs = xn, vs = us;
    }
    for (size_t e = 0; e < (size_t)B * 8; e++) bad += !same(xr[e], xs[e]);
    free(xr), free(ul), free(xl);
  }
  printf("case B=%d N=%d pi=%d: clipped %d bad %d\n", B, N, (int)PI, n_clip, bad);
  for (int r = 0; r < 6; r++) free(rows[r]);
  free(RC), free(Xp), free(Up), free(uprev), free(TH), free(orig_x), free(ok), free(Ko), free(Kvo), free(Ko2), free(u);
  return bad != 0;
}

int main() {
  std::mt19937_64 rng(20241105);
  int failed = 0;
  for (int B : {13, 61})
    for (int N : {2, 10})
      for (int PI = 0; PI < 2; PI++) failed += run_case(B, N, PI != 0, rng);
  failed += run_case(13, POL_KS + 2, false, rng);  // (a second chunk of stages in k_policy_gather)
  printf("failed %d\n", failed);
  return failed ? 1 : 0;
}
