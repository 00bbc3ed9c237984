// policy.h — the feedback policy of a solve (ltompc_get_policy, ltompc_policy_step, ltompc_policy_run_dev).  The
// delta_w = 0 factorisation of the sensitivity pass (k_sens_riccati8, sensitivity.h) leaves the gains of every stage in the pass's
// Riccati buffer: K_k (2 x 8, RC_K) and Kv_k (2 x 2, RC_Kv), the words k_sens_forward propagates.  With V_0 = the u_prev of that
// solve and V_k = U_{k-1},
//     pi_k(x, v) = U_k + K_k (x - X_k) + Kv_k (v - V_k),      k = 0 .. N-1,
// and pi_k = U_k with K_k = Kv_k = 0 for an instance the pass rejected (ok = 0).  Three kinds of kernel:
//
//   k_policy_gather    the gains of all stages -> K [B][N][2][8], Kv [B][N][2][2] in the caller's order, an LDS tile transpose
//   k_policy_step      u = pi_k(x, v), thread per instance, reading iterate and gains where they are (no gather)
//   k_policy_run       n ticks of [u_j = pi_{k0+j}(x, v); x <- d_plant(x, u_j); v <- u_j] in one launch, thread per instance as
//   (_pi, _ts)         k_plant (k_plant_pi, k_plant_ts): the same d_plant call, so the states have the plant step's bits
//
// All of them read the iterate, the gains and the packing, and write only the caller's arrays.  x, v, u and the logs are
// row-major in the caller's order; a thread works on the instance in slot b and addresses them through orig[b].
#pragma once
#include "aux_kernels.h"
#include "sensitivity.h"

namespace ltompc {

constexpr int POL_NF = RC_Kv + 4;  // fields 0..19 of a stage of the Riccati buffer: K_k row-major (16), Kv_k row-major (4)
constexpr int POL_KS = 16;         // stages of one workgroup of k_policy_gather
constexpr int POL_PITCH = 9;       // doubles per field of the tile (8 instances + 1: the transposed read stays off one bank group)
static_assert(RC_K == 0 && RC_Kv == 16, "k_policy_gather copies fields [0, POL_NF) of a stage");

// For one stage and the eight instances of group t the source is POL_NF * 8 = 160 consecutive doubles (layout.h, PG); for one
// instance and consecutive stages the destination is 16 (4) consecutive doubles per stage.  A thread per (instance, stage, word)
// in either order would touch 8 bytes per 64-byte sector on one side, so a workgroup moves a tile of POL_KS stages x 8 instances
// through LDS: in by the source's order (a stage: 1280 contiguous bytes), out by the destination's (an instance: 128 POL_KS
// contiguous bytes of K, 32 POL_KS of Kv).  Zeros where ok = 0 (the buffer may hold anything there).  Workgroup = (group t, chunk
// of stages); pad instances (slot >= B) are not written, no index leaves stages [0, N) of the buffer.
__global__ void __launch_bounds__(256) k_policy_gather(Work W, const int* __restrict__ ok, double* __restrict__ Ko, double* __restrict__ Kvo) {
  __shared__ double tile[POL_KS][POL_NF * POL_PITCH];
  const int N = W.N, G8 = W.Bp >> 3;
  const int t = blockIdx.x, k0 = blockIdx.y * POL_KS;
  const int nk = N - k0 < POL_KS ? N - k0 : POL_KS;
  const int tid = threadIdx.x;
  for (int e = tid; e < nk * POL_NF * 8; e += blockDim.x) {
    const int k = e / (POL_NF * 8), w = e % (POL_NF * 8);
    tile[k][(w >> 3) * POL_PITCH + (w & 7)] = W.RC[((size_t)(k0 + k) * G8 + t) * (RC_NF * 8) + w];
  }
  __syncthreads();
  if (Ko)
    for (int e = tid; e < 8 * nk * 16; e += blockDim.x) {
      const int g = e / (nk * 16), r = e % (nk * 16), k = r >> 4, f = r & 15;
      const int b = t * 8 + g;
      if (b >= W.B) continue;
      const size_t ob = W.orig[b];
      Ko[(ob * N + k0 + k) * 16 + f] = ok[ob] ? tile[k][f * POL_PITCH + g] : 0.0;
    }
  if (Kvo)
    for (int e = tid; e < 8 * nk * 4; e += blockDim.x) {
      const int g = e / (nk * 4), r = e % (nk * 4), k = r >> 2, f = r & 3;
      const int b = t * 8 + g;
      if (b >= W.B) continue;
      const size_t ob = W.orig[b];
      Kvo[(ob * N + k0 + k) * 4 + f] = ok[ob] ? tile[k][(RC_Kv + f) * POL_PITCH + g] : 0.0;
    }
}

// pi_k(x, v) of the instance in slot b (caller's index r; 0 <= k < N), saturated when `clip`.  has_v = false: v = V_k.  The sums
// are explicit fma chains in a fixed order, so that every kernel that evaluates the policy gives the same bits.
// uprev: the u_prev of the solve, [B][2] in the caller's order (DerivState::d_psens_uprev).
__device__ __forceinline__ void d_policy_eval(const Consts& K, const Work& W, const int ok, const double* __restrict__ uprev, const int k,
                                              const int b, const size_t r, const double* x, const double* v, const bool has_v,
                                              const int clip, double* u) {
  const int N = W.N;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const double Uk = PL(W.U, c, k, N);
    double s = 0.0;
    if (ok) {
#pragma unroll
      for (int i = 0; i < 8; i++) s = fma(PG(W.RC, RC_K + c * 8 + i, k, RC_NF), x[i] - PL(W.X, i, k, N + 1), s);
#pragma unroll
      for (int l = 0; l < 2; l++) {
        const double Vk = k == 0 ? uprev[r * 2 + l] : PL(W.U, l, k - 1, N);
        s = fma(PG(W.RC, RC_Kv + c * 2 + l, k, RC_NF), has_v ? v[l] - Vk : 0.0, s);
      }
    }
    u[c] = ok ? Uk + s : Uk;
  }
  if (!clip) return;
  // delta and T integrate the inputs exactly over one t_step under a held input: their bounds first, the input bounds win
  const double dt = K.o.t_step;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    double uc = u[c];
    if (K.p.x_lb[6 + c] > -LTOMPC_NO_BOUND) uc = fmax(uc, (K.p.x_lb[6 + c] - x[6 + c]) / dt);
    if (K.p.x_ub[6 + c] < LTOMPC_NO_BOUND) uc = fmin(uc, (K.p.x_ub[6 + c] - x[6 + c]) / dt);
    if (K.p.u_lb[c] > -LTOMPC_NO_BOUND) uc = fmax(uc, K.p.u_lb[c]);
    if (K.p.u_ub[c] < LTOMPC_NO_BOUND) uc = fmin(uc, K.p.u_ub[c]);
    u[c] = uc;
  }
}

// u[r] = pi_k(x[r], v[r]) (v = nullptr: V_k); x [B][8], v [B][2], u [B][2]
__global__ void __launch_bounds__(64) k_policy_step(Consts K, Work W, const int* __restrict__ ok, const double* __restrict__ uprev, int k,
                                                    const double* __restrict__ x, const double* __restrict__ v, int clip,
                                                    double* __restrict__ u) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  const size_t r = W.orig[b];
  double xb[8], vb[2] = {0.0, 0.0}, ub[2];
#pragma unroll
  for (int i = 0; i < 8; i++) xb[i] = x[r * 8 + i];
  if (v) vb[0] = v[r * 2], vb[1] = v[r * 2 + 1];
  d_policy_eval(K, W, ok[r], uprev, k, b, r, xb, vb, v != nullptr, clip, ub);
  u[r * 2] = ub[0], u[r * 2 + 1] = ub[1];
}

// n ticks from stage k0 (k0 + n <= N): x [B][8] in and out, v [B][2] or nullptr (V_k0), u_log [B][n][2] and x_log [B][n][8] (the
// state after each tick) or nullptr; v and u_log carry no __restrict__: with n = 1 they may be one array (a thread reads its row of v
// before it writes that row of u_log).  K: the handle's constants in effect (the plant's tables, as k_plant); th, tsv, tsi as the
// plant kernels take them, in the caller's order.
template <bool PI, bool TS>
__device__ __forceinline__ void d_policy_run(const Consts& K, const Work& W, const int* __restrict__ ok, const double* __restrict__ uprev,
                                             const int k0, const int n, double* __restrict__ x, const double* v, const int n_sub,
                                             const int clip, double* u_log, double* __restrict__ x_log,
                                             const double* __restrict__ th, const double* __restrict__ tsv, const int* __restrict__ tsi) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  const size_t r = W.orig[b];
  const int okb = ok[r];
  const double dt = K.o.t_step;
  double xb[8], y[8], vb[2] = {0.0, 0.0}, uu[2];
#pragma unroll
  for (int i = 0; i < 8; i++) xb[i] = x[r * 8 + i];
  bool has_v = v != nullptr;
  if (has_v) vb[0] = v[r * 2], vb[1] = v[r * 2 + 1];
#pragma unroll 1
  for (int j = 0; j < n; j++) {
    d_policy_eval(K, W, okb, uprev, k0 + j, b, r, xb, vb, has_v, clip, uu);
    if (u_log) u_log[(r * n + j) * 2] = uu[0], u_log[(r * n + j) * 2 + 1] = uu[1];
    if constexpr (TS) d_plant<true, const double*, true>(K, xb, uu, dt, n_sub, y, th, W.Bp, r, tsv, tsi[r]);
    else if constexpr (PI) d_plant<true>(K, xb, uu, dt, n_sub, y, th, W.Bp, r);
    else d_plant(K, xb, uu, dt, n_sub, y);
#pragma unroll
    for (int i = 0; i < 8; i++) xb[i] = y[i];
    if (x_log) {
#pragma unroll
      for (int i = 0; i < 8; i++) x_log[(r * n + j) * 8 + i] = y[i];
    }
    vb[0] = uu[0], vb[1] = uu[1], has_v = true;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) x[r * 8 + i] = xb[i];
}
__global__ void __launch_bounds__(64) k_policy_run(Consts K, Work W, const int* __restrict__ ok, const double* __restrict__ uprev, int k0, int n,
                                                   double* __restrict__ x, const double* v, int n_sub, int clip,
                                                   double* u_log, double* __restrict__ x_log) {
  d_policy_run<false, false>(K, W, ok, uprev, k0, n, x, v, n_sub, clip, u_log, x_log, nullptr, nullptr, nullptr);
}
// with per-instance vehicle parameters: th is a [LTOMPC_NTHETA][Bp] plane in the caller's instance order (as k_plant_pi)
__global__ void __launch_bounds__(64) k_policy_run_pi(Consts K, Work W, const int* __restrict__ ok, const double* __restrict__ uprev, int k0, int n,
                                                      double* __restrict__ x, const double* v, int n_sub, int clip,
                                                      double* u_log, double* __restrict__ x_log, const double* __restrict__ th) {
  d_policy_run<true, false>(K, W, ok, uprev, k0, n, x, v, n_sub, clip, u_log, x_log, th, nullptr, nullptr);
}
// ... and per-instance table sets: tsv [n_sets][LTOMPC_TABLE_VALUE_ROWS][n_table], tsi [Bp] in the caller's order (as k_plant_ts)
__global__ void __launch_bounds__(64) k_policy_run_ts(Consts K, Work W, const int* __restrict__ ok, const double* __restrict__ uprev, int k0, int n,
                                                      double* __restrict__ x, const double* v, int n_sub, int clip,
                                                      double* u_log, double* __restrict__ x_log, const double* __restrict__ th,
                                                      const double* __restrict__ tsv, const int* __restrict__ tsi) {
  d_policy_run<true, true>(K, W, ok, uprev, k0, n, x, v, n_sub, clip, u_log, x_log, th, tsv, tsi);
}

}  // namespace ltompc
