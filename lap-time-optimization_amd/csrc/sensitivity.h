// sensitivity.h — parametric sensitivities of the solution w.r.t. p = (x0[0..7], u_prev[0..1]) (ltompc_get_sensitivities,
// DESIGN.md §9).  At the final iterate of a converged solve the barrier KKT system is differentiated (implicit-function
// theorem, as in sIPOPT): with delta_w = 0 its Riccati factorisation gives, per stage, the gains of
//     dU_k = K_k dX_k + Kv_k dV_k,   dX_{k+1} = A_k dX_k + B_k dU_k,   dV_{k+1} = dU_k,   dX_0 = [I | 0], dV_0 = [0 | I],
// so that du0/dx0 = K_0 and du0/du_prev = Kv_0.  Three kernels, run once over the whole batch on request:
//
//   k_sens_eval8 / k_sens_eval  the evaluation kernels' device functions (d_eval8 / d_eval, the handle's instantiation) at
//                               the final iterate, into the pass's own stage-QP / residual buffers
//   k_sens_riccati8             d_riccati8<true>: the backward sweep of k_riccati8 without its head, delta_w = 0, one sweep;
//                               records the inertia test and K_k, Kv_k into the pass's own Riccati buffer
//   k_sens_forward              the 10 directions through the gains, 8 lanes per instance (lane (g, i): row i of dX_k, the
//                               10 columns in registers); ok, margin, and the outputs in the caller's order (orig)
//
// The pass reads the iterate, st, si and the packing, and writes only buffers of its own (Ws below): the next make_step or
// rollout sees every bit it would have seen without it.
#pragma once
#include "eval8.h"
#include "linearise.h"
#include "riccati.h"

namespace ltompc {

constexpr int SENS_NP = 10;  // columns: x0[0..7], u_prev[0..1]

// Ws: the handle's Work with QP, RC, RS, LS -> the pass's buffers and si -> a zeroed plane set (no instance is DONE, none
// re-initialises its slacks: the evaluation functions then linearise every slot and write nothing but QP / RS / LS).
__global__ void __launch_bounds__(64) k_sens_eval8(const Consts* __restrict__ Kp, const Work* __restrict__ Wsp) {
  const Consts& K = *Kp;
  const Work& W = *Wsp;
  __shared__ E8Lds lds[8];
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int G8 = W.Bp >> 3;
  const int k = blockIdx.x / G8, j = (blockIdx.x % G8) * 8 + g;
  const bool valid = j < W.B;
  d_eval8(K, W, lds[g], i, k, valid ? j : 0, valid);  // (padding lanes shadow slot 0 read-only)
}
// the _pi kernels: with per-instance vehicle and cost parameters (W.TH)
__global__ void __launch_bounds__(64) k_sens_eval8_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wsp) {
  const Consts& K = *Kp;
  const Work& W = *Wsp;
  __shared__ E8Lds lds[8];
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int G8 = W.Bp >> 3;
  const int k = blockIdx.x / G8, j = (blockIdx.x % G8) * 8 + g;
  const bool valid = j < W.B;
  d_eval8<true>(K, W, lds[g], i, k, valid ? j : 0, valid);  // (padding lanes shadow slot 0 read-only)
}

template <class BP, bool ELL>
__global__ void __launch_bounds__(64) k_sens_eval(const Consts* __restrict__ Kp, const Work* __restrict__ Wsp) {
  const Consts& K = *Kp;
  const Work& W = *Wsp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_eval<BP, ELL>(K, W, k, b, true);
}
template <class BP>
__global__ void __launch_bounds__(64) k_sens_eval_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wsp) {
  const Consts& K = *Kp;
  const Work& W = *Wsp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_eval<BP, false, true>(K, W, k, b, true);
}
// ... and per-instance table sets (W.TSV / W.TSI; the head-less sweep and the forward pass read no table: the _pi ones)
template <class BP>
__global__ void __launch_bounds__(64) k_sens_eval_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wsp) {
  const Consts& K = *Kp;
  const Work& W = *Wsp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_eval<BP, false, true, true>(K, W, k, b, true);
}

// si_solve: the solver's own si planes (read only).  An instance is differentiated when the solver's status (before the
// node-0 rule) is SOLVED or ACCEPTABLE and it was not re-initialised; inertia[b] = 1 when every stage's Huu is positive definite
// at delta_w = 0.
template <bool PI>
__device__ __forceinline__ void d_sens_riccati8(const Consts& K, const Work& Ws, RicLds& L, const int* __restrict__ si_solve,
                                                int* __restrict__ inertia) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < Ws.B;
  const int b = valid ? j : 0;
  const size_t Bp = Ws.Bp;
  const int node0 = si_solve[(size_t)SI_NODE0 * Bp + b];
  const int status = node0 ? node0 - 1 : si_solve[(size_t)SI_STATUS * Bp + b];
  const bool el = valid && (status == LTOMPC_STATUS_SOLVED || status == LTOMPC_STATUS_ACCEPTABLE) && !si_solve[(size_t)SI_REINIT * Bp + b];
  d_riccati8<true, PI>(K, Ws, L, g, i, b, valid, -1, 1, el, inertia);
}
__global__ void __launch_bounds__(64) k_sens_riccati8(Consts K, Work Ws, const int* __restrict__ si_solve, int* __restrict__ inertia) {
  __shared__ RicLds L;
  d_sens_riccati8<false>(K, Ws, L, si_solve, inertia);
}
__global__ void __launch_bounds__(64) k_sens_riccati8_pi(Consts K, WorkPI Ws, const int* __restrict__ si_solve, int* __restrict__ inertia) {
  __shared__ RicLds L;
  d_sens_riccati8<true>(K, Ws, L, si_solve, inertia);
}

// Forward propagation of the 10 directions.  Wave = 8 instances x 8 lanes; lane (g, i) carries row i of dX_k (10 columns),
// every lane of an instance the whole dV_k (2 x 10); dU_k = K_k dX_k + Kv_k dV_k is a sum over the rows (grp_sum), dX_{k+1}
// needs the whole dX_k (exchanged through LDS).  Stage k + 1's 16 operands per lane are requested during stage k.
//   Pass 1 (ok_known = nullptr): du0 [B][2][10], ok [B], margin [B] in the caller's order; ok = inertia && every value of the
//   propagation finite, else every output of the instance is 0.
//   Pass 2 (ok_known = pass 1's ok): the trajectories dX [B][N+1][8][10], dU [B][N][2][10] (zeros where not ok).
__global__ void __launch_bounds__(64) k_sens_forward(Work W, const int* __restrict__ inertia, int ni, double* __restrict__ du0,
                                                     int* __restrict__ ok_out, double* __restrict__ margin, double* __restrict__ dXo,
                                                     double* __restrict__ dUo, const int* __restrict__ ok_known) {
  __shared__ double xs[8][8 * SENS_NP];  // [g][row * 10 + col]
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < W.B;
  const int b = valid ? j : 0;
  const int N = W.N;
  const size_t ob = W.orig[b];
  const bool okk = ok_known ? ok_known[ob] != 0 : true;  // (pass 2: zeros for the instances pass 1 rejected)
  double dx[SENS_NP], dv[2][SENS_NP], du[2][SENS_NP];
#pragma unroll
  for (int c = 0; c < SENS_NP; c++) dx[c] = (c == i) ? 1.0 : 0.0, dv[0][c] = (c == 8) ? 1.0 : 0.0, dv[1][c] = (c == 9) ? 1.0 : 0.0;
  if (valid && dXo) {
#pragma unroll
    for (int c = 0; c < SENS_NP; c++) dXo[(ob * (N + 1) * 8 + i) * SENS_NP + c] = okk ? dx[c] : 0.0;
  }
  double A[8], Bi[2], Kc[2], Kv[4];  // stage k: row i of A_k, B_k; column i of K_k; Kv_k
  auto load = [&](const int k, double* a, double* bb, double* kc, double* kv) {
#pragma unroll
    for (int l = 0; l < 8; l++) a[l] = PG(W.QP, QP_A + i * 8 + l, k, QP_NF);
    bb[0] = PG(W.QP, QP_B + i * 2, k, QP_NF), bb[1] = PG(W.QP, QP_B + i * 2 + 1, k, QP_NF);
    kc[0] = PG(W.RC, RC_K + i, k, RC_NF), kc[1] = PG(W.RC, RC_K + 8 + i, k, RC_NF);
#pragma unroll
    for (int l = 0; l < 4; l++) kv[l] = PG(W.RC, RC_Kv + l, k, RC_NF);
  };
  load(0, A, Bi, Kc, Kv);
  bool fin = true;
#pragma unroll 1
  for (int k = 0; k < N; k++) {
    double An[8], Bn[2], Kcn[2], Kvn[4];
    load(k + 1 < N ? k + 1 : k, An, Bn, Kcn, Kvn);
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int col = 0; col < SENS_NP; col++)
        du[c][col] = grp_sum(Kc[c] * dx[col]) + Kv[c * 2] * dv[0][col] + Kv[c * 2 + 1] * dv[1][col];
    WAVE_SYNC();
#pragma unroll
    for (int col = 0; col < SENS_NP; col++) xs[g][i * SENS_NP + col] = dx[col];
    WAVE_SYNC();
#pragma unroll
    for (int col = 0; col < SENS_NP; col++) {
      double s = Bi[0] * du[0][col] + Bi[1] * du[1][col];
#pragma unroll
      for (int l = 0; l < 8; l++) s += A[l] * xs[g][l * SENS_NP + col];
      dx[col] = s;
      fin = fin && isfinite(s) && isfinite(du[0][col]) && isfinite(du[1][col]);
    }
#pragma unroll
    for (int col = 0; col < SENS_NP; col++) dv[0][col] = du[0][col], dv[1][col] = du[1][col];
    if (valid) {
      if (k == 0 && du0 && i < 2) {
#pragma unroll
        for (int col = 0; col < SENS_NP; col++) du0[(ob * 2 + i) * SENS_NP + col] = i == 0 ? du[0][col] : du[1][col];
      }
      if (dUo && i < 2) {
#pragma unroll
        for (int col = 0; col < SENS_NP; col++) dUo[((ob * N + k) * 2 + i) * SENS_NP + col] = okk ? (i == 0 ? du[0][col] : du[1][col]) : 0.0;
      }
      if (dXo) {
#pragma unroll
        for (int col = 0; col < SENS_NP; col++) dXo[((ob * (N + 1) + k + 1) * 8 + i) * SENS_NP + col] = okk ? dx[col] : 0.0;
      }
    }
#pragma unroll
    for (int l = 0; l < 8; l++) A[l] = An[l];
    Bi[0] = Bn[0], Bi[1] = Bn[1], Kc[0] = Kcn[0], Kc[1] = Kcn[1];
#pragma unroll
    for (int l = 0; l < 4; l++) Kv[l] = Kvn[l];
  }
  if (ok_known) return;
  // margin = min over the (slack, multiplier) pairs of max(t, nu): lane i takes the pairs m = i, i + 8, ...
  double mg = INFINITY;
#pragma unroll 1
  for (int k = 0; k < N; k++)
    for (int m = i; m < ni; m += 8) mg = fmin(mg, fmax(PL(W.T, m, k, N), PL(W.NU, m, k, N)));
  mg = grp_min(mg);
  const bool ok = inertia[b] != 0 && grp_min(fin ? 1.0 : 0.0) > 0.0;
  if (!valid) return;
  if (i == 0) ok_out[ob] = ok ? 1 : 0, margin[ob] = ok ? mg : 0.0;
  if (!ok && du0 && i < 2) {
#pragma unroll
    for (int col = 0; col < SENS_NP; col++) du0[(ob * 2 + i) * SENS_NP + col] = 0.0;
  }
}

}  // namespace ltompc
