// jvp.h — directional (forward-mode) sensitivities (ltompc_get_jvp): the Jacobian-vector product of the predicted
// trajectory with one direction dp = (d x0, d u_prev) and dtheta of the 16 parameters,
//     tX[k,i] = sum_j dX_dp[k,i,j] dp[j] + sum_j dX_dth[k,i,j] dtheta[j],     tU likewise,
// with the Jacobians of sensitivity.h and param_sensitivity.h (same barrier problem, final iterate, delta_w = 0), without forming
// them.  The linearised KKT system is linear in its right-hand side, so the 26 columns collapse into ONE: the stage vectors
// (q, r, b, qx) of the direction are the dtheta-weighted sums of k_psens_cond's planes, its dJdu / dJdv terms those of the two
// r_du columns weighted by dtheta[14], dtheta[15], and (dp[0..7], dp[8..9]) are the initial values (tX_0, tV_0) of the forward pass
//     tU_k = K_k tX_k + Kv_k tV_k + kff_k,   tX_{k+1} = A_k tX_k + B_k tU_k + b_k,   tV_{k+1} = tU_k.
//
//   k_jvp_sweep        8 instances x 8 lanes per wavefront (lane (g, i) owns row i), one direction: with dtheta the backward
//                      recursion of d_psens_sweep for the one weighted vector on the stored K, Kv, P, Pxv (Huu with the same
//                      expression and guard), kff_k of every stage into the pass's JV planes; then the forward pass above.
//                      Without dtheta (a wave-uniform branch): kff = b = 0, no backward half, PV and uprev not read.
//   k_jvp_sweep_pi     the same with r_du from the instance's row (W.TH; PV from k_psens_cond_pi)
//   k_set_uprev        the previous input of the next solve from a row-major array in the caller's order (ltompc_set_u_prev)
//
// The pass reads the iterate, the pass buffers of sensitivity.h and the PV planes, and writes only buffers of its own.
#pragma once
#include "param_sensitivity.h"

namespace ltompc {

constexpr int JVP_NP = SENS_NP;  // dp: x0[0..7], u_prev[0..1]
// JV planes [c][k][Bp]: kff_k, written by lanes 0 and 1 of an instance in the backward half and read back, plane i & 1, by all 8
// lanes of the instance in the forward half (one unconditional load; only lanes 0 and 1, which read their own word, use it)
constexpr int JV_NF = 2;

struct JvpLds {
  double x[8][8];  // [g][row]: b, Pb, then tX_k, exchanged between the rows
};

// TH: with dtheta (PV, uprev, JV used).  Directions dp [B][10], dth [B][16] in the caller's order; dp may be nullptr (zeros), dth
// is not nullptr when TH.  tX [B][N+1][8], tU [B][N][2] in the caller's order (either may be nullptr), exactly 0 where ok_in is 0.
template <bool TH, bool PI>
__device__ __forceinline__ void d_jvp_sweep(const Work& W, JvpLds& L, const double r0, const double r1, const double* __restrict__ uprev,
                                            const double* __restrict__ PV, const int* __restrict__ ok_in, const double* __restrict__ dp,
                                            const double* __restrict__ dth, double* __restrict__ JV, double* __restrict__ tX,
                                            double* __restrict__ tU) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < W.B;
  const int b = valid ? j : 0;
  const int N = W.N;
  const size_t ob = W.orig[b];
  const bool okk = ok_in[ob] != 0;
  double d[PS_NT];  // the direction over theta (the same 16 numbers in the 8 lanes of an instance)
#pragma unroll
  for (int c = 0; c < PS_NT; c++) d[c] = TH ? dth[ob * PS_NT + c] : 0.0;
  if constexpr (TH) {
    const gptr<const double> th = PI ? static_cast<const WorkPI&>(W).TH : nullptr;  // (PI: r_du of the instance's row, r0 / r1 unused)
    const double r2[2] = {2.0 * (PI ? th[(size_t)14 * W.Bp + ob] : r0), 2.0 * (PI ? th[(size_t)15 * W.Bp + ob] : r1)};
    // ---- backward recursion of the one weighted vector (d_psens_sweep's, columns summed with the weights d)
    double pp = 0.0, pv[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < PS_NDYN + 3; c++) pp += d[c] * PL(PV, pv_qx(c) + i, N - 1, N);
#pragma unroll 1
    for (int k = N - 1; k >= 0; k--) {
      // the stage's loads, issued as one batch before the arithmetic
      double Prow[8], Bm[16], Xi[2], Ac[8], Kc[2], Pvv[4];
#pragma unroll
      for (int l = 0; l < 8; l++) Prow[l] = PG(W.RC, RC_P + sidx(i, l), k + 1, RC_NF), Ac[l] = PG(W.QP, QP_A + l * 8 + i, k, QP_NF);
#pragma unroll
      for (int l = 0; l < 16; l++) Bm[l] = PG(W.QP, QP_B + l, k, QP_NF);
      Xi[0] = PG(W.RC, RC_Pxv + i * 2, k + 1, RC_NF), Xi[1] = PG(W.RC, RC_Pxv + i * 2 + 1, k + 1, RC_NF);
      Kc[0] = PG(W.RC, RC_K + i, k, RC_NF), Kc[1] = PG(W.RC, RC_K + 8 + i, k, RC_NF);
      {
        const int kn = k + 1 < N ? k + 1 : k;  // (stage N: no Delta-u coupling beyond the horizon, Pvv = 0)
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
          for (int e = 0; e < 2; e++) {
            const double pvv = ((c == e) ? r2[c] : 0.0) - r2[c] * PG(W.RC, RC_Kv + c * 2 + e, kn, RC_NF);
            Pvv[c * 2 + e] = k + 1 < N ? pvv : 0.0;
          }
      }
      const double Rm[3] = {PG(W.QP, QP_R + 0, k, QP_NF), PG(W.QP, QP_R + 1, k, QP_NF), PG(W.QP, QP_R + 2, k, QP_NF)};
      const int km = k > 0 ? k - 1 : 0;
      double du[2];
      {
        const double uk0 = PL(W.U, 0, k, N), uk1 = PL(W.U, 1, k, N);
        const double v0 = k > 0 ? PL(W.U, 0, km, N) : uprev[ob * 2], v1 = k > 0 ? PL(W.U, 1, km, N) : uprev[ob * 2 + 1];
        du[0] = uk0 - v0, du[1] = uk1 - v1;
      }
      // this slot's PV words of row i (r: rows 0, 1; qx: the node block of x_k, slot k - 1, x_0 has none), weighted
      double bi = 0.0, gx = 0.0, ri = 0.0, qxs = 0.0;
#pragma unroll
      for (int c = 0; c < PS_NDYN; c++) {
        bi += d[c] * PL(PV, pv_base(c) + PV_b + i, k, N), gx += d[c] * PL(PV, pv_base(c) + PV_q + i, k, N);
        ri += d[c] * PL(PV, pv_base(c) + PV_r + (i & 1), k, N);
      }
#pragma unroll
      for (int c = 0; c < PS_NDYN + 3; c++) qxs += d[c] * PL(PV, pv_qx(c) + i, km, N);
      gx += k > 0 ? qxs : 0.0;
      // Huu (the same number in the 8 lanes of an instance): d_psens_sweep's expression and guard
      double PB[2] = {0.0, 0.0};
#pragma unroll
      for (int l = 0; l < 8; l++) PB[0] += Prow[l] * Bm[l * 2], PB[1] += Prow[l] * Bm[l * 2 + 1];
      double Huu[4];
#pragma unroll
      for (int c = 0; c < 2; c++)
#pragma unroll
        for (int e = 0; e < 2; e++)
          Huu[c * 2 + e] = Rm[sidx(c, e)] + Pvv[c * 2 + e] +
                           grp_sum(Bm[i * 2 + c] * PB[e] + Bm[i * 2 + c] * Xi[e] + Xi[c] * Bm[i * 2 + e]);
      Huu[0] += r2[0], Huu[3] += r2[1];
      double det = Huu[0] * Huu[3] - Huu[1] * Huu[2];
      const bool bad = !(Huu[0] > 0.0) | !(det > 1e-14 * Huu[0] * Huu[3]) | !isfinite(det);
      det = bad ? 1.0 : det;  // (ok = 0 for such an instance: keep the lock-step arithmetic finite)
      Huu[0] = bad ? 1.0 : Huu[0], Huu[3] = bad ? 1.0 : Huu[3], Huu[1] = bad ? 0.0 : Huu[1], Huu[2] = bad ? 0.0 : Huu[2];
      const double idet = 1.0 / det;
      const double Hi[4] = {Huu[3] * idet, -Huu[1] * idet, -Huu[2] * idet, Huu[0] * idet};
      // row i of b, then of Pb = pp + P b, exchanged through LDS
      WAVE_SYNC();
      L.x[g][i] = bi;
      WAVE_SYNC();
      double Pb = pp;
#pragma unroll
      for (int l = 0; l < 8; l++) Pb += Prow[l] * L.x[g][l];
      WAVE_SYNC();
      L.x[g][i] = Pb;
      WAVE_SYNC();
      double gu[2];
#pragma unroll
      for (int e = 0; e < 2; e++) gu[e] = grp_sum(Bm[i * 2 + e] * Pb + Xi[e] * bi + (i == e ? ri : 0.0)) + pv[e];  // (lane e adds r_e once)
      gu[0] += d[14] * (2.0 * du[0]), gu[1] += d[15] * (2.0 * du[1]);
#pragma unroll
      for (int l = 0; l < 8; l++) gx += Ac[l] * L.x[g][l];
      const double kf0 = -(Hi[0] * gu[0] + Hi[1] * gu[1]), kf1 = -(Hi[2] * gu[0] + Hi[3] * gu[1]);
      pp = gx + Kc[0] * gu[0] + Kc[1] * gu[1];
      pv[0] = d[14] * (-2.0 * du[0]) - r2[0] * kf0;
      pv[1] = d[15] * (-2.0 * du[1]) - r2[1] * kf1;
      if (valid && i < 2) PL(JV, i, k, N) = i == 0 ? kf0 : kf1;
    }
    WAVE_SYNC();
  }
  // ---- forward pass from (tX_0, tV_0) = (dp[0..7], dp[8..9])
  double tx = dp ? dp[ob * JVP_NP + i] : 0.0;
  double tv[2] = {dp ? dp[ob * JVP_NP + 8] : 0.0, dp ? dp[ob * JVP_NP + 9] : 0.0};
  if (valid && tX) tX[ob * (size_t)(N + 1) * 8 + i] = okk ? tx : 0.0;
#pragma unroll 1
  for (int k = 0; k < N; k++) {
    double Ar[8], Kv[4];
#pragma unroll
    for (int l = 0; l < 8; l++) Ar[l] = PG(W.QP, QP_A + i * 8 + l, k, QP_NF);
    const double Bi[2] = {PG(W.QP, QP_B + i * 2, k, QP_NF), PG(W.QP, QP_B + i * 2 + 1, k, QP_NF)};
    const double Kc[2] = {PG(W.RC, RC_K + i, k, RC_NF), PG(W.RC, RC_K + 8 + i, k, RC_NF)};
#pragma unroll
    for (int l = 0; l < 4; l++) Kv[l] = PG(W.RC, RC_Kv + l, k, RC_NF);
    double kfo = 0.0, bi = 0.0;
    if constexpr (TH) {
      // lanes 0 and 1 wrote kff_k and read their own word; lanes 2..7 load the same two words and drop them, and padding lanes
      // (b = 0, nothing stored) load slot 0's, which its own wavefront may be writing: the value is never used there
      kfo = PL(JV, i & 1, k, N);
#pragma unroll
      for (int c = 0; c < PS_NDYN; c++) bi += d[c] * PL(PV, pv_base(c) + PV_b + i, k, N);
    }
    const double kf[2] = {i == 0 ? kfo : 0.0, i == 1 ? kfo : 0.0};
    const double u[2] = {grp_sum(Kc[0] * tx + kf[0]) + Kv[0] * tv[0] + Kv[1] * tv[1],
                         grp_sum(Kc[1] * tx + kf[1]) + Kv[2] * tv[0] + Kv[3] * tv[1]};
    WAVE_SYNC();
    L.x[g][i] = tx;
    WAVE_SYNC();
    double xn = bi + Bi[0] * u[0] + Bi[1] * u[1];
#pragma unroll
    for (int l = 0; l < 8; l++) xn += Ar[l] * L.x[g][l];
    tx = xn, tv[0] = u[0], tv[1] = u[1];
    if (valid && tU && i < 2) tU[(ob * N + k) * 2 + i] = okk ? (i == 0 ? u[0] : u[1]) : 0.0;
    if (valid && tX) tX[(ob * (N + 1) + k + 1) * 8 + i] = okk ? tx : 0.0;
  }
}

// W: the pass's Work descriptor (QP, RC: the stored factorisation; U, orig: the solver's); uprev: k_psens_keep_uprev's; PV:
// k_psens_cond's planes; dth == nullptr: the dp part only (PV, uprev, JV not touched)
__global__ void __launch_bounds__(64) k_jvp_sweep(Work W, double r0, double r1, const double* __restrict__ uprev, const double* __restrict__ PV,
                                                  const int* __restrict__ ok_in, const double* __restrict__ dp, const double* __restrict__ dth,
                                                  double* __restrict__ JV, double* __restrict__ tX, double* __restrict__ tU) {
  __shared__ JvpLds L;
  if (dth) d_jvp_sweep<true, false>(W, L, r0, r1, uprev, PV, ok_in, dp, dth, JV, tX, tU);
  else d_jvp_sweep<false, false>(W, L, r0, r1, uprev, PV, ok_in, dp, dth, JV, tX, tU);
}
// with per-instance r_du (W.TH)
__global__ void __launch_bounds__(64) k_jvp_sweep_pi(WorkPI W, const double* __restrict__ uprev, const double* __restrict__ PV,
                                                     const int* __restrict__ ok_in, const double* __restrict__ dp, const double* __restrict__ dth,
                                                     double* __restrict__ JV, double* __restrict__ tX, double* __restrict__ tU) {
  __shared__ JvpLds L;
  if (dth) d_jvp_sweep<true, true>(W, L, 0.0, 0.0, uprev, PV, ok_in, dp, dth, JV, tX, tU);
  else d_jvp_sweep<false, true>(W, L, 0.0, 0.0, uprev, PV, ok_in, dp, dth, JV, tX, tU);
}

// u_prev of the next solve from a row-major B x 2 array in the caller's order (orig: slot -> caller's index when the instances
// are packed, else nullptr)
__global__ void k_set_uprev(Work W, const double* __restrict__ uprev_rm, const int* __restrict__ orig) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  const size_t r = orig ? orig[b] : b;
  W.uprev[b] = uprev_rm[r * 2], W.uprev[(size_t)W.Bp + b] = uprev_rm[r * 2 + 1];
}

}  // namespace ltompc
