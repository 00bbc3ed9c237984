// adjoint.h — adjoint sensitivities (ltompc_get_adjoint): the gradient of a scalar loss L(X, U) of the predicted
// trajectory w.r.t. p = (x0, u_prev) and the 16 parameters theta, from its cotangents gX = dL/dX (N+1 x 8), gU = dL/dU (N x 2):
//     grad_p[j] = <gX, dX_dp[.., j]> + <gU, dU_dp[.., j]>,     grad_theta[j] = <gX, dX_dth[.., j]> + <gU, dU_dth[.., j]>
// with the Jacobians of sensitivity.h and param_sensitivity.h (same barrier problem, final iterate, delta_w = 0), without
// forming them.  A forward column j is the minimiser w_j of the stage QP with gradient g_j = (q, qx, r, dJdu, dJdv) and
// dynamics offset b_j; the KKT matrix is symmetric, so with (a, e; nu) the minimiser and the costates of the SAME QP with the
// cotangent as gradient, no offset and a_0 = v_0 = 0,
//     <(gX, gU), w_j> = <(a, e), g_j> + <nu, b_j>,     nu_{k+1} = P_{k+1} a_{k+1} + Pxv_{k+1} e_k + pp_{k+1}
// (costate of x_{k+1} = A x_k + B u_k + b: the gradient of the cost-to-go at the adjoint trajectory), and the (x0, u_prev)
// columns are the stage-0 vectors of the backward recursion: grad_x0 = pp_0 (gX_0 enters as the stage-0 q), grad_uprev = pv_0.
//
//   k_adj_sweep        8 instances x 8 lanes per wavefront (lane (g, i) owns row i), one cotangent: the backward recursion of
//                      d_psens_sweep with q := gX_k, r := gU_k, b := 0 and no dJ terms on the stored K, Kv, P, Pxv (Huu with
//                      the same expression and guard), pp_{k+1} and kff_k of every stage into the pass's AJ planes; then the
//                      forward pass a_{k+1} = A a_k + B e_k, e_k = K a_k + Kv e_{k-1} + kff_k, the costates, and the 16 sums
//                      over the PV planes of k_psens_cond (gth != nullptr), reduced over the 8 rows at the end
//   k_adj_sweep_pi     the same with r_du from the instance's row (W.TH; PV from k_psens_cond_pi)
//   k_prediction_dev   thread = (node k, instance b): X, U planes -> row-major arrays in the caller's order through orig
//
// The pass reads the iterate, the pass buffers of sensitivity.h and the PV planes, and writes only buffers of its own.
#pragma once
#include "param_sensitivity.h"

namespace ltompc {

constexpr int ADJ_NP = SENS_NP;  // grad_p: x0[0..7], u_prev[0..1]
// AJ planes [field][k][Bp] written by the backward half at stage k and read back by the same lanes in the forward half:
// pp_{k+1} (8, row i by lane i), kff_k (2, by lanes 0 and 1)
constexpr int AJ_pp = 0, AJ_kff = 8, AJ_NF = 10;

struct AdjLds {
  double x[8][8];  // [g][row]: pp, then a_k, exchanged between the rows
};

// TH: with the theta sums (PV, uprev, gth used).  Cotangents gX [B][N+1][8], gU [B][N][2] in the caller's order, either may be
// nullptr (zeros).  gp [B][10], gth [B][16] in the caller's order, exactly 0 where ok_in is 0.
template <bool TH, bool PI>
__device__ __forceinline__ void d_adj_sweep(const Work& W, AdjLds& L, const double r0, const double r1, const double* __restrict__ uprev,
                                            const double* __restrict__ PV, const int* __restrict__ ok_in, const double* __restrict__ gX,
                                            const double* __restrict__ gU, double* __restrict__ AJ, double* __restrict__ gp,
                                            double* __restrict__ gth) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < W.B;
  const int b = valid ? j : 0;
  const int N = W.N;
  const size_t ob = W.orig[b];
  const bool okk = ok_in[ob] != 0;
  const gptr<const double> th = PI ? static_cast<const WorkPI&>(W).TH : nullptr;  // (PI: r_du of the instance's row, r0 / r1 unused)
  const double r2[2] = {2.0 * (PI ? th[(size_t)14 * W.Bp + ob] : r0), 2.0 * (PI ? th[(size_t)15 * W.Bp + ob] : r1)};
  const double* gXb = gX ? gX + ob * (size_t)(N + 1) * 8 + i : nullptr;  // row i of this instance's cotangent blocks
  const double* gUb = gU ? gU + ob * (size_t)N * 2 : nullptr;
  // ---- backward recursion of the one vector (d_psens_sweep with q := gX_k, r := gU_k, b := 0)
  double pp = gXb ? gXb[(size_t)N * 8] : 0.0, pv[2] = {0.0, 0.0};
#pragma unroll 1
  for (int k = N - 1; k >= 0; k--) {
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
        for (int d = 0; d < 2; d++) {
          const double pvv = ((c == d) ? r2[c] : 0.0) - r2[c] * PG(W.RC, RC_Kv + c * 2 + d, kn, RC_NF);
          Pvv[c * 2 + d] = k + 1 < N ? pvv : 0.0;
        }
    }
    const double Rm[3] = {PG(W.QP, QP_R + 0, k, QP_NF), PG(W.QP, QP_R + 1, k, QP_NF), PG(W.QP, QP_R + 2, k, QP_NF)};
    const double gx0 = gXb ? gXb[(size_t)k * 8] : 0.0;
    const double gu0 = gUb ? gUb[(size_t)k * 2] : 0.0, gu1 = gUb ? gUb[(size_t)k * 2 + 1] : 0.0;
    // Huu (the same number in the 8 lanes of an instance): d_psens_sweep's expression and guard
    double PB[2] = {0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 8; l++) PB[0] += Prow[l] * Bm[l * 2], PB[1] += Prow[l] * Bm[l * 2 + 1];
    double Huu[4];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int d = 0; d < 2; d++)
        Huu[c * 2 + d] = Rm[sidx(c, d)] + Pvv[c * 2 + d] +
                         grp_sum(Bm[i * 2 + c] * PB[d] + Bm[i * 2 + c] * Xi[d] + Xi[c] * Bm[i * 2 + d]);
    Huu[0] += r2[0], Huu[3] += r2[1];
    double det = Huu[0] * Huu[3] - Huu[1] * Huu[2];
    const bool bad = !(Huu[0] > 0.0) | !(det > 1e-14 * Huu[0] * Huu[3]) | !isfinite(det);
    det = bad ? 1.0 : det;  // (ok = 0 for such an instance: keep the lock-step arithmetic finite)
    Huu[0] = bad ? 1.0 : Huu[0], Huu[3] = bad ? 1.0 : Huu[3], Huu[1] = bad ? 0.0 : Huu[1], Huu[2] = bad ? 0.0 : Huu[2];
    const double idet = 1.0 / det;
    const double Hi[4] = {Huu[3] * idet, -Huu[1] * idet, -Huu[2] * idet, Huu[0] * idet};
    // pp_{k+1}: kept for the costates (the forward half: TH only), and exchanged between the rows for A^T pp
    if (TH && valid) PL(AJ, AJ_pp + i, k, N) = pp;
    WAVE_SYNC();
    L.x[g][i] = pp;
    WAVE_SYNC();
    const double gu[2] = {gu0 + pv[0] + grp_sum(Bm[i * 2] * pp), gu1 + pv[1] + grp_sum(Bm[i * 2 + 1] * pp)};
    double gx = gx0;
#pragma unroll
    for (int l = 0; l < 8; l++) gx += Ac[l] * L.x[g][l];
    const double kf0 = -(Hi[0] * gu[0] + Hi[1] * gu[1]), kf1 = -(Hi[2] * gu[0] + Hi[3] * gu[1]);
    pp = gx + Kc[0] * gu[0] + Kc[1] * gu[1];
    pv[0] = -r2[0] * kf0, pv[1] = -r2[1] * kf1;
    if (TH && valid && i < 2) PL(AJ, AJ_kff + i, k, N) = i == 0 ? kf0 : kf1;
  }
  // the (x0, u_prev) columns: the stage-0 vectors
  if (valid && gp) {
    gp[ob * ADJ_NP + i] = okk ? pp : 0.0;
    if (i < 2) gp[ob * ADJ_NP + 8 + i] = okk ? (i == 0 ? pv[0] : pv[1]) : 0.0;
  }
  if constexpr (!TH) return;
  // ---- forward pass, costates and the 16 sums (lane i: its row's share, reduced at the end)
  double S[PS_NT];
#pragma unroll
  for (int c = 0; c < PS_NT; c++) S[c] = 0.0;
  double a = 0.0, ev[2] = {0.0, 0.0};
  WAVE_SYNC();
  L.x[g][i] = 0.0;
  WAVE_SYNC();
#pragma unroll 1
  for (int k = 0; k < N; k++) {
    double Ar[8], Prow[8];
#pragma unroll
    for (int l = 0; l < 8; l++) Ar[l] = PG(W.QP, QP_A + i * 8 + l, k, QP_NF), Prow[l] = PG(W.RC, RC_P + sidx(i, l), k + 1, RC_NF);
    const double Bi[2] = {PG(W.QP, QP_B + i * 2, k, QP_NF), PG(W.QP, QP_B + i * 2 + 1, k, QP_NF)};
    const double Kc[2] = {PG(W.RC, RC_K + i, k, RC_NF), PG(W.RC, RC_K + 8 + i, k, RC_NF)};
    const double Xi[2] = {PG(W.RC, RC_Pxv + i * 2, k + 1, RC_NF), PG(W.RC, RC_Pxv + i * 2 + 1, k + 1, RC_NF)};
    double Kv[4];
#pragma unroll
    for (int l = 0; l < 4; l++) Kv[l] = PG(W.RC, RC_Kv + l, k, RC_NF);
    const double kfo = PL(AJ, AJ_kff + (i & 1), k, N);  // (lanes 0 and 1 wrote kff_k and read their own)
    const double kf[2] = {i == 0 ? kfo : 0.0, i == 1 ? kfo : 0.0};
    const double ppn = PL(AJ, AJ_pp + i, k, N);
    // this slot's PV words of row i: q, b, qx of the dynamics columns (r: rows 0, 1), qx of the cost columns
    double vq[PS_NDYN], vb[PS_NDYN], vqx[PS_NDYN + 3], vr[PS_NDYN];
#pragma unroll
    for (int c = 0; c < PS_NDYN; c++) {
      vq[c] = PL(PV, pv_base(c) + PV_q + i, k, N), vb[c] = PL(PV, pv_base(c) + PV_b + i, k, N);
      vr[c] = PL(PV, pv_base(c) + PV_r + (i & 1), k, N);
    }
#pragma unroll
    for (int c = 0; c < PS_NDYN + 3; c++) vqx[c] = PL(PV, pv_qx(c) + i, k, N);
    double du;  // (u_k - u_{k-1})_c in lane c (lanes >= 2: unused)
    {
      const int c = i & 1, km = k > 0 ? k - 1 : 0;
      const double v = k > 0 ? PL(W.U, c, km, N) : uprev[ob * 2 + c];
      du = PL(W.U, c, k, N) - v;
    }
    const double e[2] = {grp_sum(Kc[0] * a + kf[0]) + Kv[0] * ev[0] + Kv[1] * ev[1],
                         grp_sum(Kc[1] * a + kf[1]) + Kv[2] * ev[0] + Kv[3] * ev[1]};
    double an = Bi[0] * e[0] + Bi[1] * e[1];
#pragma unroll
    for (int l = 0; l < 8; l++) an += Ar[l] * L.x[g][l];
    WAVE_SYNC();
    L.x[g][i] = an;
    WAVE_SYNC();
    double nu = ppn + Xi[0] * e[0] + Xi[1] * e[1];
#pragma unroll
    for (int l = 0; l < 8; l++) nu += Prow[l] * L.x[g][l];
    const double ei = i == 0 ? e[0] : (i == 1 ? e[1] : 0.0);  // (lanes 0 and 1 add e_k . r once)
#pragma unroll
    for (int c = 0; c < PS_NDYN; c++) S[c] += a * vq[c] + an * vqx[c] + nu * vb[c] + ei * vr[c];
#pragma unroll
    for (int c = PS_NDYN; c < PS_NDYN + 3; c++) S[c] += an * vqx[c];
    S[14] += i == 0 ? 2.0 * du * (e[0] - ev[0]) : 0.0;
    S[15] += i == 1 ? 2.0 * du * (e[1] - ev[1]) : 0.0;
    a = an, ev[0] = e[0], ev[1] = e[1];
  }
#pragma unroll
  for (int c = 0; c < PS_NT; c++) {
    const double s = grp_sum(S[c]);
    if (valid && gth && i == (c & 7)) gth[ob * PS_NT + c] = okk ? s : 0.0;
  }
}

// W: the pass's Work descriptor (QP, RC: the stored factorisation; U, orig: the solver's); uprev: k_psens_keep_uprev's; PV:
// k_psens_cond's planes; gth == nullptr: grad_p only (PV, uprev not read)
__global__ void __launch_bounds__(64) k_adj_sweep(Work W, double r0, double r1, const double* __restrict__ uprev, const double* __restrict__ PV,
                                                  const int* __restrict__ ok_in, const double* __restrict__ gX, const double* __restrict__ gU,
                                                  double* __restrict__ AJ, double* __restrict__ gp, double* __restrict__ gth) {
  __shared__ AdjLds L;
  if (gth) d_adj_sweep<true, false>(W, L, r0, r1, uprev, PV, ok_in, gX, gU, AJ, gp, gth);
  else d_adj_sweep<false, false>(W, L, r0, r1, uprev, PV, ok_in, gX, gU, AJ, gp, gth);
}
// with per-instance r_du (W.TH)
__global__ void __launch_bounds__(64) k_adj_sweep_pi(WorkPI W, const double* __restrict__ uprev, const double* __restrict__ PV,
                                                     const int* __restrict__ ok_in, const double* __restrict__ gX, const double* __restrict__ gU,
                                                     double* __restrict__ AJ, double* __restrict__ gp, double* __restrict__ gth) {
  __shared__ AdjLds L;
  if (gth) d_adj_sweep<true, true>(W, L, 0.0, 0.0, uprev, PV, ok_in, gX, gU, AJ, gp, gth);
  else d_adj_sweep<false, true>(W, L, 0.0, 0.0, uprev, PV, ok_in, gX, gU, AJ, gp, gth);
}

// The prediction of the last solve as row-major device arrays in the caller's order: Xo [B][N+1][8], Uo [B][N][2] (either may
// be nullptr).  Reads the planes where the instances are (orig: slot -> caller's index): the packed order stays as it is.
__global__ void __launch_bounds__(256) k_prediction_dev(Work W, double* __restrict__ Xo, double* __restrict__ Uo) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)(tid % W.Bp), k = (int)(tid / W.Bp);
  const int N = W.N;
  if (k > N || b >= W.B) return;
  const size_t ob = W.orig[b];
  if (Xo) {
#pragma unroll
    for (int i = 0; i < 8; i++) Xo[(ob * (N + 1) + k) * 8 + i] = PL(W.X, i, k, N + 1);
  }
  if (Uo && k < N) {
#pragma unroll
    for (int c = 0; c < 2; c++) Uo[(ob * N + k) * 2 + c] = PL(W.U, c, k, N);
  }
}

}  // namespace ltompc
