// table_sensitivity.h — adjoint gradients w.r.t. the track tables (ltompc_get_adjoint_tables): the gradient of a
// scalar loss L(X, U) of the predicted trajectory w.r.t. the knot values y of the four value rows kappa, n_left, n_right, v_ref,
// from its cotangents gX, gU.  Same problem as sensitivity.h / adjoint.h (the barrier problem at the final iterate, delta_w = 0,
// the slot's ST_EPS), same instances and ok.
//
// The tables enter slot (k, b) through ten scalars, the value and the slope that the look-ups returned (TS_* below): kappa at
// s(c_k) and at s(x_{k+1}) (the dynamics rows s and mu of both collocation equations and the stationarity rows of c_k and
// x_{k+1}), and n_left, n_right, v_ref at s(x_{k+1}) for k + 1 <= N - 1 (the node block: track rows and stage cost).  Each scalar
// has a condensed column (q, b, qx, r) like a column of param_sensitivity.h, and its gradient is adjoint.h's contraction without
// the sum over k,
//     a_k . q + a_{k+1} . qx + e_k . r + nu_{k+1} . b
// with (a, e; nu) the adjoint trajectory and costates of the cotangent.  Value and slope are linear in the knot values,
// sum_j y_j phi_j(s) and sum_j y_j phi_j'(s), with or without the rounding patch of lut_eval, so the chain rule to the knots is
// exact and touches four knots at most (lut_basis).
//
//   k_adj_sweep_tab      d_adj_sweep's recursion (adjoint.h: the same expressions) for one cotangent, keeping the trajectory:
//                        a_{k+1}, e_k, nu_{k+1} of every stage into the pass's TJ planes (a_0 = 0)
//   k_adj_sweep_tab_pi   the same with r_du from the instance's row (W.TH)
//   k_tab_cond<BP>       thread = (interval k, instance b): E1, E2, Hc and the M8 factor by the calls d_psens_cond makes, the
//                        kappa jets in closed form, the four kappa columns condensed one at a time and contracted with the
//                        stored vectors in registers, the six node columns (qx only) likewise -> slot_grad [B][N][10] in the
//                        caller's order, exactly 0 where ok is 0.  Deterministic.
//   k_tab_cond_pi<BP>    the same with the instance's vehicle parameters in E1, E2, Hc (the kappa jets hold no vehicle parameter)
//   k_tab_scatter        thread = (look-up point, k, b): lut_basis, then atomicAdd(double) of slot_grad times the basis weights
//                        into grad_tables [4][n_table], summed over the ok instances.  The caller zeroes grad_tables.  The last
//                        bits of grad_tables depend on the order in which the adds arrive.
//   k_tab_add            dst += src: the grad_tables of one part of a split batch added to the caller's array
//
// Requires ptv = 0 and ell_penalty = 0 (the host rejects other handles).  The pass reads the iterate and the pass buffers of
// sensitivity.h and writes only buffers of its own.
#pragma once
#include "adjoint.h"

namespace ltompc {

// the ten scalars of a slot, value then slope: kappa at c_k, kappa at x_{k+1}, n_left, n_right, v_ref at x_{k+1}
enum : int { TS_KC = 0, TS_KX = 2, TS_NL = 4, TS_NR = 6, TS_VR = 8, TS_NS = 10 };
constexpr int TAB_ROWS = LTOMPC_TABLE_VALUE_ROWS;  // grad_tables rows: kappa, n_left, n_right, v_ref
// TJ planes [field][k][Bp] of the sweep, stage k: a_{k+1} (8, row i by lane i), e_k (2, by lanes 0 and 1), nu_{k+1} (8).  The
// backward half parks pp_{k+1} in the nu planes and kff_k in the e planes; the forward half reads them back, lane by lane, and
// overwrites them.
constexpr int TJ_a = 0, TJ_e = 8, TJ_nu = 10, TJ_NF = 18;

// ------------------------------------------------------------------------------------------ lut_basis
// The at most four knots i-1 .. i+2 of a look-up at s and their weights: value = sum wv[j] y[idx[j]], slope = sum ws[j] y[idx[j]]
// for every row y on `grid`, equal to lut_eval's value and slope to rounding.  The same wrap, interval estimate with the same
// fallback search, window test and patch coefficients as lut_eval (model.h), one round trip in the common case; only the grid
// is read.  At the ends of the grid a clamped index repeats its neighbour and has weight 0.
struct LutBasis {
  int idx[4];
  double wv[4], ws[4];
};
__device__ __forceinline__ void lut_basis(const double* __restrict__ grid, int n, double g0, double inv, double period, double s,
                                          double eps, LutBasis& R) {
  if (period > 0.0) s -= period * floor((s - g0) / period);
  const double fi = (s - g0) * inv;
  int i = fi <= 0.0 ? 0 : (fi >= (double)(n - 2) ? n - 2 : (int)fi);
  int im = i > 0 ? i - 1 : 0, ip = i + 2 < n ? i + 2 : n - 1;
  double gm = grid[im], gi = grid[i], gi1 = grid[i + 1], gp = grid[ip];
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(gm), "+v"(gi), "+v"(gi1), "+v"(gp));  // (all four in registers here, as in lut_eval)
#endif
  if ((i > 0 && s < gi) || (i < n - 2 && s >= gi1)) {
    while (i > 0 && s < grid[i]) --i;
    while (i < n - 2 && s >= grid[i + 1]) ++i;
    im = i > 0 ? i - 1 : 0, ip = i + 2 < n ? i + 2 : n - 1;
    gm = grid[im], gi = grid[i], gi1 = grid[i + 1], gp = grid[ip];
  }
  R.idx[0] = im, R.idx[1] = i, R.idx[2] = i + 1, R.idx[3] = ip;
  const double d = gi1 - gi, id = 1.0 / d;
  const double t = (s - gi) * id;
  R.wv[0] = 0.0, R.wv[1] = 1.0 - t, R.wv[2] = t, R.wv[3] = 0.0;
  R.ws[0] = 0.0, R.ws[1] = -id, R.ws[2] = id, R.ws[3] = 0.0;
  if (eps > 0.0) {
    int kn = -1;
    double z = 0.0, W = 0.0, sg = 0.0;
    if (i > 0) {
      double Wk = 0.5 * fmin(gi - gm, d), zz = s - gi;
      if (zz >= 0.0 && zz < Wk) kn = i, z = zz, W = Wk, sg = 1.0;
    }
    if (kn < 0 && i + 1 < n - 1) {
      double Wk = 0.5 * fmin(d, gp - gi1), zz = s - gi1;
      if (zz < 0.0 && -zz < Wk) kn = i + 1, z = zz, W = Wk, sg = -1.0;
    }
    if (kn > 0) {
      const bool left = kn == i;  // knots kn-1, kn, kn+1: entries 0, 1, 2 or 1, 2, 3
      const double ga = left ? gm : gi, gb = left ? gi : gi1, gc = left ? gi1 : gp;
      // lut_eval's coefficients a = (1 - W / RW) / (2 W), b = W - RW - a W^2 and its factors R + a z^2 + b - sg z (value) and
      // z / R + 2 a z - sg (slope), with the differences of nearly equal numbers written out (R - |z| = eps^2 / (R + |z|), ...):
      // eps << W, and a knot that only the patch reaches would otherwise get a weight with seven digits
      const double R2 = sqrt(z * z + eps * eps), RW = sqrt(W * W + eps * eps), e2 = eps * eps, az = fabs(z);
      const double a = e2 / (RW * (RW + W)) / (2.0 * W), b = -e2 / (RW + W) - a * W * W;
      const double cv = 0.5 * (e2 / (R2 + az) + a * z * z + b), cs = 0.5 * (2.0 * a * z - sg * e2 / (R2 * (R2 + az)));
      // the slope jump J = (yc - yb) / (gc - gb) - (yb - ya) / (gb - ga) over (ya, yb, yc)
      const double ia = 1.0 / (gb - ga), ic = 1.0 / (gc - gb);
      const double Ja = ia, Jb = -ic - ia, Jc = ic;
      R.wv[0] += left ? cv * Ja : 0.0, R.wv[1] += left ? cv * Jb : cv * Ja, R.wv[2] += left ? cv * Jc : cv * Jb, R.wv[3] += left ? 0.0 : cv * Jc;
      R.ws[0] += left ? cs * Ja : 0.0, R.ws[1] += left ? cs * Jb : cs * Ja, R.ws[2] += left ? cs * Jc : cs * Jb, R.ws[3] += left ? 0.0 : cs * Jc;
    }
  }
}

// ------------------------------------------------------------------------------------------ k_adj_sweep_tab
// adjoint.h's d_adj_sweep for one cotangent with the same expressions, stage by stage, but keeping the adjoint trajectory
// instead of contracting it with the PV planes.  The backward half up to Huu's inverse (operand loads, Pvv, Huu, the guard) is
// d_adj_sweep's text line for line: tests/test_table_sweep_source.py compares the two, so a fix there has to be made here too.
// Cotangents gX [B][N+1][8], gU [B][N][2] in the caller's order, either may be nullptr (zeros); gX block 0 does not enter (x0 is
// data: a_0 = 0).
template <bool PI>
__device__ __forceinline__ void d_adj_sweep_tab(const Work& W, AdjLds& L, const double r0, const double r1, const double* __restrict__ gX,
                                                const double* __restrict__ gU, double* __restrict__ TJ) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < W.B;
  const int b = valid ? j : 0;
  const int N = W.N;
  const size_t ob = W.orig[b];
  const gptr<const double> th = PI ? static_cast<const WorkPI&>(W).TH : nullptr;  // (PI: r_du of the instance's row, r0 / r1 unused)
  const double r2[2] = {2.0 * (PI ? th[(size_t)14 * W.Bp + ob] : r0), 2.0 * (PI ? th[(size_t)15 * W.Bp + ob] : r1)};
  const double* gXb = gX ? gX + ob * (size_t)(N + 1) * 8 + i : nullptr;  // row i of this instance's cotangent blocks
  const double* gUb = gU ? gU + ob * (size_t)N * 2 : nullptr;
  // ---- backward recursion of the one vector
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
    const double gx0 = gXb ? gXb[(size_t)k * 8] : 0.0;  // (k = 0: gX block 0 reaches pp_0 only, which this pass does not use)
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
    if (valid) PL(TJ, TJ_nu + i, k, N) = pp;  // pp_{k+1}, parked for the costates
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
    if (valid && i < 2) PL(TJ, TJ_e + i, k, N) = i == 0 ? kf0 : kf1;
  }
  // ---- forward pass and costates: a_{k+1} = A a_k + B e_k, e_k = K a_k + Kv e_{k-1} + kff_k, nu_{k+1} = P a_{k+1} + Pxv e_k + pp_{k+1}
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
    const double kfo = valid ? PL(TJ, TJ_e + (i & 1), k, N) : 0.0;  // (lanes 0 and 1 wrote kff_k and read their own)
    const double kf[2] = {i == 0 ? kfo : 0.0, i == 1 ? kfo : 0.0};
    const double ppn = valid ? PL(TJ, TJ_nu + i, k, N) : 0.0;
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
    if (valid) {
      PL(TJ, TJ_a + i, k, N) = an, PL(TJ, TJ_nu + i, k, N) = nu;
      if (i < 2) PL(TJ, TJ_e + i, k, N) = i == 0 ? e[0] : e[1];
    }
    a = an, ev[0] = e[0], ev[1] = e[1];
  }
}

// W: the pass's Work descriptor (QP, RC: the stored factorisation; orig: the solver's); TJ: the pass's planes [TJ_NF][N][Bp]
__global__ void __launch_bounds__(64) k_adj_sweep_tab(Work W, double r0, double r1, const double* __restrict__ gX, const double* __restrict__ gU,
                                                      double* __restrict__ TJ) {
  __shared__ AdjLds L;
  d_adj_sweep_tab<false>(W, L, r0, r1, gX, gU, TJ);
}
// with per-instance r_du (W.TH)
__global__ void __launch_bounds__(64) k_adj_sweep_tab_pi(WorkPI W, const double* __restrict__ gX, const double* __restrict__ gU,
                                                         double* __restrict__ TJ) {
  __shared__ AdjLds L;
  d_adj_sweep_tab<true>(W, L, 0.0, 0.0, gX, gU, TJ);
}

// ------------------------------------------------------------------------------------------ k_tab_cond
// The kappa jets at one point w (c_k or x_{k+1}) in closed form, from sdot = (vx cos mu - vy sin mu) / (1 - n kappa) and
// mu' = r - kappa sdot (no vehicle parameter enters): for the value column
//   fv[0], fv[1] = d(f_s, f_mu)/dkappa,   gv[m] = sum_{i in {s, mu}} lam_i d(df_i/dw_m)/dkappa over w = (s, n, mu, vx, vy)
// (df_i/ds = df_i/dkappa kappa', so its derivative holds kappa' = kp), and for the slope column only the s entry
//   gs0 = sum_i lam_i df_i/dkappa.
__device__ __forceinline__ void kappa_jet(const double* w, const double kap, const double kp, const double l0, const double l2, double* fv,
                                          double* gv, double& gs0) {
  const double n = w[1], vx = w[3], vy = w[4];
  double sm, cm;
  sincos(w[2], &sm, &cm);
  const double S = vx * cm - vy * sm, nd = vx * sm + vy * cm;
  const double g = 1.0 / (1.0 - n * kap), g2 = g * g, g3 = g2 * g;
  const double f0 = S * g, f0k = S * n * g2, f0kk = 2.0 * S * n * n * g3;
  fv[0] = f0k, fv[1] = -f0 - kap * f0k;
  // first derivatives of sdot over (n, mu, vx, vy) and their derivatives w.r.t. kappa
  const double S1[5] = {0.0, S * kap * g2, -nd * g, cm * g, -sm * g};
  const double A0[5] = {f0kk * kp, S * (1.0 + n * kap) * g3, -nd * n * g2, cm * n * g2, -sm * n * g2};
  gv[0] = l0 * A0[0] + l2 * (-2.0 * f0k - kap * f0kk) * kp;
#pragma unroll
  for (int m = 1; m < 5; m++) gv[m] = l0 * A0[m] + l2 * (-S1[m] - kap * A0[m]);
  gs0 = l0 * fv[0] + l2 * fv[1];
}

// One kappa column through the collocation elimination (param_sensitivity.h: d_psens_cond's formulas with rows 0 and 2 of
// G1t / G2t instead of rows 3..5: v and bc have rows 0..2, b rows 0..2, w = Hc bc + gct rows 0..4), contracted at once:
//   bc = M8^-1 (-G2t - 2 E2 G1t),  b = 2 (E1 bc + G1t),  w = Hc bc + gct,  y = M8^-T w,
//   q = (2I - 4E2)^T y,  r = -h [(I + 2E2)^T y]_{delta, T},  qx = gxt;     a_k . q + a_{k+1} . qx + e_k . r + nu_{k+1} . b
// g1 / g2: rows (0, 2) of G1t / G2t; gct / gxt: entries 0..4.
__device__ __forceinline__ double tab_kappa_column(const Slot& S, const M8Blocks& M, const double hdt, const double* g1, const double* g2,
                                                   const double* gct, const double* gxt, const double* ak, const double* an,
                                                   const double* e, const double* nu) {
  double G1[8] = {g1[0], 0, g1[1], 0, 0, 0, 0, 0}, v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8], y[8];
  v[0] = -g2[0], v[2] = -g2[1];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int l = 0; l < 3; l++) v[i] -= 2.0 * S.E2[i * 8 + l] * G1[l];
  m8_solve<2>(M, v, bc);
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double s = G1[i];
#pragma unroll
    for (int l = 0; l < 3; l++) s += S.E1[i * 8 + l] * bc[l];
    acc += nu[i] * 2.0 * s;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    double s = i < 5 ? gct[i] : 0.0;
#pragma unroll
    for (int l = 0; l < 3; l++)
      if (hnz_(i, l)) s += sym_get(S.Hc, i, l) * bc[l];
    w[i] = s;
  }
  m8_solve_t(M, w, y);
#pragma unroll
  for (int a = 0; a < 8; a++) {
    double s = 2.0 * y[a];
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (a >= elo_(i) && a <= ehi_(i)) s -= 4.0 * S.E2[i * 8 + a] * y[i];
    acc += ak[a] * s;
  }
#pragma unroll
  for (int cc = 0; cc < 2; cc++) {
    double s = y[6 + cc];
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (6 + cc >= elo_(i) && 6 + cc <= ehi_(i)) s += 2.0 * S.E2[i * 8 + 6 + cc] * y[i];
    acc += e[cc] * (-hdt * s);
  }
#pragma unroll
  for (int m = 0; m < 5; m++) acc += an[m] * gxt[m];
  return acc;
}

template <class BP, bool PI = false, bool TS = false>
__device__ __forceinline__ void d_tab_cond(const Consts& K, const Work& W, const int k, const int b, const double* __restrict__ TJ,
                                           const int* __restrict__ ok_in, double* __restrict__ slot_grad) {
  const int N = W.N;
  const double hdt = K.o.t_step;
  const double eps = W.st[(size_t)ST_EPS * W.Bp + b], rho = W.st[(size_t)ST_RHO * W.Bp + b];
  const size_t ob = W.orig[b];
  double* const out = slot_grad + (ob * N + k) * TS_NS;
  if (!ok_in[ob]) {
#pragma unroll
    for (int c = 0; c < TS_NS; c++) out[c] = 0.0;
    return;
  }
  double c[8], xp[8], ak[8], an[8], nu[8], e[2];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c[i] = PL(W.C, i, k, N), xp[i] = PL(W.X, i, k + 1, N + 1);
    ak[i] = k > 0 ? PL(TJ, TJ_a + i, k - 1, N) : 0.0;
    an[i] = PL(TJ, TJ_a + i, k, N), nu[i] = PL(TJ, TJ_nu + i, k, N);
  }
  e[0] = PL(TJ, TJ_e, k, N), e[1] = PL(TJ, TJ_e + 1, k, N);
  // ---- the six node columns (qx only): track rows (nu d(grad h)/dy + grad h Sigma dh/dy) and the stage cost, nodes 1 .. N-1
  double node[6] = {0, 0, 0, 0, 0, 0};
  if (k + 1 <= N - 1) {
    const int m_nl = for_each_bound<BP>(K.p, [](int, int, int, double, double) {});
    double gv[3], gs[3], gn[3], gm[3], hss[3], hmm[3], Sg[3], nq[3];
    cons_eval(K.p, inst_tables<TS>(K.T, W, b), eps, xp, gv, gs, gn, gm, hss, hmm);
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const double t = PL(W.T, m_nl + q, k, N), el = rho > 0.0 ? PL(W.T, K.bd.ni + q, k, N) : 0.0;
      nq[q] = PL(W.NU, m_nl + q, k, N);
      double s0, s1;
      track_barrier(rho, gv[q], t, nq[q], el, Sg[q], s0, s1);
    }
    // dg/dN = -1 for the row's own table; d(grad g)/dN' = (-1, 0, 0)
    node[0] = -Sg[0] * (gs[0] * an[0] + gn[0] * an[1] + gm[0] * an[2]);
    node[1] = -nq[0] * an[0];
    node[2] = -Sg[1] * (gs[1] * an[0] + gn[1] * an[1] + gm[1] * an[2]) - Sg[2] * (gs[2] * an[0] + gn[2] * an[1] + gm[2] * an[2]);
    node[3] = -(nq[1] + nq[2]) * an[0];
    // stage cost q_v (vx - cv v_ref(s))^2: gradient (-2 q_v e cv v', 2 q_v e) over (s, vx)
    double vr, vr1, vr2;
    lut_eval(K.T.s_arc, inst_tables<TS>(K.T, W, b).v_ref, K.T.n, K.T.g0_arc, K.T.inv_arc, K.T.period, xp[0], eps, vr, vr1, vr2);
    const double cv = K.p.vref_scale, ee = xp[3] - cv * vr;
    node[4] = 2.0 * K.p.q_v * cv * (cv * vr1 * an[0] - an[3]);
    node[5] = -2.0 * K.p.q_v * ee * cv * an[0];
  }
#pragma unroll
  for (int q = 0; q < 6; q++) out[TS_NL + q] = node[q];
  // ---- the four kappa columns.  E1, E2 and the c-block Hc exactly as d_psens_cond forms them (same calls, same order)
  double kc, kpc, kx, kpx, cv_;
  lut_eval(K.T.s_kappa, inst_tables<TS>(K.T, W, b).kappa, K.T.n, K.T.g0_kappa, K.T.inv_kappa, K.T.period, c[0], eps, kc, kpc, cv_);
  lut_eval(K.T.s_kappa, inst_tables<TS>(K.T, W, b).kappa, K.T.n, K.T.g0_kappa, K.T.inv_kappa, K.T.period, xp[0], eps, kx, kpx, cv_);
  Slot S;
  {
    double lam[8], f[8], J[48];
#pragma unroll
    for (int i = 0; i < 8; i++) lam[i] = PL(W.L1, i, k, N);
#pragma unroll
    for (int i = 0; i < 36; i++) S.Hc[i] = 0.0;
    rhs_derivs(inst_params<PI>(K.p, W, b), inst_tables<TS>(K.T, W, b), eps, c, f, J, lam, hdt, S.Hc);
#pragma unroll
    for (int i = 0; i < 64; i++) S.E1[i] = 0.0, S.E2[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 48; i++) S.E1[i] = hdt * J[i];
    rhs_derivs(inst_params<PI>(K.p, W, b), inst_tables<TS>(K.T, W, b), eps, xp, f, J, nullptr, 0.0, nullptr);
#pragma unroll
    for (int i = 0; i < 48; i++) S.E2[i] = hdt * J[i];
#pragma unroll
    for (int i = 0; i < 8; i++) S.E1[i * 8 + i] -= 1.5, S.E2[i * 8 + i] -= 2.5;
    for_each_bound<BP>(K.p, [&](int m, int kind, int j, double, double) {
      if (kind == 1) S.Hc[sidx(j, j)] += PL(W.NU, m, k, N) * (1.0 / PL(W.T, m, k, N));
    });
  }
  M8Blocks M;
  factor_m8(S, M);
  // (the point's values are copied with selects, not reached through a pointer chosen at run time: that would put the arrays
  //  into scratch memory)
#pragma unroll 1
  for (int p = 0; p < 2; p++) {  // the point: c_k (multipliers L1, enters G1 and the c block) or x_{k+1} (L2, G2 and the node block)
    const bool atc = p == 0;
    double w[5];
#pragma unroll
    for (int m = 0; m < 5; m++) w[m] = atc ? c[m] : xp[m];
    const double l0 = hdt * (atc ? PL(W.L1, 0, k, N) : PL(W.L2, 0, k, N)), l2 = hdt * (atc ? PL(W.L1, 2, k, N) : PL(W.L2, 2, k, N));
    double fv[2], gvv[5], gs0;
    kappa_jet(w, atc ? kc : kx, atc ? kpc : kpx, l0, l2, fv, gvv, gs0);
    double g1[2], g2[2], gct[5], gxt[5];
#pragma unroll
    for (int i = 0; i < 2; i++) g1[i] = atc ? hdt * fv[i] : 0.0, g2[i] = atc ? 0.0 : hdt * fv[i];
#pragma unroll
    for (int m = 0; m < 5; m++) gct[m] = atc ? gvv[m] : 0.0, gxt[m] = atc ? 0.0 : gvv[m];
    out[2 * p] = tab_kappa_column(S, M, hdt, g1, g2, gct, gxt, ak, an, e, nu);
    g1[0] = g1[1] = g2[0] = g2[1] = 0.0;
#pragma unroll
    for (int m = 0; m < 5; m++) gct[m] = (m == 0 && atc) ? gs0 : 0.0, gxt[m] = (m == 0 && !atc) ? gs0 : 0.0;
    out[2 * p + 1] = tab_kappa_column(S, M, hdt, g1, g2, gct, gxt, ak, an, e, nu);
  }
}

template <class BP>
__global__ void __launch_bounds__(64) k_tab_cond(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, const double* __restrict__ TJ,
                                                 const int* __restrict__ ok_in, double* __restrict__ slot_grad) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_tab_cond<BP>(K, W, k, b, TJ, ok_in, slot_grad);
}
// with per-instance vehicle parameters (W.TH)
template <class BP>
__global__ void __launch_bounds__(64) k_tab_cond_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, const double* __restrict__ TJ,
                                                    const int* __restrict__ ok_in, double* __restrict__ slot_grad) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_tab_cond<BP, true>(K, W, k, b, TJ, ok_in, slot_grad);
}
// ... and per-instance table sets (W.TSV / W.TSI): every look-up on the rows of the instance's set
template <class BP>
__global__ void __launch_bounds__(64) k_tab_cond_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, const double* __restrict__ TJ,
                                                    const int* __restrict__ ok_in, double* __restrict__ slot_grad) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_tab_cond<BP, true, true>(K, W, k, b, TJ, ok_in, slot_grad);
}

// ------------------------------------------------------------------------------------------ k_tab_scatter
// thread = (look-up point p, interval k, instance b), p = 0: kappa at s(c_k), 1: kappa at s(x_{k+1}), 2: n_left, n_right, v_ref at
// s(x_{k+1}) (one basis for the three rows of the arc-length grid).  grad_tables [TAB_ROWS][n] must be zero before the launch.
// An instance with ok = 0 adds nothing, whatever its iterate holds (a non-finite s would give non-finite weights, and 0 times
// those is not 0).
__global__ void __launch_bounds__(256) k_tab_scatter(const Consts* __restrict__ Kp, Work W, const int* __restrict__ ok_in,
                                                     const double* __restrict__ slot_grad, double* __restrict__ grad_tables) {
  const Tables& T = Kp->T;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = W.N;
  const int b = (int)(tid % W.Bp), k = (int)((tid / W.Bp) % N), p = (int)(tid / ((size_t)W.Bp * N));
  if (p > 2 || b >= W.B) return;
  const size_t ob = W.orig[b];
  if (!ok_in[ob]) return;
  const double eps = W.st[(size_t)ST_EPS * W.Bp + b];
  const double s = p == 0 ? PL(W.C, 0, k, N) : PL(W.X, 0, k + 1, N + 1);
  const double* sg = slot_grad + (ob * N + k) * TS_NS;
  const int n = T.n;
  LutBasis R;
  if (p < 2) lut_basis(T.s_kappa, n, T.g0_kappa, T.inv_kappa, T.period, s, eps, R);
  else lut_basis(T.s_arc, n, T.g0_arc, T.inv_arc, T.period, s, eps, R);
  const int rows = p < 2 ? 1 : 3;
  for (int r = 0; r < rows; r++) {
    const int col = p < 2 ? 2 * p : TS_NL + 2 * r, row = p < 2 ? 0 : 1 + r;
    const double gval = sg[col], gslope = sg[col + 1];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double t = gval * R.wv[j] + gslope * R.ws[j];
      if (t != 0.0) atomicAdd(grad_tables + (size_t)row * n + R.idx[j], t);
    }
  }
}
// ... on a handle with per-instance table sets: grad_tables is [n_sets][TAB_ROWS][n] and an instance adds into the
// block of its set, tsi[its caller's index].  A copy of the kernel above (tests/test_table_sets_resources.py checks the text): through a
// shared __device__ function the uniform kernel's instructions changed (operand order of its multiplies).
__global__ void __launch_bounds__(256) k_tab_scatter_ts(const Consts* __restrict__ Kp, Work W, const int* __restrict__ ok_in,
                                                        const double* __restrict__ slot_grad, double* __restrict__ grad_tables,
                                                        const int* __restrict__ tsi) {
  const Tables& T = Kp->T;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = W.N;
  const int b = (int)(tid % W.Bp), k = (int)((tid / W.Bp) % N), p = (int)(tid / ((size_t)W.Bp * N));
  if (p > 2 || b >= W.B) return;
  const size_t ob = W.orig[b];
  if (!ok_in[ob]) return;
  const double eps = W.st[(size_t)ST_EPS * W.Bp + b];
  const double s = p == 0 ? PL(W.C, 0, k, N) : PL(W.X, 0, k + 1, N + 1);
  const double* sg = slot_grad + (ob * N + k) * TS_NS;
  const int n = T.n;
  grad_tables += (size_t)tsi[ob] * TAB_ROWS * n;
  LutBasis R;
  if (p < 2) lut_basis(T.s_kappa, n, T.g0_kappa, T.inv_kappa, T.period, s, eps, R);
  else lut_basis(T.s_arc, n, T.g0_arc, T.inv_arc, T.period, s, eps, R);
  const int rows = p < 2 ? 1 : 3;
  for (int r = 0; r < rows; r++) {
    const int col = p < 2 ? 2 * p : TS_NL + 2 * r, row = p < 2 ? 0 : 1 + r;
    const double gval = sg[col], gslope = sg[col + 1];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double t = gval * R.wv[j] + gslope * R.ws[j];
      if (t != 0.0) atomicAdd(grad_tables + (size_t)row * n + R.idx[j], t);
    }
  }
}

// dst += src, n words: a part of a split batch adds its grad_tables to the caller's array (ltompc_adjoint_tables_add_dev)
__global__ void __launch_bounds__(256) k_tab_add(double* __restrict__ dst, const double* __restrict__ src, const int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

}  // namespace ltompc
