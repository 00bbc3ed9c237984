// table_jvp.h — forward-mode sensitivities along a direction in the track tables (ltompc_get_jvp_tables): the
// product of the Jacobians of the predicted trajectory w.r.t. the knot values y of the four value rows kappa, n_left, n_right,
// v_ref with one direction dy,
//     tX[k,i] = sum_{r,j} dX[k,i]/dy[r][j] dy[r][j] (+ sum_j dX_dp[k,i,j] dp[j]),     tU likewise,
// the forward twin of table_sensitivity.h: dX/dy, dU/dy are the sensitivities whose transpose that header applies (the barrier
// problem at the final iterate, delta_w = 0, the slot's ST_EPS), same instances and ok.
//
// The tables enter slot (k, b) through the ten look-up results TS_* of table_sensitivity.h, which are linear in the knot values,
// so the direction reaches a slot as ten tangents: given by the caller (dslot, the forward twin of slot_grad), gathered from
// dtables with lut_basis' weights, or both, summed.  The linearised KKT system is linear in its right-hand side (jvp.h), so the
// ten columns of a slot collapse into ONE stage vector (q, r, b, qx), their tangent-weighted sum, and the recursion of jvp.h runs
// on that.  The condensation is linear too: the four kappa columns are summed BEFORE the two M8 solves.
//
//   k_tabjvp_cond<BP>    thread = (interval k, instance b): the ten tangents (dslot, and the gather of dtables through three
//                        bases: kappa at s(c_k), kappa at s(x_{k+1}), the arc grid at s(x_{k+1})), E1, E2, Hc and the M8
//                        factor by the calls d_tab_cond makes, tab_kappa_column's expressions uncontracted for the summed kappa
//                        columns and d_tab_cond's node columns -> the pass's TQ planes [26][N][Bp].  Zeros where ok is 0.  A
//                        gather without atomics: deterministic.
//   k_tabjvp_cond_pi<BP> the same with the instance's vehicle parameters in E1, E2, Hc
//   k_tabjvp_cond_ts<BP> ... and the rows (and the block of dtables, [n_sets][4][n_table]) of the instance's table set
//   k_jvp_sweep_tab      d_jvp_sweep<TH = true>'s recursion (jvp.h: the same expressions) with the stage vectors read from the TQ
//                        planes and without the r_du direction terms; kff through JV planes of the pass's own
//   k_jvp_sweep_tab_pi   the same with r_du from the instance's row (W.TH)
//
// Requires ptv = 0 and ell_penalty = 0 (the host rejects other handles).  The pass reads the iterate and the pass buffers of
// sensitivity.h and writes only buffers of its own.
#pragma once
#include "jvp.h"
#include "table_sensitivity.h"

namespace ltompc {

// TQ planes [field][k][Bp] written by slot k, in the order of a dynamics column of the PV planes: q (8, gradient of x_k from the
// collocation block), r (2), b (8), qx (8, node block of x_{k+1})
constexpr int TQ_q = 0, TQ_r = 8, TQ_b = 10, TQ_qx = 18, TQ_NF = 26;

// ------------------------------------------------------------------------------------------ k_tabjvp_cond
// sum_j y[idx[j]] (wv[j], ws[j]): value and slope tangent of one look-up along the row direction y
__device__ __forceinline__ void tabjvp_gather(const LutBasis& R, const double* __restrict__ y, double& tv, double& ts) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double d = y[R.idx[j]];
    tv += R.wv[j] * d, ts += R.ws[j] * d;
  }
}

// dtables: [TAB_ROWS][n] (TS: [n_sets][TAB_ROWS][n], the block of the instance's set) or nullptr; dslot: [B][N][TS_NS] in the
// caller's order or nullptr.
template <class BP, bool PI = false, bool TS = false>
__device__ __forceinline__ void d_tabjvp_cond(const Consts& K, const Work& W, const int k, const int b, const int* __restrict__ ok_in,
                                              const double* __restrict__ dtables, const double* __restrict__ dslot, double* __restrict__ TQ) {
  const int N = W.N;
  const double hdt = K.o.t_step;
  const double eps = W.st[(size_t)ST_EPS * W.Bp + b], rho = W.st[(size_t)ST_RHO * W.Bp + b];
  const size_t ob = W.orig[b];
  if (!ok_in[ob]) {  // (before any look-up: a non-finite s has no interval)
#pragma unroll
    for (int f = 0; f < TQ_NF; f++) PL(TQ, f, k, N) = 0.0;
    return;
  }
  double c[8], xp[8];
#pragma unroll
  for (int i = 0; i < 8; i++) c[i] = PL(W.C, i, k, N), xp[i] = PL(W.X, i, k + 1, N + 1);
  // ---- the ten tangents of the slot
  double t[TS_NS];
#pragma unroll
  for (int q = 0; q < TS_NS; q++) t[q] = dslot ? dslot[(ob * N + k) * TS_NS + q] : 0.0;
  if (dtables) {
    const Tables& T = K.T;
    const int n = T.n;
    const double* dy = dtables;
    if constexpr (TS) dy += (size_t)static_cast<const WorkTS&>(W).TSI[ob] * TAB_ROWS * n;
    LutBasis R;
    lut_basis(T.s_kappa, n, T.g0_kappa, T.inv_kappa, T.period, c[0], eps, R);
    tabjvp_gather(R, dy, t[TS_KC], t[TS_KC + 1]);
    lut_basis(T.s_kappa, n, T.g0_kappa, T.inv_kappa, T.period, xp[0], eps, R);
    tabjvp_gather(R, dy, t[TS_KX], t[TS_KX + 1]);
    if (k + 1 <= N - 1) {  // (the last slot has no node block)
      lut_basis(T.s_arc, n, T.g0_arc, T.inv_arc, T.period, xp[0], eps, R);
#pragma unroll
      for (int r = 0; r < 3; r++) tabjvp_gather(R, dy + (size_t)(1 + r) * n, t[TS_NL + 2 * r], t[TS_NL + 2 * r + 1]);
    }
  }
  // ---- the six node columns (qx over (s, n, mu, vx) only), d_tab_cond's without the adjoint vector, weighted and summed
  double qx[5] = {0, 0, 0, 0, 0};
  if (k + 1 <= N - 1) {
    const int m_nl = for_each_bound<BP>(K.p, [](int, int, int, double, double) {});
    double gv[3], gs[3], gn[3], gm[3], hss[3], hmm[3], Sg[3], nq[3];
    cons_eval(K.p, inst_tables<TS>(K.T, W, b), eps, xp, gv, gs, gn, gm, hss, hmm);
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const double tt = PL(W.T, m_nl + q, k, N), el = rho > 0.0 ? PL(W.T, K.bd.ni + q, k, N) : 0.0;
      nq[q] = PL(W.NU, m_nl + q, k, N);
      double s0, s1;
      track_barrier(rho, gv[q], tt, nq[q], el, Sg[q], s0, s1);
    }
    // dg/dN = -1 for the row's own table; d(grad g)/dN' = (-1, 0, 0)
    const double wl = -Sg[0] * t[TS_NL], wr1 = -Sg[1] * t[TS_NR], wr2 = -Sg[2] * t[TS_NR];
    qx[0] = wl * gs[0] + wr1 * gs[1] + wr2 * gs[2] - nq[0] * t[TS_NL + 1] - (nq[1] + nq[2]) * t[TS_NR + 1];
    qx[1] = wl * gn[0] + wr1 * gn[1] + wr2 * gn[2];
    qx[2] = wl * gm[0] + wr1 * gm[1] + wr2 * gm[2];
    // stage cost q_v (vx - cv v_ref(s))^2: gradient (-2 q_v e cv v', 2 q_v e) over (s, vx)
    double vr, vr1, vr2;
    lut_eval(K.T.s_arc, inst_tables<TS>(K.T, W, b).v_ref, K.T.n, K.T.g0_arc, K.T.inv_arc, K.T.period, xp[0], eps, vr, vr1, vr2);
    const double cv = K.p.vref_scale, ee = xp[3] - cv * vr;
    qx[0] += 2.0 * K.p.q_v * cv * (cv * vr1) * t[TS_VR] - 2.0 * K.p.q_v * ee * cv * t[TS_VR + 1];
    qx[3] = -2.0 * K.p.q_v * cv * t[TS_VR];
  }
  // ---- the four kappa columns, summed.  E1, E2 and the c-block Hc exactly as d_tab_cond forms them (same calls, same order)
  double kc, kpc, kx, kpx, cv_;
  lut_eval(K.T.s_kappa, inst_tables<TS>(K.T, W, b).kappa, K.T.n, K.T.g0_kappa, K.T.inv_kappa, K.T.period, c[0], eps, kc, kpc, cv_);
  lut_eval(K.T.s_kappa, inst_tables<TS>(K.T, W, b).kappa, K.T.n, K.T.g0_kappa, K.T.inv_kappa, K.T.period, xp[0], eps, kx, kpx, cv_);
  // the jets of both points weighted with their tangents: rows (0, 2) of G1t / G2t, entries 0..4 of gct / gxt.  (The point's
  // values are copied with selects, not reached through a pointer chosen at run time: that would put the arrays into scratch.)
  double g1[2] = {0, 0}, g2[2] = {0, 0}, gct[5] = {0, 0, 0, 0, 0}, gxt[5] = {0, 0, 0, 0, 0};
#pragma unroll 1
  for (int p = 0; p < 2; p++) {  // the point: c_k (multipliers L1, enters G1 and the c block) or x_{k+1} (L2, G2 and the node block)
    const bool atc = p == 0;
    double w[5];
#pragma unroll
    for (int m = 0; m < 5; m++) w[m] = atc ? c[m] : xp[m];
    const double l0 = hdt * (atc ? PL(W.L1, 0, k, N) : PL(W.L2, 0, k, N)), l2 = hdt * (atc ? PL(W.L1, 2, k, N) : PL(W.L2, 2, k, N));
    double fv[2], gvv[5], gs0;
    kappa_jet(w, atc ? kc : kx, atc ? kpc : kpx, l0, l2, fv, gvv, gs0);
    const double tv = atc ? t[TS_KC] : t[TS_KX], ts = atc ? t[TS_KC + 1] : t[TS_KX + 1];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const double v = hdt * fv[i] * tv;
      g1[i] = atc ? v : g1[i], g2[i] = atc ? g2[i] : v;
    }
#pragma unroll
    for (int m = 0; m < 5; m++) {
      const double v = gvv[m] * tv + (m == 0 ? gs0 * ts : 0.0);
      gct[m] = atc ? v : gct[m], gxt[m] = atc ? gxt[m] : v;
    }
  }
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
  // tab_kappa_column's elimination, uncontracted:
  //   bc = M8^-1 (-G2t - 2 E2 G1t),  b = 2 (E1 bc + G1t),  w = Hc bc + gct,  y = M8^-T w,
  //   q = (2I - 4E2)^T y,  r = -h [(I + 2E2)^T y]_{delta, T},  qx += gxt
  double G1[8] = {g1[0], 0, g1[1], 0, 0, 0, 0, 0}, v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8], y[8];
  v[0] = -g2[0], v[2] = -g2[1];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int l = 0; l < 3; l++) v[i] -= 2.0 * S.E2[i * 8 + l] * G1[l];
  m8_solve<2>(M, v, bc);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    double s = 0.0;
    if (i < 3) {
      s = G1[i];
#pragma unroll
      for (int l = 0; l < 3; l++) s += S.E1[i * 8 + l] * bc[l];
    }
    PL(TQ, TQ_b + i, k, N) = 2.0 * s;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    double s = i < 5 ? gct[i < 5 ? i : 0] : 0.0;
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
    PL(TQ, TQ_q + a, k, N) = s;
  }
#pragma unroll
  for (int cc = 0; cc < 2; cc++) {
    double s = y[6 + cc];
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (6 + cc >= elo_(i) && 6 + cc <= ehi_(i)) s += 2.0 * S.E2[i * 8 + 6 + cc] * y[i];
    PL(TQ, TQ_r + cc, k, N) = -hdt * s;
  }
#pragma unroll
  for (int m = 0; m < 8; m++) PL(TQ, TQ_qx + m, k, N) = m < 5 ? qx[m < 5 ? m : 0] + gxt[m < 5 ? m : 0] : 0.0;
}

template <class BP>
__global__ void __launch_bounds__(64) k_tabjvp_cond(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, const int* __restrict__ ok_in,
                                                    const double* __restrict__ dtables, const double* __restrict__ dslot,
                                                    double* __restrict__ TQ) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_tabjvp_cond<BP>(K, W, k, b, ok_in, dtables, dslot, TQ);
}
// with per-instance vehicle parameters (W.TH)
template <class BP>
__global__ void __launch_bounds__(64) k_tabjvp_cond_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, const int* __restrict__ ok_in,
                                                       const double* __restrict__ dtables, const double* __restrict__ dslot,
                                                       double* __restrict__ TQ) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_tabjvp_cond<BP, true>(K, W, k, b, ok_in, dtables, dslot, TQ);
}
// ... and per-instance table sets (W.TSV / W.TSI): every look-up on the rows of the instance's set, the direction
// from the block of its set
template <class BP>
__global__ void __launch_bounds__(64) k_tabjvp_cond_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, const int* __restrict__ ok_in,
                                                       const double* __restrict__ dtables, const double* __restrict__ dslot,
                                                       double* __restrict__ TQ) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_tabjvp_cond<BP, true, true>(K, W, k, b, ok_in, dtables, dslot, TQ);
}

// ------------------------------------------------------------------------------------------ k_jvp_sweep_tab
// jvp.h's d_jvp_sweep<TH = true> for the one stage vector of the TQ planes, with the same expressions stage by stage: the
// backward half from the operand loads to Huu's inverse and the exchange of b, Pb, gu, gx, and the forward pass, are
// d_jvp_sweep's text line for line (tests/test_table_jvp_sweep_source.py compares the two, so a fix there has to be made here
// too).  What differs: bi, gx, ri, qxs come from the TQ planes, and the r_du direction terms (d[14], d[15], du, uprev) are absent.
// Directions dp [B][10] in the caller's order or nullptr (zeros).  tX [B][N+1][8], tU [B][N][2] in the caller's order (either
// may be nullptr), exactly 0 where ok_in is 0.  JV: kff planes [JV_NF][N][Bp] of this pass.
template <bool PI>
__device__ __forceinline__ void d_jvp_sweep_tab(const Work& W, JvpLds& L, const double r0, const double r1, const double* __restrict__ TQ,
                                                const int* __restrict__ ok_in, const double* __restrict__ dp, double* __restrict__ JV,
                                                double* __restrict__ tX, double* __restrict__ tU) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < W.B;
  const int b = valid ? j : 0;
  const int N = W.N;
  const size_t ob = W.orig[b];
  const bool okk = ok_in[ob] != 0;
  {
    const gptr<const double> th = PI ? static_cast<const WorkPI&>(W).TH : nullptr;  // (PI: r_du of the instance's row, r0 / r1 unused)
    const double r2[2] = {2.0 * (PI ? th[(size_t)14 * W.Bp + ob] : r0), 2.0 * (PI ? th[(size_t)15 * W.Bp + ob] : r1)};
    // ---- backward recursion of the one vector (terminal: qx of the last slot)
    double pp = PL(TQ, TQ_qx + i, N - 1, N), pv[2] = {0.0, 0.0};
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
      // this slot's TQ words of row i (r: rows 0, 1; qx: the node block of x_k, slot k - 1, x_0 has none)
      const double bi = PL(TQ, TQ_b + i, k, N), ri = PL(TQ, TQ_r + (i & 1), k, N), qxs = PL(TQ, TQ_qx + i, km, N);
      double gx = PL(TQ, TQ_q + i, k, N);
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
#pragma unroll
      for (int l = 0; l < 8; l++) gx += Ac[l] * L.x[g][l];
      const double kf0 = -(Hi[0] * gu[0] + Hi[1] * gu[1]), kf1 = -(Hi[2] * gu[0] + Hi[3] * gu[1]);
      pp = gx + Kc[0] * gu[0] + Kc[1] * gu[1];
      pv[0] = -r2[0] * kf0;
      pv[1] = -r2[1] * kf1;
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
    // lanes 0 and 1 wrote kff_k and read their own word; lanes 2..7 load the same two words and drop them, and padding lanes
    // (b = 0, nothing stored) load slot 0's, which its own wavefront may be writing: the value is never used there
    const double kfo = PL(JV, i & 1, k, N), bi = PL(TQ, TQ_b + i, k, N);
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

// W: the pass's Work descriptor (QP, RC: the stored factorisation; orig: the solver's); TQ: k_tabjvp_cond's planes; JV: the
// pass's own kff planes
__global__ void __launch_bounds__(64) k_jvp_sweep_tab(Work W, double r0, double r1, const double* __restrict__ TQ, const int* __restrict__ ok_in,
                                                      const double* __restrict__ dp, double* __restrict__ JV, double* __restrict__ tX,
                                                      double* __restrict__ tU) {
  __shared__ JvpLds L;
  d_jvp_sweep_tab<false>(W, L, r0, r1, TQ, ok_in, dp, JV, tX, tU);
}
// with per-instance r_du (W.TH)
__global__ void __launch_bounds__(64) k_jvp_sweep_tab_pi(WorkPI W, const double* __restrict__ TQ, const int* __restrict__ ok_in,
                                                         const double* __restrict__ dp, double* __restrict__ JV, double* __restrict__ tX,
                                                         double* __restrict__ tU) {
  __shared__ JvpLds L;
  d_jvp_sweep_tab<true>(W, L, 0.0, 0.0, TQ, ok_in, dp, JV, tX, tU);
}

}  // namespace ltompc
