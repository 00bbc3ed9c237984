// param_sensitivity.h — parametric sensitivities of the solution w.r.t. the vehicle and cost parameters theta
// (ltompc_get_param_sensitivities).  Same definition as sensitivity.h (the barrier problem at the final
// iterate, delta_w = 0, implicit-function theorem): dz/dtheta = -F_z^-1 F_theta, on the factorisation that k_sens_riccati8
// stored in the pass's Riccati buffer.  Unlike (x0, u_prev), theta enters every stage, so each column has its own right-hand
// side: the condensed vectors (q, r, b) of F_theta, a backward recursion over the vectors only, then the forward pass
//     dU_k = K_k dX_k + Kv_k dV_k + kff_k,   dX_{k+1} = A_k dX_k + B_k dU_k + b_k,   dV_{k+1} = dU_k,   dX_0 = dV_0 = 0.
//
// theta (LTOMPC_NTHETA = 16 columns, natural units):
//   0 mass, 1 inertia_z, 2 B_f, 3 C_f, 4 D_f, 5 B_r, 6 C_r, 7 D_r, 8 C_m, 9 Cr_0, 10 Cr_2   (the dynamics: columns < PS_NDYN)
//   11 q_n, 12 q_mu, 13 q_B                                                                 (the node cost)
//   14 r_du[0], 15 r_du[1]                                                                  (the Delta-u cost)
// F_theta: the dynamics columns change h f in both collocation equations (rows vx, vy, r only: the kinematic rows have no
// vehicle parameter) and lambda^T df/dw in the stationarity rows of c_k and x_{k+1} (mixed second derivatives); the cost
// columns change the gradient of the node cost; r_du changes the gradient of r (u_k - u_{k-1})^2.
//
//   k_psens_cond<BP>  thread = (interval k, instance b): linearise_slot and the M8 factor of the evaluation kernels, the
//                     parameter jets of the dynamics at c_k and x_{k+1}, and the collocation elimination applied to the 11
//                     dynamics columns (M8, projection onto (x_k, u_k)) -> the pass's PV planes
//   k_psens_sweep     8 instances x 8 lanes per wavefront, 8 columns per wavefront (blockIdx.y: columns 0-7 / 8-15): the
//                     backward recursion of the vectors on the stored K, Kv, P, Pxv (Huu with the sweep's expression from
//                     the same blocks), then the forward pass; outputs in the caller's order through orig, 0 where the
//                     (x0, u_prev) pass's ok is 0
//
// Requires ptv = 0 and ell_penalty = 0 (the host rejects other handles).  The pass reads the iterate and the pass buffers of
// sensitivity.h and writes only buffers of its own.
#pragma once
#include "sensitivity.h"

namespace ltompc {

constexpr int PS_NT = LTOMPC_NTHETA;  // 16
constexpr int PS_NDYN = 11;           // columns that enter the dynamics
constexpr int PS_NC = 8;              // columns per wavefront of k_psens_sweep
// PV planes [field][k][Bp] written by slot k: dynamics column j < 11 at j * 26: q (8, gradient of x_k from the collocation
// block), r (2), b (8), qx (8, node block of x_{k+1}); cost column j = 11..13 at pv_base(j): qx (8)
constexpr int PV_q = 0, PV_r = 8, PV_b = 10, PV_qx = 18, PV_DYN = 26;
__host__ __device__ constexpr int pv_base(int j) { return j < PS_NDYN ? j * PV_DYN : PS_NDYN * PV_DYN + (j - PS_NDYN) * 8; }
__host__ __device__ constexpr int pv_qx(int j) { return j < PS_NDYN ? pv_base(j) + PV_qx : pv_base(j); }
constexpr int PV_NF = PS_NDYN * PV_DYN + 3 * 8;

// ------------------------------------------------------------------------------------------ parameter jets
// Tyre F = -K sin(C atan(B alpha)), K = F_N D (model.h: pacejka_jet).  Its gradient over the states is p1 dalpha/dw with
// p1 = dF/dalpha, and dalpha/dw does not depend on (B, C, D): their mixed derivatives are dp1/dtheta dalpha/dw.
struct TyreTheta {
  double F, p1;          // value, slope
  double Ft[3], p1t[3];  // d/dB, d/dC, d/dD of F and p1
  double ag[4];          // dalpha / d(vx, vy, r, delta)
};

__device__ __forceinline__ void tyre_theta(double vx, double vy, double r, double delta, double l, double delta_on, double Bp,
                                           double Cp, double Fn, double Dp, TyreTheta& T) {
  const double a = vy + l * r;
  const double iq = 1.0 / (a * a + vx * vx);
  const double ta = vx * iq, tb = -a * iq;
  const double alpha = atan2(a, vx) - delta_on * delta;
  T.ag[0] = tb, T.ag[1] = ta, T.ag[2] = l * ta, T.ag[3] = -delta_on;
  const double z = Bp * alpha, id = 1.0 / (1.0 + z * z), t = atan(z);
  double sc, cc;
  sincos(Cp * t, &sc, &cc);
  const double K = Fn * Dp;
  T.F = -K * sc;
  T.p1 = -K * cc * Cp * Bp * id;
  T.Ft[0] = -K * cc * Cp * alpha * id;
  T.Ft[1] = -K * cc * t;
  T.Ft[2] = -Fn * sc;
  T.p1t[0] = -K * Cp * id * id * (cc * (1.0 - z * z) - Cp * z * sc);
  T.p1t[1] = -K * Bp * id * (cc - Cp * t * sc);
  T.p1t[2] = -Fn * cc * Cp * Bp * id;
}

// Dynamics column j < PS_NDYN at one point w (c_k or x_{k+1}): fth = d(f_3, f_4, f_5)/dtheta_j and
// gth = sum_i lam_i d(df_i/dw)/dtheta_j over w = states 3..7 (ptv = 0).  j is a run-time, wave-uniform value: the pass loops
// over the columns with one column's values live at a time (unrolled, the compiler interleaved the 11 columns and spilled).
__device__ __forceinline__ void theta_jet(const ltompc_params& p, const int j, const double* w, const double* lam, double* fth, double* gth) {
  const double L = p.length_f + p.length_r, im = 1.0 / p.mass, iz = 1.0 / p.inertia_z;
  TyreTheta fr, rr;
  tyre_theta(w[3], w[4], w[5], w[6], p.length_f, 1.0, p.B_f, p.C_f, p.length_r * p.mass * p.gravity / L, p.D_f, fr);
  tyre_theta(w[3], w[4], w[5], w[6], -p.length_r, 0.0, p.B_r, p.C_r, p.length_f * p.mass * p.gravity / L, p.D_r, rr);
  double sd, cd;
  sincos(w[6], &sd, &cd);
  const double vx = w[3], th = w[7];
  double J3[5] = {0, 0, 0, 0, 0}, J4[5] = {0, 0, 0, 0, 0}, J5[5] = {0, 0, 0, 0, 0};
  fth[0] = fth[1] = fth[2] = 0.0;
  if (j <= 1) {  // mass, inertia_z: the yaw row f5 = (l_f F_yf cos(delta) - l_r F_yr) / I_z is proportional to F_N ~ m and to 1 / I_z
    const double s = j == 0 ? im : -iz;
    fth[2] = s * (p.length_f * fr.F * cd - p.length_r * rr.F) * iz;
#pragma unroll
    for (int m = 0; m < 4; m++) {
      double pc = fr.p1 * fr.ag[m] * cd;
      if (m == 3) pc -= fr.F * sd;
      J5[m] = s * (p.length_f * pc - p.length_r * rr.p1 * rr.ag[m]) * iz;
    }
    if (j == 0) {  // the vx row: F_y / m does not depend on m, the drivetrain and drag do
      fth[0] = -(p.C_m * th - p.Cr_0 - p.Cr_2 * vx * vx) * im * im;
      J3[0] = 2.0 * p.Cr_2 * vx * im * im, J3[4] = -p.C_m * im * im;
    }
  } else if (j <= 4) {  // B_f, C_f, D_f: through F_yf sin(delta) (vx row) and F_yf cos(delta) (vy, r rows)
    const double Ft = j == 2 ? fr.Ft[0] : (j == 3 ? fr.Ft[1] : fr.Ft[2]), pt = j == 2 ? fr.p1t[0] : (j == 3 ? fr.p1t[1] : fr.p1t[2]);
    fth[0] = -Ft * sd * im, fth[1] = Ft * cd * im, fth[2] = p.length_f * Ft * cd * iz;
#pragma unroll
    for (int m = 0; m < 4; m++) {
      double gs = pt * fr.ag[m] * sd, gc = pt * fr.ag[m] * cd;
      if (m == 3) gs += Ft * cd, gc -= Ft * sd;
      J3[m] = -gs * im, J4[m] = gc * im, J5[m] = p.length_f * gc * iz;
    }
  } else if (j <= 7) {  // B_r, C_r, D_r
    const double Ft = j == 5 ? rr.Ft[0] : (j == 6 ? rr.Ft[1] : rr.Ft[2]), pt = j == 5 ? rr.p1t[0] : (j == 6 ? rr.p1t[1] : rr.p1t[2]);
    fth[1] = Ft * im, fth[2] = -p.length_r * Ft * iz;
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const double gr = pt * rr.ag[m];
      J4[m] = gr * im, J5[m] = -p.length_r * gr * iz;
    }
  } else if (j == 8) {  // C_m
    fth[0] = th * im, J3[4] = im;
  } else if (j == 9) {  // Cr_0
    fth[0] = -im;
  } else {  // Cr_2
    fth[0] = -vx * vx * im, J3[0] = -2.0 * vx * im;
  }
#pragma unroll
  for (int m = 0; m < 5; m++) gth[m] = lam[0] * J3[m] + lam[1] * J4[m] + lam[2] * J5[m];
}

// Cost column j = 11..13: d/dtheta_j of the node cost's gradient at x (model.h: cost_eval; q_B only in the stage cost)
__device__ __forceinline__ void cost_theta(const ltompc_params& p, const int j, const double* x, const bool terminal, double* g) {
#pragma unroll
  for (int m = 0; m < 8; m++) g[m] = 0.0;
  if (j == 11) g[1] = 2.0 * x[1];
  if (j == 12) g[2] = 2.0 * x[2];
  if (j == 13 && !terminal) {
    const double vx = x[3], vy = x[4], de = x[6];
    const double rho = p.length_r / (p.length_f + p.length_r);
    const double iq = 1.0 / (vx * vx + vy * vy), d = 1.0 + rho * rho * de * de;
    const double bb = 2.0 * (atan(vy / vx) - atan(rho * de));
    g[3] = bb * (-vy * iq), g[4] = bb * (vx * iq), g[6] = bb * (-rho / d);
  }
}

// ------------------------------------------------------------------------------------------ k_psens_cond
// The dynamics columns through the collocation elimination of condense_slot (linearise.h), with (G1, G2) -> their theta
// derivatives and the gradients of c_k, x_{k+1} -> the mixed terms:
//   bc = M8^-1 (-G2t - 2 E2 G1t),  b = 2 (E1 bc + G1t),  w = Hc bc + gct,
//   q = Ac^T w = (2I - 4E2)^T M8^-T w,  r = Bc^T w = -h [(I + 2E2)^T M8^-T w]_{delta, T},  qx = gxt
// G1t, G2t have rows vx, vy, r only, so bc and b have rows 0..5 only.
template <class BP, bool PI = false>
__device__ __forceinline__ void d_psens_cond(const Consts& K, const Work& W, const int k, const int b, double* __restrict__ PV) {
  const int N = W.N;
  const double hdt = K.o.t_step;
  const double eps = W.st[(size_t)ST_EPS * W.Bp + b];
  double c[8], xp[8];
#pragma unroll
  for (int i = 0; i < 8; i++) c[i] = PL(W.C, i, k, N), xp[i] = PL(W.X, i, k + 1, N + 1);
  // Phase 1: the jets of every column, parked in the column's own planes (b: G1t rows 3..5, q: G2t rows 3..5 in 0..2 and gct
  // in 3..7; qx is final).  Phase 2 holds E1, E2, Hc and M8 (~130 values) and only one column at a time beside them.
  {
    double l1[3], l2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) l1[i] = hdt * PL(W.L1, 3 + i, k, N), l2[i] = hdt * PL(W.L2, 3 + i, k, N);
#pragma unroll 1
    for (int j = 0; j < PS_NDYN; j++) {
      double f1[3], g1[5], f2[3], g2[5];
      theta_jet(inst_params<PI>(K.p, W, b), j, c, l1, f1, g1);
      theta_jet(inst_params<PI>(K.p, W, b), j, xp, l2, f2, g2);
      double* out = PV + (size_t)pv_base(j) * N * W.Bp;  // (this column's planes)
#pragma unroll
      for (int i = 0; i < 3; i++) PL(out, PV_b + 3 + i, k, N) = hdt * f1[i], PL(out, PV_q + i, k, N) = hdt * f2[i];
#pragma unroll
      for (int m = 0; m < 5; m++) PL(out, PV_q + 3 + m, k, N) = g1[m];
#pragma unroll
      for (int a = 0; a < 8; a++) PL(out, PV_qx + a, k, N) = a >= 3 ? g2[a - 3] : 0.0;
    }
#pragma unroll 1
    for (int j = PS_NDYN; j < PS_NDYN + 3; j++) {
      double g[8];
      cost_theta(inst_params<PI>(K.p, W, b), j, xp, k == N - 1, g);
      double* out = PV + (size_t)pv_qx(j) * N * W.Bp;
#pragma unroll
      for (int a = 0; a < 8; a++) PL(out, a, k, N) = g[a];
    }
  }
  // Phase 2.  E1, E2 and the c-block Hc exactly as linearise_slot forms them (same calls, same order of the sums); nothing of
  // x_{k+1}'s node block, the cost or the track constraints is needed here.
  Slot S;
  {
    double lam[8], f[8], J[48];
#pragma unroll
    for (int i = 0; i < 8; i++) lam[i] = PL(W.L1, i, k, N);
#pragma unroll
    for (int i = 0; i < 36; i++) S.Hc[i] = 0.0;
    rhs_derivs(inst_params<PI>(K.p, W, b), K.T, eps, c, f, J, lam, hdt, S.Hc);
#pragma unroll
    for (int i = 0; i < 64; i++) S.E1[i] = 0.0, S.E2[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 48; i++) S.E1[i] = hdt * J[i];
    rhs_derivs(inst_params<PI>(K.p, W, b), K.T, eps, xp, f, J, nullptr, 0.0, nullptr);
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
#pragma unroll 1
  for (int j = 0; j < PS_NDYN; j++) {
    double* out = PV + (size_t)pv_base(j) * N * W.Bp;
    double G1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8], y[8];
#pragma unroll
    for (int i = 0; i < 3; i++) G1[3 + i] = PL(out, PV_b + 3 + i, k, N), v[3 + i] = -PL(out, PV_q + i, k, N);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = i >= 3 ? PL(out, PV_q + i, k, N) : 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int l = 3; l < 6; l++)
        if (l >= elo_(i) && l <= ehi_(i)) v[i] -= 2.0 * S.E2[i * 8 + l] * G1[l];
    m8_solve<5>(M, v, bc);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < 6; l++)
        if (l >= elo_(i) && l <= ehi_(i)) s += S.E1[i * 8 + l] * bc[l];
      PL(out, PV_b + i, k, N) = 2.0 * (s + G1[i]);
#pragma unroll
      for (int l = 0; l < 6; l++)
        if (hnz_(i, l)) w[i] += sym_get(S.Hc, i, l) * bc[l];
    }
    m8_solve_t(M, w, y);
#pragma unroll
    for (int a = 0; a < 8; a++) {
      double s = 2.0 * y[a];
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (a >= elo_(i) && a <= ehi_(i)) s -= 4.0 * S.E2[i * 8 + a] * y[i];
      PL(out, PV_q + a, k, N) = s;
    }
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
      double s = y[6 + cc];
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (6 + cc >= elo_(i) && 6 + cc <= ehi_(i)) s += 2.0 * S.E2[i * 8 + 6 + cc] * y[i];
      PL(out, PV_r + cc, k, N) = -hdt * s;
    }
  }
}

template <class BP>
__global__ void __launch_bounds__(64) k_psens_cond(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, double* __restrict__ PV) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_psens_cond<BP>(K, W, k, b, PV);
}
// with per-instance vehicle and cost parameters (W.TH)
template <class BP>
__global__ void __launch_bounds__(64) k_psens_cond_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, double* __restrict__ PV) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_psens_cond<BP, true>(K, W, k, b, PV);
}

// ------------------------------------------------------------------------------------------ k_psens_sweep
// Columns c0 = 8 * blockIdx.y + col.  Per stage k (N-1 .. 0), with P, Pxv of stage k+1 and K, Kv of stage k as stored by the
// head-less sweep, for every column (lane (g, i) owns row i; pp, pv: the vector parts of the cost-to-go):
//   Pb = pp + P b,   gu = r + dJdu + pv + B^T Pb + Pxv^T b,   gx = q + qx + A^T Pb,   kff = -Huu^-1 gu,
//   pp <- gx + Hxu kff = gx + K^T gu,   pv <- dJdv - diag(2 r_du) kff
// (dJdu, dJdv: the r_du columns' d/dr of the gradient of r (u_k - v_k)^2; terminal: pp = qx of node N, pv = 0).
// Huu = R + Pvv + B^T P B + B^T Pxv + Pxv^T B + diag(2 r_du) with Pvv = diag(2 r_du) (I - Kv_{k+1}) is the sweep's
// expression (d_riccati8) on the blocks it stored, inverted and guarded the same way.  kff goes to KF ([k][c][16][Bp], lane c
// writes and later reads its own), then the forward pass.  ok_in: the (x0, u_prev) pass's ok in the caller's order.
struct PsensLds {
  double x[8][8 * PS_NC];  // [g][row * 8 + col]: b, Pb and dX exchanged between the rows
};

template <int H, bool PI = false>
__device__ __forceinline__ void d_psens_sweep(const Work& W, PsensLds& L, const double r0, const double r1, const double* __restrict__ uprev,
                                              const double* __restrict__ PV,
                                              const int* __restrict__ ok_in, double* __restrict__ KF, double* __restrict__ du0,
                                              double* __restrict__ dXo, double* __restrict__ dUo) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int j = blockIdx.x * 8 + g;
  const bool valid = j < W.B;
  const int b = valid ? j : 0;
  const int N = W.N;
  const size_t ob = W.orig[b];
  const bool okk = ok_in[ob] != 0;
  const gptr<const double> th = PI ? static_cast<const WorkPI&>(W).TH : nullptr;  // (PI: r_du of the instance's row, r0 / r1 unused)
  const double r2[2] = {2.0 * (PI ? th[(size_t)14 * W.Bp + ob] : r0), 2.0 * (PI ? th[(size_t)15 * W.Bp + ob] : r1)};
  constexpr int C0 = H * PS_NC;
  // row i of a column's vector at slot k (compile-time zero where the column has none)
  auto vq = [&](const int c, const int k) { return C0 + c < PS_NDYN ? PL(PV, pv_base(C0 + c) + PV_q + i, k, N) : 0.0; };
  auto vb = [&](const int c, const int k) { return C0 + c < PS_NDYN ? PL(PV, pv_base(C0 + c) + PV_b + i, k, N) : 0.0; };
  auto vqx = [&](const int c, const int k) { return C0 + c < PS_NDYN + 3 ? PL(PV, pv_qx(C0 + c) + i, k, N) : 0.0; };
  auto vr = [&](const int c, const int k, const int d) { return C0 + c < PS_NDYN ? PL(PV, pv_base(C0 + c) + PV_r + d, k, N) : 0.0; };
  // ---- backward recursion of the vectors
  double pp[PS_NC], pv[2][PS_NC];
#pragma unroll
  for (int c = 0; c < PS_NC; c++) pp[c] = vqx(c, N - 1), pv[0][c] = pv[1][c] = 0.0;
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
    double du[2];
    {
      const double uk0 = PL(W.U, 0, k, N), uk1 = PL(W.U, 1, k, N);
      const int km = k > 0 ? k - 1 : 0;
      const double v0 = k > 0 ? PL(W.U, 0, km, N) : uprev[ob * 2], v1 = k > 0 ? PL(W.U, 1, km, N) : uprev[ob * 2 + 1];
      du[0] = uk0 - v0, du[1] = uk1 - v1;
    }
    // Huu (the same number in the 8 lanes of an instance)
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
    // the columns: row i of b, then of Pb, exchanged through LDS
    double bi[PS_NC], Pb[PS_NC];
#pragma unroll
    for (int c = 0; c < PS_NC; c++) bi[c] = vb(c, k);
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < PS_NC; c++) L.x[g][i * PS_NC + c] = bi[c];
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < PS_NC; c++) {
      double s = pp[c];
#pragma unroll
      for (int l = 0; l < 8; l++) s += Prow[l] * L.x[g][l * PS_NC + c];
      Pb[c] = s;
    }
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < PS_NC; c++) L.x[g][i * PS_NC + c] = Pb[c];
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < PS_NC; c++) {
      double gu[2];
#pragma unroll
      for (int d = 0; d < 2; d++) {
        const double own = i == d ? vr(c, k, d) : 0.0;  // (lane d adds the column's r_d once)
        gu[d] = grp_sum(Bm[i * 2 + d] * Pb[c] + Xi[d] * bi[c] + own) + pv[d][c];
      }
      if (C0 + c == 14) gu[0] += 2.0 * du[0];
      if (C0 + c == 15) gu[1] += 2.0 * du[1];
      const double qxn = vqx(c, k > 0 ? k - 1 : 0);  // (node block of x_k: slot k - 1; x_0 has none)
      double gx = vq(c, k) + (k > 0 ? qxn : 0.0);
#pragma unroll
      for (int l = 0; l < 8; l++) gx += Ac[l] * L.x[g][l * PS_NC + c];
      const double kf0 = -(Hi[0] * gu[0] + Hi[1] * gu[1]), kf1 = -(Hi[2] * gu[0] + Hi[3] * gu[1]);
      pp[c] = gx + Kc[0] * gu[0] + Kc[1] * gu[1];
      pv[0][c] = (C0 + c == 14 ? -2.0 * du[0] : 0.0) - r2[0] * kf0;
      pv[1][c] = (C0 + c == 15 ? -2.0 * du[1] : 0.0) - r2[1] * kf1;
      if (valid && i < 2) KF[(((size_t)k * 2 + i) * PS_NT + C0 + c) * W.Bp + b] = i == 0 ? kf0 : kf1;
    }
  }
  // ---- forward pass
  double dx[PS_NC], dv[2][PS_NC];
#pragma unroll
  for (int c = 0; c < PS_NC; c++) dx[c] = 0.0, dv[0][c] = dv[1][c] = 0.0;
  if (valid && dXo) {
#pragma unroll
    for (int c = 0; c < PS_NC; c++) dXo[(ob * (N + 1) * 8 + i) * PS_NT + C0 + c] = 0.0;
  }
#pragma unroll 1
  for (int k = 0; k < N; k++) {
    double Ar[8], Bi[2], Kc[2], Kv[4];
#pragma unroll
    for (int l = 0; l < 8; l++) Ar[l] = PG(W.QP, QP_A + i * 8 + l, k, QP_NF);
    Bi[0] = PG(W.QP, QP_B + i * 2, k, QP_NF), Bi[1] = PG(W.QP, QP_B + i * 2 + 1, k, QP_NF);
    Kc[0] = PG(W.RC, RC_K + i, k, RC_NF), Kc[1] = PG(W.RC, RC_K + 8 + i, k, RC_NF);
#pragma unroll
    for (int l = 0; l < 4; l++) Kv[l] = PG(W.RC, RC_Kv + l, k, RC_NF);
    double kf[PS_NC], bi[PS_NC];
#pragma unroll
    for (int c = 0; c < PS_NC; c++) {
      kf[c] = i < 2 ? KF[(((size_t)k * 2 + i) * PS_NT + C0 + c) * W.Bp + b] : 0.0;
      bi[c] = vb(c, k);
    }
    double du[2][PS_NC];
#pragma unroll
    for (int c = 0; c < PS_NC; c++)
#pragma unroll
      for (int d = 0; d < 2; d++)
        du[d][c] = grp_sum(Kc[d] * dx[c] + (i == d ? kf[c] : 0.0)) + Kv[d * 2] * dv[0][c] + Kv[d * 2 + 1] * dv[1][c];
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < PS_NC; c++) L.x[g][i * PS_NC + c] = dx[c];
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < PS_NC; c++) {
      double s = bi[c] + Bi[0] * du[0][c] + Bi[1] * du[1][c];
#pragma unroll
      for (int l = 0; l < 8; l++) s += Ar[l] * L.x[g][l * PS_NC + c];
      dx[c] = s;
      dv[0][c] = du[0][c], dv[1][c] = du[1][c];
    }
    if (valid) {
      if (k == 0 && du0 && i < 2) {
#pragma unroll
        for (int c = 0; c < PS_NC; c++) du0[(ob * 2 + i) * PS_NT + C0 + c] = okk ? (i == 0 ? du[0][c] : du[1][c]) : 0.0;
      }
      if (dUo && i < 2) {
#pragma unroll
        for (int c = 0; c < PS_NC; c++) dUo[((ob * N + k) * 2 + i) * PS_NT + C0 + c] = okk ? (i == 0 ? du[0][c] : du[1][c]) : 0.0;
      }
      if (dXo) {
#pragma unroll
        for (int c = 0; c < PS_NC; c++) dXo[((ob * (N + 1) + k + 1) * 8 + i) * PS_NT + C0 + c] = okk ? dx[c] : 0.0;
      }
    }
  }
}

// u_prev of the solve (caller's order, B x 2) by make_step, before k_store_u0 makes W.uprev its u0 (the r_du columns need u_0 - u_prev)
__global__ void k_psens_keep_uprev(Work W, double* __restrict__ uprev_rm, const int* __restrict__ orig) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  const size_t r = orig ? orig[b] : b;
  uprev_rm[r * 2] = W.uprev[b], uprev_rm[r * 2 + 1] = W.uprev[(size_t)W.Bp + b];
}

// W: the pass's Work descriptor (QP, RC: the stored factorisation; U, orig: the solver's); uprev: k_psens_keep_uprev's
__global__ void __launch_bounds__(64) k_psens_sweep(Work W, double r0, double r1, const double* __restrict__ uprev, const double* __restrict__ PV,
                                                    const int* __restrict__ ok_in,
                                                    double* __restrict__ KF, double* __restrict__ du0, double* __restrict__ dXo,
                                                    double* __restrict__ dUo) {
  __shared__ PsensLds L;
  if (blockIdx.y == 0) d_psens_sweep<0>(W, L, r0, r1, uprev, PV, ok_in, KF, du0, dXo, dUo);
  else d_psens_sweep<1>(W, L, r0, r1, uprev, PV, ok_in, KF, du0, dXo, dUo);
}
// with per-instance r_du (W.TH)
__global__ void __launch_bounds__(64) k_psens_sweep_pi(WorkPI W, const double* __restrict__ uprev, const double* __restrict__ PV,
                                                    const int* __restrict__ ok_in,
                                                    double* __restrict__ KF, double* __restrict__ du0, double* __restrict__ dXo,
                                                    double* __restrict__ dUo) {
  __shared__ PsensLds L;
  if (blockIdx.y == 0) d_psens_sweep<0, true>(W, L, 0.0, 0.0, uprev, PV, ok_in, KF, du0, dXo, dUo);
  else d_psens_sweep<1, true>(W, L, 0.0, 0.0, uprev, PV, ok_in, KF, du0, dXo, dUo);
}

}  // namespace ltompc
