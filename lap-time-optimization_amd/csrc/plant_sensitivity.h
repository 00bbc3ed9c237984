// plant_sensitivity.h — sensitivities of the plant step and of the closed loop (ltompc_plant_sensitivities, ltompc_loop_*,
// DESIGN.md §12).
//
// The plant step x_next = Phi(x, u, theta) is k_plant's discrete map: classical RK4 with n_sub sub-steps under zero-order-hold u
// (aux_kernels.h: d_plant), the curvature table exact (eps = 0, slope of the current interval).  Its derivative is the TANGENT of
// those 4 n_sub stage evaluations: with z_i the stage points and v a column of d y / d q,
//     kv_i = df/dx(z_i) vz_i + df/dtheta(z_i),   vz_1 = v,  vz_2 = v + h/2 kv_1,  vz_3 = v + h/2 kv_2,  vz_4 = v + h kv_3,
//     v <- v + h/6 (kv_1 + 2 kv_2 + 2 kv_3 + kv_4),
// not the continuous variational equation integrated on its own.  df/dx is rhs_derivs' J (model.h), df/dtheta theta_jet's fth
// (param_sensitivity.h: rows vx, vy, r of the 11 dynamics columns; the five cost columns do not enter the plant: exactly 0).
//
//   k_plant_sens      8 instances x 8 lanes per wavefront.  21 columns are integrated (x: 8, u: 2, dynamics theta: 11), rows
//                     s .. r only: the rows delta and T of every column are closed forms (d delta / d delta = 1,
//                     d delta(t) / d u_0 = t, 0 for theta) that enter the stage tangents as constants.  Lane i of an instance owns
//                     the columns i, 8 + i and 16 + i of that list (x_i; u_i or theta_{i-2}; theta_{i+6} or none) - 36 values per
//                     lane - and evaluates the stage point and J itself (the 8 lanes of an instance run in lock-step anyway;
//                     nothing is exchanged).  The column index of theta_jet is a run-time value, one per lane.
//                     Output: planes [PSN_NF][Bp] (instance-fastest), dxn_dx | dxn_du | dxn_dtheta, each row-major per instance.
//                     x_next is k_plant's own (the host launches it): bit for bit the plant step.
//   k_loop_begin      Sx = [I_8 | 0], Du = 0, ok = 1, ticks = 0
//   k_loop_accum      thread = (column q of (x_init[0..7], theta[0..15]), instance b): one tick of the closed-loop recursion
//                         Du <- K0 Sx + Kv0 Du + [mode & 1] Tth,      Sx <- Phi_x Sx + Phi_u Du + [mode & 2] Phi_th
//                     with K0, Kv0 (ltompc_sensitivities_dev) and Tth (ltompc_param_sensitivities_dev) of the tick's solve and
//                     Phi of the plant step at (x_t, u0_t).  An instance whose solve has ok = 0 leaves the loop: its loop ok
//                     becomes 0, Sx and Du exactly 0 from then on, its tick counter stops.
//   k_planes_rows     planes [F][Bp] -> row-major [B][F] (the caller-facing arrays)
//
// All of it in the caller's instance order (the plant step and the du0 outputs of the passes are), and in buffers of its own.
#pragma once
#include "param_sensitivity.h"

namespace ltompc {

constexpr int PSN_DX = 0, PSN_DU = 64, PSN_DTH = 80, PSN_NF = 80 + 8 * PS_NT;  // fields of the planes: 8 x 8 | 8 x 2 | 8 x 16
constexpr int LOOP_NQ = LTOMPC_NLOOP;                                            // columns q = (x_init[0..7], theta[0..15])
static_assert(LOOP_NQ == 8 + PS_NT, "LTOMPC_NLOOP = 8 + LTOMPC_NTHETA");

// structural non-zeros of rhs_derivs' J (rows s .. r over the 8 states)
__host__ __device__ constexpr bool psn_jnz(int r, int l) {
  return r == 0 ? l <= 4 : r == 1 ? (l >= 2 && l <= 4) : r == 2 ? l <= 5 : r == 3 ? l >= 3 : (l >= 3 && l <= 6);
}

template <bool PI, class TP>
__device__ __forceinline__ void d_plant_sens(const Consts& K, const int B, const size_t Bp, const double* __restrict__ x,
                                             const double* __restrict__ u, const double dt, const int n_sub, const int with_theta,
                                             double* __restrict__ planes, const TP th) {
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int inst = blockIdx.x * 8 + g;
  const bool valid = inst < B;
  const size_t b = valid ? inst : 0;  // (padding lanes follow instance 0 and store nothing)
  decltype(auto) p = sel_params<PI>(K.p, th, Bp, b);
  double y[8];
#pragma unroll
  for (int r = 0; r < 8; r++) y[r] = x[b * 8 + r];
  const double uu[2] = {u[b * 2], u[b * 2 + 1]};
  // the lane's three columns: constant (c6, c7) and ramp (r6, r7) parts of their rows delta, T; theta index (-1: none)
  const double c6[3] = {i == 6 ? 1.0 : 0.0, 0.0, 0.0}, c7[3] = {i == 7 ? 1.0 : 0.0, 0.0, 0.0};
  const double r6[3] = {0.0, i == 0 ? 1.0 : 0.0, 0.0}, r7[3] = {0.0, i == 1 ? 1.0 : 0.0, 0.0};
  const int jt[3] = {-1, (with_theta && i >= 2) ? i - 2 : -1, (with_theta && i < 5) ? i + 6 : -1};
  double v[3][6], kp[3][6], av[3][6];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int r = 0; r < 6; r++) v[c][r] = (c == 0 && r == i) ? 1.0 : 0.0, kp[c][r] = 0.0;
  const double hs = dt / n_sub;
#pragma unroll 1
  for (int s = 0; s < n_sub; s++) {
    const double t0 = s * hs;  // time since the start of the step: the ramp of the u columns
    double kf[6], af[6];
#pragma unroll
    for (int r = 0; r < 6; r++) kf[r] = 0.0, af[r] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int r = 0; r < 6; r++) av[c][r] = 0.0;
#pragma unroll 1
    for (int st = 0; st < 4; st++) {
      const double a = (st == 0 ? 0.0 : (st == 3 ? 1.0 : 0.5)) * hs, w = (st == 0 || st == 3) ? 1.0 : 2.0;
      double z[8], f[6], J[48];
#pragma unroll
      for (int r = 0; r < 6; r++) z[r] = y[r] + a * kf[r];
      z[6] = y[6] + a * uu[0], z[7] = y[7] + a * uu[1];
      rhs_derivs(p, K.T, 0.0, z, f, J, nullptr, 0.0, nullptr);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double fth[3] = {0.0, 0.0, 0.0};
        if (c > 0 && jt[c] >= 0) {
          const double lam[3] = {0.0, 0.0, 0.0};
          double gth[5];
          theta_jet(p, jt[c], z, lam, fth, gth);
        }
        const double vz6 = c6[c] + r6[c] * (t0 + a), vz7 = c7[c] + r7[c] * (t0 + a);
        double vz[6], kv[6];
#pragma unroll
        for (int l = 0; l < 6; l++) vz[l] = v[c][l] + a * kp[c][l];
#pragma unroll
        for (int r = 0; r < 6; r++) {
          double acc = r >= 3 ? fth[r - 3] : 0.0;
#pragma unroll
          for (int l = 0; l < 6; l++)
            if (psn_jnz(r, l)) acc += J[r * 8 + l] * vz[l];
          if (psn_jnz(r, 6)) acc += J[r * 8 + 6] * vz6;
          if (psn_jnz(r, 7)) acc += J[r * 8 + 7] * vz7;
          kv[r] = acc;
        }
#pragma unroll
        for (int r = 0; r < 6; r++) kp[c][r] = kv[r], av[c][r] += w * kv[r];
      }
#pragma unroll
      for (int r = 0; r < 6; r++) kf[r] = f[r], af[r] += w * f[r];
    }
#pragma unroll
    for (int r = 0; r < 6; r++) y[r] += hs / 6.0 * af[r];
    y[6] += hs * uu[0], y[7] += hs * uu[1];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int r = 0; r < 6; r++) v[c][r] += hs / 6.0 * av[c][r];
  }
  if (!valid) return;
  auto out = [&](const int f) -> double& { return planes[(size_t)f * Bp + b]; };
#pragma unroll
  for (int r = 0; r < 8; r++) out(PSN_DX + r * 8 + i) = r < 6 ? v[0][r] : (r == i ? 1.0 : 0.0);
  if (i < 2) {
#pragma unroll
    for (int r = 0; r < 8; r++) out(PSN_DU + r * 2 + i) = r < 6 ? v[1][r] : (r - 6 == i ? dt : 0.0);
  } else if (with_theta) {
#pragma unroll
    for (int r = 0; r < 8; r++) out(PSN_DTH + r * PS_NT + i - 2) = r < 6 ? v[1][r] : 0.0;
  }
  if (with_theta) {
    if (i < 5) {
#pragma unroll
      for (int r = 0; r < 8; r++) out(PSN_DTH + r * PS_NT + i + 6) = r < 6 ? v[2][r] : 0.0;
    }
    if (i >= 3) {  // the cost columns 11 .. 15
#pragma unroll
      for (int r = 0; r < 8; r++) out(PSN_DTH + r * PS_NT + PS_NDYN + i - 3) = 0.0;
    }
  }
}

__global__ void __launch_bounds__(64) k_plant_sens(Consts K, int B, int Bp, const double* __restrict__ x, const double* __restrict__ u, double dt,
                                                   int n_sub, int with_theta, double* __restrict__ planes) {
  d_plant_sens<false>(K, B, Bp, x, u, dt, n_sub, with_theta, planes, (const double*)nullptr);
}
// with per-instance vehicle parameters: th is a [LTOMPC_NTHETA][Bp] plane in the caller's instance order (as for k_plant_pi)
__global__ void __launch_bounds__(64) k_plant_sens_pi(Consts K, const double* __restrict__ th, int B, int Bp, const double* __restrict__ x,
                                                      const double* __restrict__ u, double dt, int n_sub, int with_theta,
                                                      double* __restrict__ planes) {
  d_plant_sens<true>(K, B, Bp, x, u, dt, n_sub, with_theta, planes, th);
}

// planes [f0 + f][Bp], f < F  ->  row-major out[b][f]
__global__ void k_planes_rows(const double* __restrict__ planes, int f0, int F, int B, int Bp, double* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * F) return;
  const size_t b = t / F, f = t % F;
  out[t] = planes[(size_t)(f0 + f) * Bp + b];
}

// ------------------------------------------------------------------------------------------ closed loop
// Sx [8 * LOOP_NQ][Bp] (field r * LOOP_NQ + q), Du [2 * LOOP_NQ][Bp], ok [Bp], ticks [Bp]
__global__ void k_loop_begin(int B, int Bp, double* __restrict__ Sx, double* __restrict__ Du, int* __restrict__ ok, int* __restrict__ ticks) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % Bp, q = tid / Bp;
  if (q >= LOOP_NQ || b >= B) return;
#pragma unroll
  for (int r = 0; r < 8; r++) Sx[(size_t)(r * LOOP_NQ + q) * Bp + b] = r == q ? 1.0 : 0.0;
  Du[(size_t)q * Bp + b] = 0.0, Du[(size_t)(LOOP_NQ + q) * Bp + b] = 0.0;
  if (q == 0) ok[b] = 1, ticks[b] = 0;
}

// du0_dp: B x 2 x 10, du0_dth: B x 2 x 16 (null without mode bit 1), sens_ok: B - the tick's solve, in the caller's order;
// phi: k_plant_sens' planes at (x_t, u0_t) (the theta block only with mode bit 2).  A thread reads and writes its own column
// only; ok[b] is written by column 0 alone, and every column gets the same new value from either the old or the new one.
__global__ void __launch_bounds__(256) k_loop_accum(int B, int Bp, int mode, const double* __restrict__ du0_dp, const double* __restrict__ du0_dth,
                             const int* __restrict__ sens_ok, const double* __restrict__ phi, double* __restrict__ Sx,
                             double* __restrict__ Du, int* ok, int* __restrict__ ticks) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = tid % Bp, q = tid / Bp;
  if (q >= LOOP_NQ || b >= B) return;
  const bool good = ok[b] != 0 && sens_ok[b] != 0;
  double sx[8], nx[8], du[2], nu[2];
#pragma unroll
  for (int r = 0; r < 8; r++) sx[r] = Sx[(size_t)(r * LOOP_NQ + q) * Bp + b];
  du[0] = Du[(size_t)q * Bp + b], du[1] = Du[(size_t)(LOOP_NQ + q) * Bp + b];
  const bool thc = q >= 8;  // a theta column
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const double* kr = du0_dp + ((size_t)b * 2 + c) * SENS_NP;
    double s = (thc && (mode & 1)) ? du0_dth[((size_t)b * 2 + c) * PS_NT + (q - 8)] : 0.0;
#pragma unroll
    for (int l = 0; l < 8; l++) s += kr[l] * sx[l];
    nu[c] = s + kr[8] * du[0] + kr[9] * du[1];
  }
#pragma unroll
  for (int r = 0; r < 8; r++) {
    double s = (thc && (mode & 2)) ? phi[(size_t)(PSN_DTH + r * PS_NT + (q - 8)) * Bp + b] : 0.0;
#pragma unroll
    for (int l = 0; l < 8; l++) s += phi[(size_t)(PSN_DX + r * 8 + l) * Bp + b] * sx[l];
    nx[r] = s + phi[(size_t)(PSN_DU + r * 2) * Bp + b] * nu[0] + phi[(size_t)(PSN_DU + r * 2 + 1) * Bp + b] * nu[1];
  }
#pragma unroll
  for (int r = 0; r < 8; r++) Sx[(size_t)(r * LOOP_NQ + q) * Bp + b] = good ? nx[r] : 0.0;
  Du[(size_t)q * Bp + b] = good ? nu[0] : 0.0, Du[(size_t)(LOOP_NQ + q) * Bp + b] = good ? nu[1] : 0.0;
  if (q == 0) {
    if (good) ticks[b] += 1;
    else ok[b] = 0;
  }
}

}  // namespace ltompc
