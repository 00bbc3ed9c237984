// linesearch.h — step candidates, filter test, update (k_linesearch, k_pick, k_update) and their fusion for narrow
// launches (k_step1).
#pragma once
#include "layout.h"

namespace ltompc {

// ------------------------------------------------------------------------------------------ where the line search reads
// The operands of d_linesearch that belong to the instance's iterate and step (not to the candidate): the planes themselves
// (SrcPlanes: k_linesearch, every wide kernel) or the copy that k_step1 keeps in LDS (StepStage, below).  One text, two sources:
// every accessor of SrcPlanes is the expression d_linesearch had in its place.
struct SrcPlanes {
  static constexpr bool staged = false;
  __device__ __forceinline__ double eps(const Work& W, const int b) const { return W.st[(size_t)ST_EPS * W.Bp + b]; }
  __device__ __forceinline__ double rho(const Work& W, const int b) const { return W.st[(size_t)ST_RHO * W.Bp + b]; }
  __device__ __forceinline__ double apri(const Work& W, const int b, const int N, const int kk) const { return PL(W.SP, SP_apri, kk, N); }
  __device__ __forceinline__ double Xn(const Work& W, const int b, const int N, const int i, const int k) const {  // node k, node 0 the measured state
    return k == 0 ? W.x0[(size_t)i * W.Bp + b] : PL(W.X, i, k, N + 1);
  }
  __device__ __forceinline__ double X(const Work& W, const int b, const int N, const int i, const int k) const { return PL(W.X, i, k, N + 1); }
  __device__ __forceinline__ double dX(const Work& W, const int b, const int N, const int i, const int k) const { return PL(W.dX, i, k, N + 1); }
  __device__ __forceinline__ double C(const Work& W, const int b, const int N, const int i, const int k) const { return PL(W.C, i, k, N); }
  __device__ __forceinline__ double dC(const Work& W, const int b, const int N, const int i, const int k) const { return PL(W.dC, i, k, N); }
  __device__ __forceinline__ double U(const Work& W, const int b, const int N, const int i, const int k) const { return PL(W.U, i, k, N); }
  __device__ __forceinline__ double dU(const Work& W, const int b, const int N, const int i, const int k) const { return PL(W.dU, i, k, N); }
  __device__ __forceinline__ double Up(const Work& W, const int b, const int N, const int i, const int k) const {  // slot k - 1, slot -1 the applied input
    return k ? PL(W.U, i, k - 1, N) : W.uprev[(size_t)i * W.Bp + b];
  }
  __device__ __forceinline__ double dUp(const Work& W, const int b, const int N, const int i, const int k) const { return k ? PL(W.dU, i, k - 1, N) : 0.0; }
  __device__ __forceinline__ double T(const Work& W, const int b, const int N, const int m, const int k) const { return PL(W.T, m, k, N); }
  __device__ __forceinline__ double dT(const Work& W, const int b, const int N, const int m, const int k) const { return PL(W.dT, m, k, N); }
};

// k_step1's copy of one instance's operands in LDS.  The planes are [field][k][Bp], instance fastest, and a workgroup of k_step1
// holds ONE instance: every word it loads is a 64-byte sector of its own, and all of them pass the CU's one cache port.  The
// eight candidates of a slot, the neighbour slots (x_k is x_{k+1} of the slot before, u_{k-1} its u_k) and the update after the
// pick asked for each word about seven times; staged, each word passes the port once (d_step1_stage) and the rest are LDS reads.
// Layout, in doubles: eps, rho | the N partials SP_apri | `cols` columns of `stride` words, column = node or slot minus k0, the
// word of a column = the row: x_i, dx_i at 2 i, 2 i + 1 (column = node, node 0 of X is W.x0), c_i, dc_i at SG_C + 2 i, + 1 (column =
// slot), u_i, du_i at SG_U + 2 i, + 1 (column = slot + 1, so that column 0 of the first window is slot -1: W.uprev and a step of 0),
// t_m, dt_m at SG_T + 2 m, + 1 for the R = ni + NNL + nel rows of T (the slacks and the elastic variables, every row the planes
// have; column = slot).  A lane reads through ONE address, its column's, with the row as the instruction's constant offset, a
// word and its step side by side in one read; stride is odd, so lanes with consecutive k read without a bank conflict, and the
// candidates of one slot read the same word (a broadcast).  (Rows of `cols` words each, [field][k], need an address per row:
// 119 SGPRs spilled and 10 VGPRs with them, where this layout spills 80 and none.)
// A window holds the slots k0 .. k0 + ks - 1, ks = cols - 1 (their nodes k0 .. k0 + ks need cols columns), as many as the
// array has room for beside the N partials: at the reference's bound pattern (R = 26) N <= 67 is ONE window and the update reads it
// too (`whole`); a longer horizon or a larger pattern takes several windows, one after the other, and its update reads the planes.
constexpr int STG_WORDS = 6144;  // 48 KiB, static: three workgroups a CU, as many as the registers allow
enum : int { SG_X = 0, SG_C = 16, SG_U = 32, SG_T = 36 };
struct StepStage {
  static constexpr bool staged = true;
  double* s;       // the workgroup's array
  int N, R;        // horizon; rows of T (and of dT)
  int stride, ks;  // words of a column; slots of a window
  int k0;          // first slot of the window held
  __device__ __forceinline__ bool whole() const { return N <= ks; }  // the one window is the instance
  __device__ __forceinline__ const double* at(const int row, const int col) const { return s + 2 + N + (col - k0) * stride + row; }
  __device__ __forceinline__ double eps(const Work&, const int) const { return s[0]; }
  __device__ __forceinline__ double rho(const Work&, const int) const { return s[1]; }
  __device__ __forceinline__ double apri(const Work&, const int, const int, const int kk) const { return s[2 + kk]; }
  __device__ __forceinline__ double Xn(const Work&, const int, const int, const int i, const int k) const { return *at(SG_X + 2 * i, k); }
  __device__ __forceinline__ double X(const Work&, const int, const int, const int i, const int k) const { return *at(SG_X + 2 * i, k); }
  __device__ __forceinline__ double dX(const Work&, const int, const int, const int i, const int k) const { return *at(SG_X + 2 * i + 1, k); }
  __device__ __forceinline__ double C(const Work&, const int, const int, const int i, const int k) const { return *at(SG_C + 2 * i, k); }
  __device__ __forceinline__ double dC(const Work&, const int, const int, const int i, const int k) const { return *at(SG_C + 2 * i + 1, k); }
  __device__ __forceinline__ double U(const Work&, const int, const int, const int i, const int k) const { return *at(SG_U + 2 * i, k + 1); }
  __device__ __forceinline__ double dU(const Work&, const int, const int, const int i, const int k) const { return *at(SG_U + 2 * i + 1, k + 1); }
  __device__ __forceinline__ double Up(const Work&, const int, const int, const int i, const int k) const { return *at(SG_U + 2 * i, k); }
  __device__ __forceinline__ double dUp(const Work&, const int, const int, const int i, const int k) const { return *at(SG_U + 2 * i + 1, k); }
  __device__ __forceinline__ double T(const Work&, const int, const int, const int m, const int k) const { return *at(SG_T + 2 * m, k); }
  __device__ __forceinline__ double dT(const Work&, const int, const int, const int m, const int k) const { return *at(SG_T + 2 * m + 1, k); }
};
// words of a column for R rows of T (odd), and the columns for horizon N: what is left beside eps, rho and the partials, over the
// stride; at most 128 columns, so that the 320 lanes are at least two rows of columns (d_step1_stage).
// (tests/test_host_harness_step1_stage.py derives the last horizon of one window from the same lines.)
__host__ __device__ constexpr int stage_stride(const int R) { return SG_T + 2 * R + 1; }
__host__ __device__ constexpr int stage_cols(const int N, const int R) {
  const int c = (STG_WORDS - 2 - N) / stage_stride(R);
  return c < 128 ? c : 128;
}
static_assert(stage_cols(4096, MAX_NI + NNL + NEL) >= 2, "a window holds at least one slot at the longest horizon and the largest pattern");
static_assert(stage_cols(40, 23 + NNL + NEL) > 40, "the benchmark's instance (N = 40, the reference's pattern, with or without the ellipse) is one window");

// ------------------------------------------------------------------------------------------ k_linesearch
// candidate 0 is the current point (alpha = 0); candidate l >= 1 has alpha = a_pri * 2^-(l-1).
// LS plane layout: [3 * (n_ls + 1)][N][Bp] : theta, cost, sum log t per candidate.
// Two phases (97% of all iterations accept the full step): phase 0 evaluates the current point and the first candidate
// for every instance; phase 1 evaluates the remaining candidates for the instances whose first candidate was rejected.
// Filter measures (theta, cost, sum log t) of the step candidates l_begin..l_end of interval k of instance b;
// candidate l >= 1 has alpha = a_pri * 2^-(l-1) (l = 0, the current point, is written by k_eval).
template <class BP, bool PIN, bool ELL, bool PI = false, bool TS = false, class SRC = SrcPlanes>
__device__ __forceinline__ void d_linesearch(const Consts& K, const Work& W, const int k, const int b, const int l_begin,
                                             const int l_end, const SRC& src = SRC()) {
  const int N = W.N;
  const double hdt = K.o.t_step;
  if constexpr (!SRC::staged) {  // (k_step1 has tested the two flags for the workgroup before it staged anything)
    if (W.si[(size_t)SI_DONE * W.Bp + b] || !W.si[(size_t)SI_STEP * W.Bp + b]) return;  // no step this launch
  }
  const double eps = src.eps(W, b), rho = src.rho(W, b);
  double a_pri = 1.0;
  for (int kk = 0; kk < N; kk += 20) {  // twenty loads in flight per round trip (a plain loop waits for every single one)
    double v20[20];
#pragma unroll
    for (int q = 0; q < 20; q++) v20[q] = src.apri(W, b, N, kk + q < N ? kk + q : N - 1);
#pragma unroll
    for (int q = 0; q < 20; q++) a_pri = fmin(a_pri, v20[q]);
  }
  double xk[8], xp[8], c[8], u[2], v[2], dxk[8], dxp[8], dc[8], du[2], dv[2];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    xk[i] = src.Xn(W, b, N, i, k);
    dxk[i] = src.dX(W, b, N, i, k);
    xp[i] = src.X(W, b, N, i, k + 1), dxp[i] = src.dX(W, b, N, i, k + 1);
    c[i] = src.C(W, b, N, i, k), dc[i] = src.dC(W, b, N, i, k);
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    u[i] = src.U(W, b, N, i, k), du[i] = src.dU(W, b, N, i, k);
    v[i] = src.Up(W, b, N, i, k);
    dv[i] = src.dUp(W, b, N, i, k);
  }
  const bool nl = (k + 1 <= N - 1);
  // candidate index l: 0 = current point, l >= 1: alpha = a_pri * 2^-(l-1)
  for (int l = l_begin; l <= l_end; l++) {
    const double alpha = l == 0 ? 0.0 : ldexp(a_pri, -(l - 1));
    double txk[8], txp[8], tc[8], tu[2], tv[2];
#pragma unroll
    for (int i = 0; i < 8; i++) txk[i] = xk[i] + alpha * dxk[i], txp[i] = xp[i] + alpha * dxp[i], tc[i] = c[i] + alpha * dc[i];
#pragma unroll
    for (int i = 0; i < 2; i++) tu[i] = u[i] + alpha * du[i], tv[i] = v[i] + alpha * dv[i];
    // the five table look-ups of the candidate (kappa at both points, v_ref / n_left / n_right at x_{k+1}) in ONE batch of
    // loads, and with them the slacks of the track constraints (and their elastic variables): loaded unconditionally, used
    // conditionally.  (Looked up one after the other inside rhs_val / cost_eval / cons_eval, and the slacks pair by pair between
    // the tests of nl and rho, these were eleven dependent round trips.)
    const Tables& Tb = inst_tables<TS>(K.T, W, b);
#if defined(__HIP_DEVICE_COMPILE__)
    if (!PIN) {
      // (k_step1: the candidate's point complete before the knots are asked for.  Left alone the compiler fetches the two arc
      //  lengths first and issues the knots among the other 50 loads of the state: state and step, the knots and the slacks
      //  together do not fit the 256 registers of two wavefronts per SIMD)
      asm volatile("" : "+v"(tc[0]), "+v"(tc[1]), "+v"(tc[2]), "+v"(tc[3]), "+v"(tc[4]), "+v"(tc[5]), "+v"(tc[6]), "+v"(tc[7]),
                        "+v"(txp[0]), "+v"(txp[1]), "+v"(txp[2]), "+v"(txp[3]), "+v"(txp[4]), "+v"(txp[5]), "+v"(txp[6]), "+v"(txp[7]),
                        "+v"(txk[0]), "+v"(txk[1]), "+v"(txk[2]), "+v"(txk[3]), "+v"(txk[4]), "+v"(txk[5]), "+v"(txk[6]), "+v"(txk[7]),
                        "+v"(tu[0]), "+v"(tu[1]), "+v"(tv[0]), "+v"(tv[1]));
    }
#endif
    SlotLutsRaw lraw;
    slot_luts_fetch(Tb, tc[0], txp[0], lraw);
    constexpr int NTR = ELL ? 5 : 3;
    double tn[NTR], dtn[NTR], en[NTR], den[NTR];
    const auto fetch_track = [&](const int m0) {  // (these planes exist for every slot: k_expand writes zeros in the last one)
#pragma unroll
      for (int q = 0; q < NTR; q++) {
        tn[q] = src.T(W, b, N, m0 + q, k), dtn[q] = src.dT(W, b, N, m0 + q, k);
        en[q] = src.T(W, b, N, K.bd.ni + q, k), den[q] = src.dT(W, b, N, K.bd.ni + q, k);
      }
    };
    // compile-time bound pattern: the slacks of the simple bounds in one batch of loads as well.  PIN: in the batch of the knots
    // (k_linesearch); else on their own after the cost (k_step1, two wavefronts per SIMD: 80 registers more in the batch of the
    // knots and it spills)
    double t0[BP::fixed ? MAX_NI : 1] = {}, d0[BP::fixed ? MAX_NI : 1] = {};  // (zero: the pinning below touches whole chunks of 8)
    const auto fetch_bounds = [&] { for_each_bound<BP>(K.p, [&](int mm, int, int, double, double) { t0[mm] = src.T(W, b, N, mm, k), d0[mm] = src.dT(W, b, N, mm, k); }); };
    const int nb = BP::fixed ? for_each_bound<BP>(K.p, [](int, int, int, double, double) {}) : 0;
    if (BP::fixed && PIN) fetch_bounds();
    if (BP::fixed) fetch_track(nb);
    // (the knots were issued first: the look-ups are finished while the slacks are still on their way)
    slot_luts_pin(lraw);
    SlotLuts lut;
    slot_luts_finish(Tb, lraw, eps, k != N - 1, nl, lut);
#if defined(__HIP_DEVICE_COMPILE__)
    if (BP::fixed) {
      // (all of them in registers before the first use: left alone the compiler issues and awaits them pair by pair)
#pragma unroll
      for (int q = 0; q < MAX_NI; q += 8)
        if (PIN && q < nb) {
          double* a = t0 + q;
          double* c = d0 + q;
          asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                            "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]));
        }
#pragma unroll
      for (int q = 0; q < NTR; q++) asm volatile("" : "+v"(tn[q]), "+v"(dtn[q]), "+v"(en[q]), "+v"(den[q]));
    }
#endif
    double f1[8], f2[8];
    rhs_val(inst_params<PI>(K.p, W, b), lut.kc.v, tc, tu, f1);
    rhs_val(inst_params<PI>(K.p, W, b), lut.kx.v, txp, tu, f2);
    double th = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      th += fabs(hdt * f1[i] + 2.0 * txk[i] - 1.5 * tc[i] - 0.5 * txp[i]);
      th += fabs(hdt * f2[i] - 2.0 * txk[i] + 4.5 * tc[i] - 2.5 * txp[i]);
    }
    double co = cost_eval(inst_params<PI>(K.p, W, b), lut.vr, txp, k == N - 1, nullptr, nullptr);
#pragma unroll
    for (int i = 0; i < 2; i++) co += inst_r_du<PI>(K.p, W, b, i) * (tu[i] - tv[i]) * (tu[i] - tv[i]);
    // sum of log t as the log of products of 8 slacks (same grouping in linearise_slot): 3 logarithms instead of 23
    double sl = 0.0, pr = 1.0;
    double tt[BP::fixed ? MAX_NI : 1];
    if (BP::fixed) {
      if (!PIN) fetch_bounds();
#pragma unroll
      for (int q = 0; q < MAX_NI; q++)
        if (q < nb) tt[q] = t0[q] + alpha * d0[q];
    }
    const int m = for_each_bound<BP>(K.p, [&](int mm, int kind, int jj, double sg, double val) {
      const double xv = kind == 0 ? tu[jj] : (kind == 1 ? tc[jj] : txp[jj]);
      double t;  // (the planes' form names no `src`: captured here, it changed the instructions of k_linesearch<BoundsAny>)
      if constexpr (SRC::staged) t = BP::fixed ? tt[mm] : src.T(W, b, N, mm, k) + alpha * src.dT(W, b, N, mm, k);
      else t = BP::fixed ? tt[mm] : PL(W.T, mm, k, N) + alpha * PL(W.dT, mm, k, N);
      th += fabs(sg * (xv - val) + t), pr *= t;
      if ((mm & 7) == 7) sl += log(pr), pr = 1.0;
    });
    if (!BP::fixed) fetch_track(m);  // run-time bound pattern: m is known only now
    if (nl) {
      double gv[3];
      cons_eval(K.p, lut.nl, lut.nr, txp, gv, nullptr, nullptr, nullptr, nullptr, nullptr);
#pragma unroll
      for (int q = 0; q < 3; q++) {
        double t = tn[q] + alpha * dtn[q];
        double e = 0.0;
        pr *= t;
        if (rho > 0.0) {  // elastic variable of the softened constraint: g - e + t = 0, cost rho e
          e = en[q] + alpha * den[q];
          pr *= e, co += rho * e;
        }
        th += fabs(gv[q] - e + t);
        if (((m + q) & 7) == 7) sl += log(pr), pr = 1.0;
      }
      if (ELL) {  // friction-ellipse constraints (always soft): same grouping of the logarithms as linearise_slot
        double ge[2];
        ellipse_val(K.p, txp, ge);
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const int mm = m + 3 + q;
          const double t = tn[NTR - 2 + q] + alpha * dtn[NTR - 2 + q];
          const double e = en[NTR - 2 + q] + alpha * den[NTR - 2 + q];
          pr *= t, pr *= e, co += K.p.ell_penalty * e;
          th += fabs(ge[q] - e + t);
          if ((mm & 7) == 7) sl += log(pr), pr = 1.0;
        }
      }
    }
    sl += log(pr);
    PL(W.LS, 3 * l + 0, k, N) = th, PL(W.LS, 3 * l + 1, k, N) = co, PL(W.LS, 3 * l + 2, k, N) = sl;
  }
}

template <class BP, bool ELL>
__global__ void __launch_bounds__(64) k_linesearch(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, Launch la, int phase, int jw) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  // phase 0: thread = (k, j), evaluates the first candidate (full step to the boundary) of instance act[j].
  // phase 1: thread = (candidate, k, j'), one candidate each (latency matters here, not throughput), over the packed
  //          list of rejected instances; jw = launch width in instances, longer lists are covered grid-stride.
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = W.N;
  const int j0 = tid % jw, rest = tid / jw, k = rest % N, cand = rest / N;
  if (phase == 0 ? (rest >= N) : (cand >= K.o.n_linesearch - 1)) return;
  const int count = phase == 0 ? la.nact[0] : W.ls_count[0];
  const int l = phase == 0 ? 1 : 2 + cand;
  for (int j = j0; j < count; j += jw) d_linesearch<BP, true, ELL>(K, W, k, phase == 0 ? la.act[j] : W.ls_list[j], l, l);
}
// with per-instance vehicle and cost parameters (W.TH)
template <class BP>
__global__ void __launch_bounds__(64) k_linesearch_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, Launch la, int phase, int jw) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  // phase 0: thread = (k, j), evaluates the first candidate (full step to the boundary) of instance act[j].
  // phase 1: thread = (candidate, k, j'), one candidate each (latency matters here, not throughput), over the packed
  //          list of rejected instances; jw = launch width in instances, longer lists are covered grid-stride.
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = W.N;
  const int j0 = tid % jw, rest = tid / jw, k = rest % N, cand = rest / N;
  if (phase == 0 ? (rest >= N) : (cand >= K.o.n_linesearch - 1)) return;
  const int count = phase == 0 ? la.nact[0] : W.ls_count[0];
  const int l = phase == 0 ? 1 : 2 + cand;
  for (int j = j0; j < count; j += jw) d_linesearch<BP, true, false, true>(K, W, k, phase == 0 ? la.act[j] : W.ls_list[j], l, l);
}

// ... and per-instance table sets (W.TSV / W.TSI)
template <class BP>
__global__ void __launch_bounds__(64) k_linesearch_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, Launch la, int phase, int jw) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  // phase 0: thread = (k, j), evaluates the first candidate (full step to the boundary) of instance act[j].
  // phase 1: thread = (candidate, k, j'), one candidate each (latency matters here, not throughput), over the packed
  //          list of rejected instances; jw = launch width in instances, longer lists are covered grid-stride.
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = W.N;
  const int j0 = tid % jw, rest = tid / jw, k = rest % N, cand = rest / N;
  if (phase == 0 ? (rest >= N) : (cand >= K.o.n_linesearch - 1)) return;
  const int count = phase == 0 ? la.nact[0] : W.ls_count[0];
  const int l = phase == 0 ? 1 : 2 + cand;
  for (int j = j0; j < count; j += jw) d_linesearch<BP, true, false, true, true>(K, W, k, phase == 0 ? la.act[j] : W.ls_list[j], l, l);
}

// ------------------------------------------------------------------------------------------ k_pick
// Filter line search of Waechter & Biegler 2006 (no second-order correction, no restoration phase).
// 8 lanes per instance (lane = g + 8 i, all 8 lanes of a group call this together): lane i reduces the stage partials
// k = i, i+8, ...; the 8 lanes then hold the same numbers and take the same decisions, lane i == 0 writes.  (Keeps the
// latency of this small step at N/8 dependent loads instead of N.)
constexpr int PICK_Q = 5;  // stages per lane and round trip: N = 40 in one (with 8, k_step1's 256 registers do not hold the batch)
template <bool PI = false, bool TS = false>
__device__ __forceinline__ void d_pick(const Consts& K, const Work& W, const int b, const int i, const int phase,
                                       const bool append_list) {
  const int N = W.N;
  double* st = W.st;
  int* si = W.si;
  const ltompc_options& o = K.o;
  // Everything the function can read on any of its paths, in ONE batch of loads: the per-instance state (the two flags that
  // decide whether there is anything to do among them), x0 (eps switch only), the filter, the step partials and the measures
  // of the current point and the full step.  The decisions are then taken in registers and lane i == 0 writes what changed in
  // one group at the end: read and written field by field where it was used, the state cost a memory round trip per field
  // (13 dependent ones on the common path; on gfx9 a load issued after a store waits for the store as well, vmcnt counts
  // both in order).
  int done = STI(SI_DONE), step = STI(SI_STEP);
  double mu = STD(ST_MU), eps = STD(ST_EPS), eps_next = STD(ST_EPS_NEXT), force_reg = STD(ST_FORCE_REG), theta0 = STD(ST_THETA0);
  double theta_max = STD(ST_THMAX), theta_min = STD(ST_THMIN), c00 = STD(ST_C00), rho = STD(ST_RHO);
  int nfilt = STI(SI_NFILT), nlsfail = STI(SI_NLSFAIL), ntiny = STI(SI_NTINY), resto = STI(SI_RESTO), nresto = STI(SI_NRESTO);
  int warm = STI(SI_WARM), nshift = STI(SI_NSHIFT), blowup = STI(SI_BLOWUP), iters = STI(SI_ITERS);
  double x0[8];
#pragma unroll
  for (int q = 0; q < 8; q++) x0[q] = W.x0[(size_t)q * W.Bp + b];
  // the filter (at most FILTER_MAX pairs), in registers: it only changes when a candidate is accepted
  double fth[FILTER_MAX], fph[FILTER_MAX];
#pragma unroll
  for (int f = 0; f < FILTER_MAX; f++) fth[f] = W.filt[(size_t)(2 * f) * W.Bp + b], fph[f] = W.filt[(size_t)(2 * f + 1) * W.Bp + b];
  // horizon sums: lane i takes the stages k = i, i + 8, ...; PICK_Q of them per round trip (all of N <= 8 PICK_Q in the batch
  // above), the additions keep the order k = i, i + 8, ...
  double sp[3][PICK_Q], ls[6][PICK_Q];
#pragma unroll
  for (int q = 0; q < PICK_Q; q++) {
    const int k = i + 8 * q < N ? i + 8 * q : N - 1;  // (past the horizon: a valid word, not used)
    sp[0][q] = PL(W.SP, SP_apri, k, N), sp[1][q] = PL(W.SP, SP_adua, k, N), sp[2][q] = PL(W.SP, SP_gphid, k, N);
#pragma unroll
    for (int f = 0; f < 6; f++) ls[f][q] = PL(W.LS, f, k, N);  // candidates 0 (the current point) and 1 (the full step)
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // (all of them in registers before the first use: left alone the compiler sinks the loads into the branches that use them)
#define LT_PIN8(a) asm volatile("" : "+v"((a)[0]), "+v"((a)[1]), "+v"((a)[2]), "+v"((a)[3]), "+v"((a)[4]), "+v"((a)[5]), "+v"((a)[6]), "+v"((a)[7]))
  asm volatile("" : "+v"(mu), "+v"(eps), "+v"(eps_next), "+v"(force_reg), "+v"(theta0), "+v"(theta_max), "+v"(theta_min), "+v"(c00), "+v"(rho));
  asm volatile("" : "+v"(nfilt), "+v"(nlsfail), "+v"(ntiny), "+v"(resto), "+v"(nresto), "+v"(warm), "+v"(nshift), "+v"(blowup), "+v"(iters),
                    "+v"(done), "+v"(step));
  LT_PIN8(x0);
  static_assert(FILTER_MAX % 8 == 0, "the filter is pinned in chunks of 8 pairs");
#pragma unroll
  for (int f = 0; f < FILTER_MAX; f += 8) LT_PIN8(fth + f);
#pragma unroll
  for (int f = 0; f < FILTER_MAX; f += 8) LT_PIN8(fph + f);
#pragma unroll
  for (int q = 0; q < PICK_Q; q++)
    asm volatile("" : "+v"(sp[0][q]), "+v"(sp[1][q]), "+v"(sp[2][q]), "+v"(ls[0][q]), "+v"(ls[1][q]), "+v"(ls[2][q]), "+v"(ls[3][q]), "+v"(ls[4][q]), "+v"(ls[5][q]));
#undef LT_PIN8
#endif
  if (done || !step) return;  // finished, or the Riccati sweep of this launch has to be repeated
  double a_pri = 1.0, a_dua = 1.0, gphid = 0.0;
#pragma unroll
  for (int q = 0; q < PICK_Q; q++)
    if (i + 8 * q < N) a_pri = fmin(a_pri, sp[0][q]), a_dua = fmin(a_dua, sp[1][q]), gphid += sp[2][q];
  for (int k0 = i + 8 * PICK_Q; k0 < N; k0 += 8 * PICK_Q) {  // (N > 8 PICK_Q)
    double v[3][PICK_Q];
#pragma unroll
    for (int q = 0; q < PICK_Q; q++) {
      const int k = k0 + 8 * q < N ? k0 + 8 * q : k0;
      v[0][q] = PL(W.SP, SP_apri, k, N), v[1][q] = PL(W.SP, SP_adua, k, N), v[2][q] = PL(W.SP, SP_gphid, k, N);
    }
#pragma unroll
    for (int q = 0; q < PICK_Q; q++)
      if (k0 + 8 * q < N) a_pri = fmin(a_pri, v[0][q]), a_dua = fmin(a_dua, v[1][q]), gphid += v[2][q];
  }
  a_pri = grp_min(a_pri), a_dua = grp_min(a_dua), gphid = grp_sum(gphid);
  // c00 = lterm(x_0) is a constant of the solve; kept so that phi matches the oracle's barrier objective
  // filter measures of candidates lA and lB (sums over the horizon of the partials written by k_eval / k_linesearch): the
  // loads of both go out together, a pair of candidates costs one round trip per 8 PICK_Q stages
  auto sums6 = [&](const int lA, const int lB, const int kbeg, double (&s)[6]) {  // adds the stages kbeg, kbeg + 8, ...
    for (int k0 = kbeg; k0 < N; k0 += 8 * PICK_Q) {
      double v[6][PICK_Q];
#pragma unroll
      for (int q = 0; q < PICK_Q; q++) {
        const int k = k0 + 8 * q < N ? k0 + 8 * q : k0;
#pragma unroll
        for (int f = 0; f < 3; f++) v[f][q] = PL(W.LS, 3 * lA + f, k, N), v[3 + f][q] = PL(W.LS, 3 * lB + f, k, N);
      }
#pragma unroll
      for (int q = 0; q < PICK_Q; q++)
        if (k0 + 8 * q < N) {
#pragma unroll
          for (int f = 0; f < 6; f++) s[f] += v[f][q];
        }
    }
  };
  auto measures = [&](double (&s)[6], double& thA, double& phA, double& thB, double& phB) {
#pragma unroll
    for (int f = 0; f < 6; f++) s[f] = grp_sum(s[f]);
    thA = s[0], phA = (c00 + s[1]) - mu * s[2], thB = s[3], phB = (c00 + s[4]) - mu * s[5];
  };
  double th0, ph0, th1, ph1;
  {  // the current point and the full step
    double s[6] = {};
#pragma unroll
    for (int q = 0; q < PICK_Q; q++)
      if (i + 8 * q < N) {
#pragma unroll
        for (int f = 0; f < 6; f++) s[f] += ls[f][q];
      }
    sums6(0, 1, i + 8 * PICK_Q, s);  // (N > 8 PICK_Q)
    measures(s, th0, ph0, th1, ph1);
  }
  const bool th_init = theta0 < 0.0;  // first filter test since the filter was reset
  if (th_init) {
    theta0 = th0, theta_max = 1e4 * fmax(1.0, theta0), theta_min = 1e-4 * fmax(1.0, theta0);
    nfilt = 0;
  }
  const double g_th = 1e-5, g_ph = 1e-8, eta_ph = 1e-8, s_th = 1.1, s_ph = 2.3, dlt = 1.0;
  const double S = pen_scale(rho), iS = 1.0 / S;  // penalty scale (layout.h): the objective side of the tests in its units
  bool accepted = false;
  double alpha = a_pri;
  const int n_ls = o.n_linesearch;
  const int n_try = (phase == 0) ? 1 : n_ls;  // phase 1 repeats the test of candidate 0 (same outcome) and goes on
  // what the accepted candidate does to the filter in memory (written with the state at the end): drop the oldest pair,
  // append one at position f_at
  bool f_shift = false;
  int f_at = -1;
  auto try_candidate = [&](const double th, const double ph) -> bool {  // true: accepted (filter updated)
    if (!isfinite(th) || !isfinite(ph) || th > theta_max) return false;
    bool in_filter = false;
#pragma unroll
    for (int f = 0; f < FILTER_MAX; f++) in_filter = in_filter || (f < nfilt && th >= fth[f] && ph >= fph[f]);
    if (in_filter) return false;
    bool sw = (gphid < 0.0) && (alpha * pow(-gphid * iS, s_ph) > dlt * pow(th0, s_th));
    bool armijo = ph <= ph0 + eta_ph * alpha * gphid;
    bool ok;
    if (th0 <= theta_min && sw) ok = armijo;
    else ok = (th <= (1.0 - g_th) * th0) || (ph <= ph0 - g_ph * S * th0);
    if (!ok) return false;
    if (!(sw && armijo)) {  // augment the filter (nobody reads it again in this launch)
      if (nfilt == FILTER_MAX) f_shift = true, nfilt--;
      f_at = nfilt;
      nfilt++;
    }
    return true;
  };
  // candidate l + 1 has alpha = a_pri 2^-l; candidates are measured in pairs (the first one came with the current point)
  accepted = try_candidate(th1, ph1);
  if (!accepted) alpha *= 0.5;
  for (int l = 1; l < n_try && !accepted; l += 2) {
    double thA, phA, thB, phB;
    double s[6] = {};
    sums6(l + 1, l + 2 <= n_ls ? l + 2 : l + 1, i, s);
    measures(s, thA, phA, thB, phB);
    accepted = try_candidate(thA, phA);
    if (!accepted) {
      alpha *= 0.5;
      if (l + 1 < n_try) {
        accepted = try_candidate(thB, phB);
        if (!accepted) alpha *= 0.5;
      }
    }
  }
  if (i != 0) return;  // one writer per instance from here on
  if (phase == 0 && !accepted && n_ls > 1) {  // nothing has been modified yet: phase 1 decides
    STI(SI_LSMORE) = 1;
    if (th_init) STD(ST_THETA0) = theta0, STD(ST_THMAX) = theta_max, STD(ST_THMIN) = theta_min;
    if (append_list) W.ls_list[atomicAdd(W.ls_count, 1)] = b;
    return;
  }
  // Restoration phase (IPOPT enters its own when the filter line search fails): here an elastic mode, entered once per
  // solve on the first failed search or after stall_iter tiny steps.
  const bool resto_ready = o.resto_rho > 0.0 && !(o.soft_rho > 0.0) && resto == 0;
  bool take = true, give_up = false, enter_resto = false, stalled = false, shift = false;
  bool th_reset = false;  // the filter restarts: theta0 = -1
  if (!accepted) {
    nlsfail += 1;
    const double fr = force_reg;
    if (resto_ready) {
      enter_resto = true, take = false;
    } else if (o.max_ls_fail > 0 && nlsfail >= o.max_ls_fail) {
      give_up = true, take = false;
    } else if (fr < 1e4 * S) {
      force_reg = fr == 0.0 ? 1e-2 * S : fr * 100.0;
      take = false;
    } else {
      nfilt = 0;
      alpha = a_pri * pow(0.5, (double)(n_ls - 1));
    }
  }
  if (give_up) stalled = true;
  if (take) {
    force_reg = 0.0;
    ntiny = alpha <= 1e-3 ? ntiny + 1 : 0;
    if ((o.stall_iter > 0 && ntiny >= o.stall_iter) || (resto_ready && blowup)) {  // (SI_BLOWUP: options.dual_inf_max, set by the head)
      if (resto_ready) enter_resto = true;
      else stalled = true;
      take = false;
    }
  }
  if (enter_resto) {
    // First remedy (options.resto_shift_retry), once per warm-started solve: the jam may be the un-shifted warm start's doing
    // (do_mpc re-uses the previous solution as it is, one interval behind the new measured state).  The solve starts again on the
    // hard constraints from its own starting point moved one interval ahead (options.warm_shift's rule): d_update, the next
    // slot-parallel kernel, loads the shifted point from the backup planes (SI_SHIFT), the next evaluation re-initialises
    // slacks and multipliers (SI_REINIT).  The restoration phase proper follows if that start jams too:
    // the track constraints get elastic variables that cost resto_rho each; equality multipliers, slacks and the barrier
    // parameter start again at the current primal point.
    shift = o.resto_shift_retry && !o.warm_shift && warm && nshift == 0;
    double rho_new = 0.0;
    if (!shift) resto = 1, nresto += 1, rho_new = o.resto_rho;
    rho = rho_new, mu = o.mu_init * pen_scale(rho_new);
    eps_next = (o.smooth_scale > 0 || o.smooth_eps_min > 0) ? fmax(o.smooth_eps_min, o.smooth_scale * o.mu_init) : 0.0;
    if (eps_next == eps) nfilt = 0, th_reset = true;  // (else: reset with the switch of the smoothing below)
    force_reg = 0.0, ntiny = 0;
  }
  if (!stalled) iters += 1;  // (a solve that stops here has completed `iters` iterations, like the oracle)
  // table smoothing follows the barrier parameter with one iteration lag; the filter restarts when it changes
  const bool eps_switched = eps_next != eps;
  if (eps_switched) {
    c00 = cost_eval(inst_params<PI>(K.p, W, b), inst_tables<TS>(K.T, W, b), eps_next, x0, false, nullptr, nullptr);
    nfilt = 0, th_reset = true;
  }
  // ---- the stores, in one group
  STI(SI_LSMORE) = 0;
  if (f_shift) {
#pragma unroll
    for (int f = 0; f + 1 < FILTER_MAX; f++) W.filt[(size_t)(2 * f) * W.Bp + b] = fth[f + 1], W.filt[(size_t)(2 * f + 1) * W.Bp + b] = fph[f + 1];
  }
  if (f_at >= 0) {
    W.filt[(size_t)(2 * f_at) * W.Bp + b] = (1.0 - g_th) * th0;
    W.filt[(size_t)(2 * f_at + 1) * W.Bp + b] = ph0 - g_ph * S * th0;
  }
  if (th_init) STD(ST_THMAX) = theta_max, STD(ST_THMIN) = theta_min;
  if (th_init || th_reset) STD(ST_THETA0) = th_reset ? -1.0 : theta0;
  if (!accepted) STI(SI_NLSFAIL) = nlsfail;
  if (stalled) STI(SI_STATUS) = LTOMPC_STATUS_STALLED, STI(SI_DONE) = 1;
  if (enter_resto) {
    if (shift) STI(SI_SHIFT) = 1, STI(SI_NSHIFT) = 1;
    else STI(SI_RESTO) = resto, STI(SI_NRESTO) = nresto;
    STI(SI_REINIT) = 1;
    STD(ST_RHO) = rho, STD(ST_MU) = mu;
    STD(ST_EPS_NEXT) = eps_next;
    STD(ST_DW_LAST) = 0.0;
    STI(SI_NACC) = 0, STI(SI_SINCEMU) = 0;
  }
  STD(ST_FORCE_REG) = force_reg;
  STI(SI_NTINY) = ntiny;
  STD(ST_ALPHA) = take ? alpha : 0.0, STD(ST_ADUA) = a_dua;
  STI(SI_STEP) = take ? 1 : 0;
  STI(SI_ITERS) = iters;
  if (eps_switched) STD(ST_EPS) = eps_next, STD(ST_C00) = c00;
  STI(SI_NFILT) = nfilt;
  STI(SI_SKIP_EVAL) = (!take && !eps_switched && !enter_resto) ? 1 : 0;  // the iterate did not move: the stage blocks stay valid
}

__global__ void __launch_bounds__(64) k_pick(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, Launch la, int phase) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int count = phase == 0 ? la.nact[0] : W.ls_count[0];
  // (phase 1 is launched for the expected length of the list of rejected steps, longer lists are covered grid-stride;
  //  the 8 lanes of an instance stay together)
  for (int j = blockIdx.x * 8 + g; j < count; j += gridDim.x * 8) d_pick(K, W, phase == 0 ? la.act[j] : W.ls_list[j], i, phase, true);
}
// with per-instance vehicle and cost parameters (W.TH)
__global__ void __launch_bounds__(64) k_pick_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, Launch la, int phase) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int count = phase == 0 ? la.nact[0] : W.ls_count[0];
  // (phase 1 is launched for the expected length of the list of rejected steps, longer lists are covered grid-stride;
  //  the 8 lanes of an instance stay together)
  for (int j = blockIdx.x * 8 + g; j < count; j += gridDim.x * 8) d_pick<true>(K, W, phase == 0 ? la.act[j] : W.ls_list[j], i, phase, true);
}

// ... and per-instance table sets (W.TSV / W.TSI, DESIGN.md §16: d_pick evaluates lterm(x_0) when the smoothing changes)
__global__ void __launch_bounds__(64) k_pick_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, Launch la, int phase) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  const int lane = threadIdx.x, g = lane & 7, i = lane >> 3;
  const int count = phase == 0 ? la.nact[0] : W.ls_count[0];
  // (phase 1 is launched for the expected length of the list of rejected steps, longer lists are covered grid-stride;
  //  the 8 lanes of an instance stay together)
  for (int j = blockIdx.x * 8 + g; j < count; j += gridDim.x * 8) d_pick<true, true>(K, W, phase == 0 ? la.act[j] : W.ls_list[j], i, phase, true);
}

// ------------------------------------------------------------------------------------------ k_update
__device__ __forceinline__ void d_update(const Consts& K, const Work& W, const int k, const int b) {
  const int N = W.N;
  if (W.si[(size_t)SI_SHIFT * W.Bp + b] && !W.si[(size_t)SI_DONE * W.Bp + b]) {
    // options.resto_shift_retry (d_pick): slot k takes the primal point the solve started from, one interval ahead (the last
    // interval repeated): x_{k+1}, c_k, u_k of the backup's slot min(k + 1, N - 1).  Slot-local writes, read-only source.
    const size_t ob = W.orig[b];
    const int ks = k + 1 <= N - 1 ? k + 1 : N - 1;
    double v[18];
#pragma unroll
    for (int f = 0; f < 18; f++) v[f] = W.BK[((size_t)f * N + ks) * W.Bp + ob];
#pragma unroll
    for (int i = 0; i < 8; i++) PL(W.X, i, k + 1, N + 1) = v[i], PL(W.C, i, k, N) = v[8 + i];
    PL(W.U, 0, k, N) = v[16], PL(W.U, 1, k, N) = v[17];
    return;
  }
  if (!W.si[(size_t)SI_STEP * W.Bp + b] || W.si[(size_t)SI_DONE * W.Bp + b]) return;
  const double alpha = W.st[(size_t)ST_ALPHA * W.Bp + b], a_dua = W.st[(size_t)ST_ADUA * W.Bp + b];
  const double mu = W.st[(size_t)ST_MU * W.Bp + b];
  // Loads in batches, stores after them: on gfx9 a load that follows a store waits for the store as well (vmcnt counts
  // both, in order), so "load, update, store" per word is one full memory round trip per word for a lone wavefront
  // (narrow launches: 23 round trips for the inequalities of a slot, 55 k cycles of k_step1's 140 k).
  {
    double x[8], dx[8], c[8], dc[8], l1[8], n1[8], l2[8], n2[8], u[2], du[2];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      x[i] = PL(W.X, i, k + 1, N + 1), dx[i] = PL(W.dX, i, k + 1, N + 1), c[i] = PL(W.C, i, k, N), dc[i] = PL(W.dC, i, k, N);
      l1[i] = PL(W.L1, i, k, N), n1[i] = PL(W.nL1, i, k, N), l2[i] = PL(W.L2, i, k, N), n2[i] = PL(W.nL2, i, k, N);
    }
    u[0] = PL(W.U, 0, k, N), u[1] = PL(W.U, 1, k, N), du[0] = PL(W.dU, 0, k, N), du[1] = PL(W.dU, 1, k, N);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      PL(W.X, i, k + 1, N + 1) = x[i] + alpha * dx[i];
      PL(W.C, i, k, N) = c[i] + alpha * dc[i];
      PL(W.L1, i, k, N) = l1[i] + alpha * (n1[i] - l1[i]);
      PL(W.L2, i, k, N) = l2[i] + alpha * (n2[i] - l2[i]);
    }
    PL(W.U, 0, k, N) = u[0] + alpha * du[0], PL(W.U, 1, k, N) = u[1] + alpha * du[1];
  }
  const int ni = K.bd.ni, nel = K.bd.nel, nact = (k + 1 <= N - 1) ? ni : ni - 3 - nel;  // (the last slot has no nonlinear constraints)
  for (int m0 = 0; m0 < nact; m0 += 8) {
    double t[8], dt[8], nu[8], dn[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int m = m0 + q < nact ? m0 + q : nact - 1;  // (the last chunk repeats its last word: branch-free loads)
      t[q] = PL(W.T, m, k, N), dt[q] = PL(W.dT, m, k, N), nu[q] = PL(W.NU, m, k, N), dn[q] = PL(W.dNU, m, k, N);
    }
#pragma unroll
    for (int q = 0; q < 8; q++)
      if (m0 + q < nact) {
        const double tn = t[q] + alpha * dt[q];
        const double nn = nu[q] + a_dua * dn[q];
        const double lo = mu / (1e10 * tn), hi = 1e10 * mu / tn;  // IPOPT eq. (16)
        PL(W.T, m0 + q, k, N) = tn, PL(W.NU, m0 + q, k, N) = nn < lo ? lo : (nn > hi ? hi : nn);
      }
  }
  if (W.st[(size_t)ST_RHO * W.Bp + b] > 0.0 && nact == ni) {  // elastic variables
    double e[3], de[3];
#pragma unroll
    for (int q = 0; q < 3; q++) e[q] = PL(W.T, ni + q, k, N), de[q] = PL(W.dT, ni + q, k, N);
#pragma unroll
    for (int q = 0; q < 3; q++) PL(W.T, ni + q, k, N) = e[q] + alpha * de[q];
  }
  if (nel && nact == ni) {  // ... of the friction-ellipse constraints
    double e[2], de[2];
#pragma unroll
    for (int q = 0; q < 2; q++) e[q] = PL(W.T, ni + 3 + q, k, N), de[q] = PL(W.dT, ni + 3 + q, k, N);
#pragma unroll
    for (int q = 0; q < 2; q++) PL(W.T, ni + 3 + q, k, N) = e[q] + alpha * de[q];
  }
}

__global__ void __launch_bounds__(64) k_update(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, Launch la) {
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid == 0) W.ls_count[1] = W.ls_count[0], W.ls_count[0] = 0;  // both line-search phases of this iteration are over ([1]: the host sizes the next phase-1 launches by it)
  int j = tid % la.n_pad, k = tid / la.n_pad;
  if (k >= W.N || j >= la.nact[0]) return;
  d_update(K, W, k, la.act[j]);
}

// ------------------------------------------------------------------------------------------ the update of k_step1, split
// d_update as k_step1 runs it is one wavefront's work: N lanes, a whole slot each, a dozen dependent round trips while 280 lanes
// idle - and before it d_pick, 8 lanes.  None of the update's operands depends on d_pick (which writes W.st, W.si, W.filt and
// ls_list only), so wavefronts 1..4 fetch them WHILE d_pick runs (d_update_fetch) and after the barrier only the seven state
// words are a round trip away (d_update_store).  Lane w = tid - 64 owns row r = w & 7 of the slots (w >> 3) + 32 j: the pairs
// (x_r, dx_r) of node k + 1, (c_r, dc_r), (l1_r, n1_r), (l2_r, n2_r), (u_r, du_r) for r < 2, the elastic pair (e_r, de_r) for
// r < 3 + nel, and the inequality units (t_m, dt_m, nu_m, dn_m), m = r + 8 q - whole units, every word formed by d_update's own
// statement.  Within a slot the loads are unconditional with clamped indices (d_update's idiom), the conditions apply to the stores.
constexpr int UPD_ROUNDS = 2;  // rounds of 32 slots held across the pick: N <= 64 (N = 40 entirely); later slots are loaded after it
constexpr int UPD_QUADS = 3;   // inequality units of a row held with them: ni <= 24 (the reference's bound pattern: at most 23)
struct UpdRow {
  double a[5], d[5], e, de;                                              // x, c, l1, l2, u and their steps / trial values; elastic
  double t[UPD_QUADS], dt[UPD_QUADS], nu[UPD_QUADS], dn[UPD_QUADS];      // inequalities m0 + r + 8 q
};
struct UpdRegs {
  UpdRow row[UPD_ROUNDS];
};

__device__ __forceinline__ void upd_load_pairs(const Consts& K, const Work& W, const int k, const int r, const int b, UpdRow& v) {
  const int N = W.N, ni = K.bd.ni, nel = K.bd.nel;
  const int ru = r < 2 ? r : 1, re = ni + (r < 3 + nel ? r : 0);  // (rows without such a unit repeat another's word: branch-free loads)
  v.a[0] = PL(W.X, r, k + 1, N + 1), v.d[0] = PL(W.dX, r, k + 1, N + 1), v.a[1] = PL(W.C, r, k, N), v.d[1] = PL(W.dC, r, k, N);
  v.a[2] = PL(W.L1, r, k, N), v.d[2] = PL(W.nL1, r, k, N), v.a[3] = PL(W.L2, r, k, N), v.d[3] = PL(W.nL2, r, k, N);
  v.a[4] = PL(W.U, ru, k, N), v.d[4] = PL(W.dU, ru, k, N);
  v.e = PL(W.T, re, k, N), v.de = PL(W.dT, re, k, N);
}
__device__ __forceinline__ void upd_load_quads(const Consts& K, const Work& W, const int k, const int r, const int b, const int m0, UpdRow& v) {
  const int N = W.N, ni = K.bd.ni, nel = K.bd.nel, nact = (k + 1 <= N - 1) ? ni : ni - 3 - nel;  // (the last slot has no nonlinear constraints)
  const int last = nact > 0 ? nact - 1 : 0;
#pragma unroll
  for (int q = 0; q < UPD_QUADS; q++) {
    const int m = m0 + r + 8 * q < nact ? m0 + r + 8 * q : last;
    v.t[q] = PL(W.T, m, k, N), v.dt[q] = PL(W.dT, m, k, N), v.nu[q] = PL(W.NU, m, k, N), v.dn[q] = PL(W.dNU, m, k, N);
  }
}
__device__ __forceinline__ void upd_store_pairs(const Consts& K, const Work& W, const int k, const int r, const int b, const double alpha,
                                                const double rho, const UpdRow& v) {
  const int N = W.N, ni = K.bd.ni, nel = K.bd.nel;
  PL(W.X, r, k + 1, N + 1) = v.a[0] + alpha * v.d[0];
  PL(W.C, r, k, N) = v.a[1] + alpha * v.d[1];
  PL(W.L1, r, k, N) = v.a[2] + alpha * (v.d[2] - v.a[2]);
  PL(W.L2, r, k, N) = v.a[3] + alpha * (v.d[3] - v.a[3]);
  if (r < 2) PL(W.U, r, k, N) = v.a[4] + alpha * v.d[4];
  // elastic variables (of the track constraints with rho > 0, of the friction ellipse with nel), not in the last slot
  if (k + 1 <= N - 1 && (r < 3 ? rho > 0.0 : r < 3 + nel)) PL(W.T, ni + r, k, N) = v.e + alpha * v.de;
}
__device__ __forceinline__ void upd_store_quads(const Consts& K, const Work& W, const int k, const int r, const int b, const int m0,
                                                const double alpha, const double a_dua, const double mu, const UpdRow& v) {
  const int N = W.N, ni = K.bd.ni, nel = K.bd.nel, nact = (k + 1 <= N - 1) ? ni : ni - 3 - nel;
#pragma unroll
  for (int q = 0; q < UPD_QUADS; q++)
    if (m0 + r + 8 * q < nact) {
      const double tn = v.t[q] + alpha * v.dt[q];
      const double nn = v.nu[q] + a_dua * v.dn[q];
      const double lo = mu / (1e10 * tn), hi = 1e10 * mu / tn;  // IPOPT eq. (16)
      PL(W.T, m0 + r + 8 * q, k, N) = tn, PL(W.NU, m0 + r + 8 * q, k, N) = nn < lo ? lo : (nn > hi ? hi : nn);
    }
}

// ... and with the line search's operands staged (StepStage::whole): of a row's 24 words the planes give the 10 that the line
// search does not read - the multiplier pairs and (nu_m, dn_m) - and the window the other 14, through the same clamped indices.
__device__ __forceinline__ void upd_load_mults(const Consts& K, const Work& W, const int k, const int r, const int b, UpdRow& v) {
  const int N = W.N, ni = K.bd.ni, nel = K.bd.nel, nact = (k + 1 <= N - 1) ? ni : ni - 3 - nel;
  const int last = nact > 0 ? nact - 1 : 0;
  v.a[2] = PL(W.L1, r, k, N), v.d[2] = PL(W.nL1, r, k, N), v.a[3] = PL(W.L2, r, k, N), v.d[3] = PL(W.nL2, r, k, N);
#pragma unroll
  for (int q = 0; q < UPD_QUADS; q++) {
    const int m = r + 8 * q < nact ? r + 8 * q : last;
    v.nu[q] = PL(W.NU, m, k, N), v.dn[q] = PL(W.dNU, m, k, N);
  }
}
__device__ __forceinline__ void upd_take_staged(const Consts& K, const Work& W, const StepStage& S, const int k, const int r, const int b, UpdRow& v) {
  const int N = W.N, ni = K.bd.ni, nel = K.bd.nel, nact = (k + 1 <= N - 1) ? ni : ni - 3 - nel;
  const int last = nact > 0 ? nact - 1 : 0;
  const int ru = r < 2 ? r : 1, re = ni + (r < 3 + nel ? r : 0);
  v.a[0] = S.X(W, b, N, r, k + 1), v.d[0] = S.dX(W, b, N, r, k + 1), v.a[1] = S.C(W, b, N, r, k), v.d[1] = S.dC(W, b, N, r, k);
  v.a[4] = S.U(W, b, N, ru, k), v.d[4] = S.dU(W, b, N, ru, k);
  v.e = S.T(W, b, N, re, k), v.de = S.dT(W, b, N, re, k);
#pragma unroll
  for (int q = 0; q < UPD_QUADS; q++) {
    const int m = r + 8 * q < nact ? r + 8 * q : last;
    v.t[q] = S.T(W, b, N, m, k), v.dt[q] = S.dT(W, b, N, m, k);
  }
}

// wavefronts 1..4, beside d_pick: the operands of the first UPD_ROUNDS * 32 slots, one batch
__device__ __forceinline__ void d_update_fetch(const Consts& K, const Work& W, const StepStage& S, const int tid, const int b, UpdRegs& R) {
  const int N = W.N, w = tid - 64;
#pragma unroll
  for (int j = 0; j < UPD_ROUNDS; j++) {
    // (a round past the horizon is skipped, not clamped: at N = 40 that is the second round of wavefronts 2..4, whole wavefronts,
    //  and their 4600 repeated loads made the fetch longer than the pick it runs beside - the workgroup's loads go through one
    //  cache port, a 64-byte sector per lane and load)
    const int k = 32 * j + (w >> 3);
    if (k < N) {
      if (S.whole()) upd_load_mults(K, W, k, w & 7, b, R.row[j]);
      else upd_load_pairs(K, W, k, w & 7, b, R.row[j]), upd_load_quads(K, W, k, w & 7, b, 0, R.row[j]);
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // in registers HERE, while the pick runs: not sunk to the stores behind the barrier
#pragma unroll
  for (int j = 0; j < UPD_ROUNDS; j++) {
    UpdRow& v = R.row[j];
    asm volatile("" : "+v"(v.a[0]), "+v"(v.d[0]), "+v"(v.a[1]), "+v"(v.d[1]), "+v"(v.a[2]), "+v"(v.d[2]), "+v"(v.a[3]), "+v"(v.d[3]),
                 "+v"(v.a[4]), "+v"(v.d[4]), "+v"(v.e), "+v"(v.de));
    asm volatile("" : "+v"(v.t[0]), "+v"(v.dt[0]), "+v"(v.nu[0]), "+v"(v.dn[0]), "+v"(v.t[1]), "+v"(v.dt[1]), "+v"(v.nu[1]), "+v"(v.dn[1]),
                 "+v"(v.t[2]), "+v"(v.dt[2]), "+v"(v.nu[2]), "+v"(v.dn[2]));
  }
#endif
}

// all wavefronts, after the pick: the state it left, one round trip, then the stores
// (whole: the words of X, dX, C, dC, U, dU, T, dT come from the window.  Nothing has written them in the planes since they were
//  staged: d_linesearch stores to W.LS only and d_pick to W.st, W.si, W.filt and ls_list only, and the stores below are this
//  kernel's first to the iterate.)
__device__ __forceinline__ void d_update_store(const Consts& K, const Work& W, const StepStage& S, const int tid, const int b, UpdRegs& R) {
  const int N = W.N;
  int shift = W.si[(size_t)SI_SHIFT * W.Bp + b], done = W.si[(size_t)SI_DONE * W.Bp + b], step = W.si[(size_t)SI_STEP * W.Bp + b];
  double alpha = W.st[(size_t)ST_ALPHA * W.Bp + b], a_dua = W.st[(size_t)ST_ADUA * W.Bp + b];
  double mu = W.st[(size_t)ST_MU * W.Bp + b], rho = W.st[(size_t)ST_RHO * W.Bp + b];
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(shift), "+v"(done), "+v"(step), "+v"(alpha), "+v"(a_dua), "+v"(mu), "+v"(rho));
#endif
  if (shift && !done) {  // options.resto_shift_retry, rare: the point comes from the backup planes (d_update)
    for (int kk = tid; kk < N; kk += 320) {
#if defined(__clang__)
      // (the flags as d_update reads them next: its other branch is not compiled in a second time)
      __builtin_assume(W.si[(size_t)SI_SHIFT * W.Bp + b] && !W.si[(size_t)SI_DONE * W.Bp + b]);
#endif
      d_update(K, W, kk, b);
    }
    return;
  }
  if (!step || done || tid < 64) return;
  const int w = tid - 64, r = w & 7;
#pragma unroll
  for (int j = 0; j < UPD_ROUNDS; j++) {
    const int k = 32 * j + (w >> 3);
    if (k < N) {
      if (S.whole()) upd_take_staged(K, W, S, k, r, b, R.row[j]);
      upd_store_pairs(K, W, k, r, b, alpha, rho, R.row[j]), upd_store_quads(K, W, k, r, b, 0, alpha, a_dua, mu, R.row[j]);
    }
  }
  // what was not held: slots from UPD_ROUNDS * 32 on, inequalities from UPD_QUADS * 8 on - load a batch, then store it
  const int ni = K.bd.ni;
  if (N <= UPD_ROUNDS * 32 && ni <= UPD_QUADS * 8) return;
  for (int k = w >> 3; k < N; k += 32) {
    UpdRow v;
    if (k >= UPD_ROUNDS * 32) {
      upd_load_pairs(K, W, k, r, b, v), upd_load_quads(K, W, k, r, b, 0, v);
      upd_store_pairs(K, W, k, r, b, alpha, rho, v), upd_store_quads(K, W, k, r, b, 0, alpha, a_dua, mu, v);
    }
    for (int m0 = UPD_QUADS * 8; m0 < ni; m0 += UPD_QUADS * 8) {
      upd_load_quads(K, W, k, r, b, m0, v);
      upd_store_quads(K, W, k, r, b, m0, alpha, a_dua, mu, v);
    }
  }
}


// ------------------------------------------------------------------------------------------ k_step1's staging
// The view of the workgroup's array for this handle's horizon and bound pattern (block-uniform).
__device__ __forceinline__ StepStage step_stage(const Consts& K, const Work& W, double* s) {
  StepStage S;
  S.s = s, S.N = W.N, S.R = K.bd.ni + NNL + K.bd.nel;
  S.stride = stage_stride(S.R), S.ks = stage_cols(S.N, S.R) - 1, S.k0 = 0;
  return S;
}
// All 320 lanes: the window of the slots k0 .. k0 + cnt - 1 into LDS, each word loaded once.  Lane tid owns column
// col = tid % (cnt + 1) of the rows tid / (cnt + 1) + j * rpp of every array, rpp = 320 / (cnt + 1) rows of lanes (at N = 40: 7, 287
// lanes at work; stage_cols keeps rpp >= 2, so an array of 8 rows is at most 4 passes).  Per array and pass the row is the same
// expression in every lane - no pointer is selected per lane - and a lane without a word (past the array's last row, in the last
// column of an array of slots, in the partial last row of lanes) loads nothing: a pass without lanes is a branch taken.  The loads
// of X, dX, C, dC, U, dU, of the first STG_TQ passes of T and dT, of eps, rho and the partials are ONE batch, in registers before
// the first write; further passes of T and dT (more than STG_TQ * rpp rows: at N = 40 none) follow batch by batch.  eps, rho and
// the N partials SP_apri go with the first window and stay for the later ones.  The caller's barriers stand between this and the
// readers, and between the readers and the next window.
constexpr int STG_TQ = 4;
__device__ __forceinline__ void d_step1_stage(const Work& W, const StepStage& S, const int tid, const int b, const int cnt) {
  const int N = S.N, R = S.R, c1 = cnt + 1, rpp = 320 / c1;
  const int row0 = tid / c1, col = tid - row0 * c1, kn = S.k0 + col;
  const bool lane = row0 < rpp, slotc = lane && col < cnt, first = S.k0 == 0;
  double* const dst = S.s + 2 + N + col * S.stride;
  double x[4] = {}, dx[4] = {}, c[4] = {}, dc[4] = {}, u = 0.0, du = 0.0, t[STG_TQ] = {}, dt[STG_TQ] = {}, ap = 0.0, er = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = row0 + j * rpp;
    if (lane && r < 8) {  // column = node; node 0 of X is the measured state
      if (kn == 0) x[j] = W.x0[(size_t)r * W.Bp + b];
      else x[j] = PL(W.X, r, kn, N + 1);
      dx[j] = PL(W.dX, r, kn, N + 1);
    }
    if (slotc && r < 8) c[j] = PL(W.C, r, kn, N), dc[j] = PL(W.dC, r, kn, N);
  }
  if (lane && row0 < 2) {  // column = slot + 1; slot -1 of U is the applied input, its step 0
    if (kn == 0) u = W.uprev[(size_t)row0 * W.Bp + b];
    else u = PL(W.U, row0, kn - 1, N), du = PL(W.dU, row0, kn - 1, N);
  }
  const auto load_t = [&](const int rb) {
#pragma unroll
    for (int j = 0; j < STG_TQ; j++) {
      const int r = rb + row0 + j * rpp;
      if (slotc && r < R) t[j] = PL(W.T, r, kn, N), dt[j] = PL(W.dT, r, kn, N);
    }
  };
  load_t(0);
  if (first && tid < N) ap = PL(W.SP, SP_apri, tid, N);
  if (first && tid >= 318) er = W.st[(size_t)(tid == 318 ? ST_EPS : ST_RHO) * W.Bp + b];
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(dx[0]), "+v"(dx[1]), "+v"(dx[2]), "+v"(dx[3]), "+v"(c[0]), "+v"(c[1]),
                    "+v"(c[2]), "+v"(c[3]), "+v"(dc[0]), "+v"(dc[1]), "+v"(dc[2]), "+v"(dc[3]), "+v"(u), "+v"(du), "+v"(t[0]), "+v"(t[1]),
                    "+v"(t[2]), "+v"(t[3]), "+v"(dt[0]), "+v"(dt[1]), "+v"(dt[2]), "+v"(dt[3]), "+v"(ap), "+v"(er));
#endif
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = row0 + j * rpp;
    if (lane && r < 8) dst[SG_X + 2 * r] = x[j], dst[SG_X + 2 * r + 1] = dx[j];
    if (slotc && r < 8) dst[SG_C + 2 * r] = c[j], dst[SG_C + 2 * r + 1] = dc[j];
  }
  if (lane && row0 < 2) dst[SG_U + 2 * row0] = u, dst[SG_U + 2 * row0 + 1] = du;
  if (first && tid < N) S.s[2 + tid] = ap;
  if (first && tid >= 318) S.s[tid - 318] = er;
  for (int rb = 0;;) {
#pragma unroll
    for (int j = 0; j < STG_TQ; j++) {
      const int r = rb + row0 + j * rpp;
      if (slotc && r < R) dst[SG_T + 2 * r] = t[j], dst[SG_T + 2 * r + 1] = dt[j];
    }
    if ((rb += STG_TQ * rpp) >= R) break;
    load_t(rb);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(dt[0]), "+v"(dt[1]), "+v"(dt[2]), "+v"(dt[3]));
#endif
  }
  if (first)
    for (int kk = tid + 320; kk < N; kk += 320) S.s[2 + kk] = PL(W.SP, SP_apri, kk, N);  // (horizons beyond 320)
}
static_assert(STG_TQ == 4, "the register pins of d_step1_stage name 4 passes of T and dT");

// ------------------------------------------------------------------------------------------ k_step1
// Narrow launches: the whole step selection of ONE instance per workgroup (both line-search phases, the filter test
// and the update), i.e. five dependent launches of 10..30 us each in one.  Same device functions, same numbers.
template <class BP, bool ELL>
__global__ void __launch_bounds__(320) k_step1(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, Launch la) {  // 320 = 8 candidates x 40 intervals in one pass
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  if ((int)blockIdx.x >= la.nact[0]) return;
  const int b = la.act[blockIdx.x];
  const int N = W.N, tid = threadIdx.x;
  const int* si = W.si;
  if (si[(size_t)SI_DONE * W.Bp + b] || !si[(size_t)SI_STEP * W.Bp + b]) return;  // block-uniform
  // all step candidates at once (the threads are there anyway; the wide path evaluates candidates 2.. only for the
  // instances that rejected the full step, with the same arithmetic)
  // LTOMPC_DBG: shader-clock cycles of block 0 per section (own line search, all line searches, pick, update), slots 8..12
  const bool rprof = W.DBG != nullptr && blockIdx.x == 0 && tid == 0;
  long long rt0 = rprof ? clock64() : 0;
#define STOCK(q) if (rprof) { const long long t1 = clock64(); W.DBG[q] += (double)(t1 - rt0); rt0 = t1; }
  // ... from the instance's operands staged in LDS, a window of slots at a time (StepStage; N = 40: one window, read again by
  // the update).  Section 8 of the clocks is the staging and the line search together.
  __shared__ double stg[STG_WORDS];
  StepStage S = step_stage(K, W, stg);
  for (;;) {
    const int cnt = N - S.k0 < S.ks ? N - S.k0 : S.ks;
    d_step1_stage(W, S, tid, b, cnt);
    __syncthreads();
    for (int idx = tid; idx < cnt * K.o.n_linesearch; idx += 320) d_linesearch<BP, false, ELL>(K, W, S.k0 + idx % cnt, b, 1 + idx / cnt, 1 + idx / cnt, S);
    if (S.k0 + cnt >= N) break;
    __syncthreads();  // (the window's readers are through before the next one is written)
    S.k0 += cnt;
  }
  STOCK(8);
  __syncthreads();
  STOCK(9);
  // (phase 1 of the filter test starts with the test of the full step, i.e. it is phase 0 followed by phase 1 when the
  //  measures of all candidates exist already: one pass, same decisions)
  // ... on 8 lanes of wavefront 0; the other wavefronts fetch the operands of the update meanwhile (d_update_fetch: nothing of
  // them is held across the pick by wavefront 0, whose batch of loads needs the registers); what the window holds is read from
  // it after the barrier (d_update_store)
  UpdRegs upd;
  if (tid < 64) {
    if ((tid & 7) == 0) d_pick(K, W, b, tid >> 3, 1, false);
  } else d_update_fetch(K, W, S, tid, b, upd);
  __syncthreads();
  STOCK(10);
  d_update_store(K, W, S, tid, b, upd);
  STOCK(11);
  if (rprof) W.DBG[12] += 1.0;
#undef STOCK
}
// with per-instance vehicle and cost parameters (W.TH).  The body is k_step1's, with the _pi device functions
// (tests/test_instance_params_resources.py checks that the two texts agree): moved into a shared __device__ function, it
// changed the instructions of the uniform k_step1 (register allocation, SGPR spills).
template <class BP>
__global__ void __launch_bounds__(320) k_step1_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, Launch la) {  // 320 = 8 candidates x 40 intervals in one pass
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  if ((int)blockIdx.x >= la.nact[0]) return;
  const int b = la.act[blockIdx.x];
  const int N = W.N, tid = threadIdx.x;
  const int* si = W.si;
  if (si[(size_t)SI_DONE * W.Bp + b] || !si[(size_t)SI_STEP * W.Bp + b]) return;  // block-uniform
  // all step candidates at once (the threads are there anyway; the wide path evaluates candidates 2.. only for the
  // instances that rejected the full step, with the same arithmetic)
  // LTOMPC_DBG: shader-clock cycles of block 0 per section (own line search, all line searches, pick, update), slots 8..12
  const bool rprof = W.DBG != nullptr && blockIdx.x == 0 && tid == 0;
  long long rt0 = rprof ? clock64() : 0;
#define STOCK(q) if (rprof) { const long long t1 = clock64(); W.DBG[q] += (double)(t1 - rt0); rt0 = t1; }
  // ... from the instance's operands staged in LDS, a window of slots at a time (StepStage; N = 40: one window, read again by
  // the update).  Section 8 of the clocks is the staging and the line search together.
  __shared__ double stg[STG_WORDS];
  StepStage S = step_stage(K, W, stg);
  for (;;) {
    const int cnt = N - S.k0 < S.ks ? N - S.k0 : S.ks;
    d_step1_stage(W, S, tid, b, cnt);
    __syncthreads();
    for (int idx = tid; idx < cnt * K.o.n_linesearch; idx += 320) d_linesearch<BP, false, false, true>(K, W, S.k0 + idx % cnt, b, 1 + idx / cnt, 1 + idx / cnt, S);
    if (S.k0 + cnt >= N) break;
    __syncthreads();  // (the window's readers are through before the next one is written)
    S.k0 += cnt;
  }
  STOCK(8);
  __syncthreads();
  STOCK(9);
  // (phase 1 of the filter test starts with the test of the full step, i.e. it is phase 0 followed by phase 1 when the
  //  measures of all candidates exist already: one pass, same decisions)
  // ... on 8 lanes of wavefront 0; the other wavefronts fetch the operands of the update meanwhile (d_update_fetch: nothing of
  // them is held across the pick by wavefront 0, whose batch of loads needs the registers); what the window holds is read from
  // it after the barrier (d_update_store)
  UpdRegs upd;
  if (tid < 64) {
    if ((tid & 7) == 0) d_pick<true>(K, W, b, tid >> 3, 1, false);
  } else d_update_fetch(K, W, S, tid, b, upd);
  __syncthreads();
  STOCK(10);
  d_update_store(K, W, S, tid, b, upd);
  STOCK(11);
  if (rprof) W.DBG[12] += 1.0;
#undef STOCK
}
// ... and per-instance table sets (W.TSV / W.TSI): once more the body of k_step1, with the _ts device functions
// (tests/test_table_sets_resources.py checks the text).
template <class BP>
__global__ void __launch_bounds__(320) k_step1_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, Launch la) {  // 320 = 8 candidates x 40 intervals in one pass
  const Consts& K = *Kp;  // K and W live in device memory: fields are fetched where they are used instead of
  const Work& W = *Wp;    // occupying (spilled) SGPRs for the whole kernel
  if ((int)blockIdx.x >= la.nact[0]) return;
  const int b = la.act[blockIdx.x];
  const int N = W.N, tid = threadIdx.x;
  const int* si = W.si;
  if (si[(size_t)SI_DONE * W.Bp + b] || !si[(size_t)SI_STEP * W.Bp + b]) return;  // block-uniform
  // all step candidates at once (the threads are there anyway; the wide path evaluates candidates 2.. only for the
  // instances that rejected the full step, with the same arithmetic)
  // LTOMPC_DBG: shader-clock cycles of block 0 per section (own line search, all line searches, pick, update), slots 8..12
  const bool rprof = W.DBG != nullptr && blockIdx.x == 0 && tid == 0;
  long long rt0 = rprof ? clock64() : 0;
#define STOCK(q) if (rprof) { const long long t1 = clock64(); W.DBG[q] += (double)(t1 - rt0); rt0 = t1; }
  // ... from the instance's operands staged in LDS, a window of slots at a time (StepStage; N = 40: one window, read again by
  // the update).  Section 8 of the clocks is the staging and the line search together.
  __shared__ double stg[STG_WORDS];
  StepStage S = step_stage(K, W, stg);
  for (;;) {
    const int cnt = N - S.k0 < S.ks ? N - S.k0 : S.ks;
    d_step1_stage(W, S, tid, b, cnt);
    __syncthreads();
    for (int idx = tid; idx < cnt * K.o.n_linesearch; idx += 320) d_linesearch<BP, false, false, true, true>(K, W, S.k0 + idx % cnt, b, 1 + idx / cnt, 1 + idx / cnt, S);
    if (S.k0 + cnt >= N) break;
    __syncthreads();  // (the window's readers are through before the next one is written)
    S.k0 += cnt;
  }
  STOCK(8);
  __syncthreads();
  STOCK(9);
  // (phase 1 of the filter test starts with the test of the full step, i.e. it is phase 0 followed by phase 1 when the
  //  measures of all candidates exist already: one pass, same decisions)
  // ... on 8 lanes of wavefront 0; the other wavefronts fetch the operands of the update meanwhile (d_update_fetch: nothing of
  // them is held across the pick by wavefront 0, whose batch of loads needs the registers); what the window holds is read from
  // it after the barrier (d_update_store)
  UpdRegs upd;
  if (tid < 64) {
    if ((tid & 7) == 0) d_pick<true, true>(K, W, b, tid >> 3, 1, false);
  } else d_update_fetch(K, W, S, tid, b, upd);
  __syncthreads();
  STOCK(10);
  d_update_store(K, W, S, tid, b, upd);
  STOCK(11);
  if (rprof) W.DBG[12] += 1.0;
#undef STOCK
}



}  // namespace ltompc
