// jvp_harness.cpp — TEST INFRASTRUCTURE: k_jvp_sweep / k_jvp_sweep_pi (csrc/jvp.h) compiled as host C++ and run on the lock-step
// 64-lane wavefront of hip_shim.h under AddressSanitizer + UndefinedBehaviorSanitizer.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// No solve: the stage blocks, the Riccati blocks, the PV planes, U, u_prev, ok and a non-identity orig are seeded, well-conditioned
// data (Huu positive definite) in buffers of exactly the size the kernel may touch, filled with NaN bit patterns wherever the kernel
// has no business reading.  Cases: B = 13 and 61 (padding lanes), N = 2 and 10, both kernels, with and without dtheta.  Each is
// compared with a plain serial restatement of the recursion (long double, natural arrays) and checked for exact zeros where ok = 0.
// The restatement follows the same formulas as the kernel: it checks the wavefront mechanics (the row exchange through LDS, the
// grp_sum reductions, padding lanes, orig, the kff planes, the ok zeros, every address), not the mathematics, which
// tests/test_gpu_jvp.py (against forward mode) and tests/test_jvp_reference.py (dense) check independently.
// Prints one line per case and `max_rel <value>`; exit status 1 when a check fails.  Nothing in the package uses this file.
#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"
#include "eval8.h"
#include "jvp.h"

#include <cmath>
#include <random>
#include <type_traits>
#include <vector>

using namespace ltompc;

// The largest |kernel - serial| / max(1, max |serial|) per instance over all cases, measured with this program (g++ -O1, x86-64):
// 8.04e-16 (B = 61, N = 10, k_jvp_sweep_pi with dtheta).  The bound is 10 x that.
static const double REL_BOUND = 8.04e-15;

static double* poisoned(size_t n) {
  double* p = (double*)malloc(n * sizeof(double));
  memset(p, 0xFF, n * sizeof(double));
  return p;
}
template <typename F>
static void wave64(const char* name, int blocks, F&& body) {
  blockDim.x = 64, gridDim.x = blocks;
  for (int blk = 0; blk < blocks; blk++) {
    blockIdx.x = blk;
    LtWave::self().run(name, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, &body);
  }
}

struct Stage {  // one instance, one stage: natural arrays
  double A[8][8], Bm[8][2], R[3], P[8][8], Pxv[8][2], K[2][8], Kv[2][2], PV[PV_NF], U[2];
};

static int run_case(const int B, const int N, const bool PI, const bool TH, std::mt19937_64& rng, double& worst) {
  const int Bp = (B + 63) / 64 * 64;
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  // ---- the data, per slot b and stage k (P, Pxv of stage k are those the sweep stored at node k: k = 0 is never read)
  std::vector<std::vector<Stage>> S(B, std::vector<Stage>(N + 1));
  for (int b = 0; b < B; b++)
    for (int k = 0; k <= N; k++) {
      Stage& s = S[b][k];
      double M[8][8];
      for (int i = 0; i < 8; i++)
        for (int l = 0; l < 8; l++) s.A[i][l] = (i == l ? 0.9 : 0.0) + 0.05 * uni(rng), M[i][l] = uni(rng);
      for (int i = 0; i < 8; i++)
        for (int l = 0; l < 8; l++) {
          double v = i == l ? 1.0 : 0.0;
          for (int m = 0; m < 8; m++) v += 0.1 * M[i][m] * M[l][m];
          s.P[i][l] = v;
        }
      for (int i = 0; i < 8; i++)
        for (int c = 0; c < 2; c++) s.Bm[i][c] = 0.3 * uni(rng), s.Pxv[i][c] = 0.05 * uni(rng), s.K[c][i] = 0.1 * uni(rng);
      s.R[0] = 1.0 + 0.5 * uni(rng), s.R[1] = 0.1 * uni(rng), s.R[2] = 1.0 + 0.5 * uni(rng);
      for (int c = 0; c < 2; c++)
        for (int e = 0; e < 2; e++) s.Kv[c][e] = 0.1 * uni(rng);
      for (int f = 0; f < PV_NF; f++) s.PV[f] = uni(rng);
      s.U[0] = 0.3 * uni(rng), s.U[1] = uni(rng);
    }
  std::vector<int> orig(B);  // slot -> caller's index: a permutation that is not the identity
  for (int b = 0; b < B; b++) orig[b] = (5 * b + 3) % B;  // (5 is coprime to 13 and 61)
  std::vector<double> uprev(2 * (size_t)B), dp(JVP_NP * (size_t)B), dth(PS_NT * (size_t)B), rdu(2 * (size_t)B);
  std::vector<int> ok(B);
  for (int o = 0; o < B; o++) {
    ok[o] = o % 5 != 2;
    uprev[2 * o] = 0.3 * uni(rng), uprev[2 * o + 1] = uni(rng);
    for (int c = 0; c < JVP_NP; c++) dp[(size_t)o * JVP_NP + c] = uni(rng);
    for (int c = 0; c < PS_NT; c++) dth[(size_t)o * PS_NT + c] = uni(rng);
    rdu[2 * o] = 0.01 * (1.5 + uni(rng)), rdu[2 * o + 1] = 0.01 * (1.5 + uni(rng));
  }
  const double r0 = 0.013, r1 = 0.021;  // (the uniform kernel's r_du)
  // ---- the kernel's buffers: exact sizes, NaN wherever nothing was put
  WorkPI W{};
  W.N = N, W.B = B, W.Bp = Bp;
  double *QP = poisoned((size_t)QP_NF * (N + 1) * Bp), *RC = poisoned((size_t)RC_NF * (N + 1) * Bp), *PV = poisoned((size_t)PV_NF * N * Bp);
  double *Upl = poisoned((size_t)2 * N * Bp), *THp = poisoned((size_t)PS_NT * Bp), *JV = poisoned((size_t)JV_NF * N * Bp);
  double *tX = poisoned((size_t)B * (N + 1) * 8), *tU = poisoned((size_t)B * N * 2);
  double* uprev_x = poisoned(2 * (size_t)B);
  memcpy(uprev_x, uprev.data(), sizeof(double) * 2 * B);
  int* orig_x = (int*)malloc(sizeof(int) * B);
  int* ok_x = (int*)malloc(sizeof(int) * B);
  double *dp_x = poisoned(dp.size()), *dth_x = poisoned(dth.size());
  memcpy(orig_x, orig.data(), sizeof(int) * B), memcpy(ok_x, ok.data(), sizeof(int) * B);
  memcpy(dp_x, dp.data(), sizeof(double) * dp.size()), memcpy(dth_x, dth.data(), sizeof(double) * dth.size());
  for (int b = 0; b < B; b++) {
    for (int k = 0; k <= N; k++) {
      const Stage& s = S[b][k];
      if (k < N) {
        for (int i = 0; i < 8; i++)
          for (int l = 0; l < 8; l++) PG(QP, QP_A + i * 8 + l, k, QP_NF) = s.A[i][l];
        for (int i = 0; i < 8; i++)
          for (int c = 0; c < 2; c++) PG(QP, QP_B + i * 2 + c, k, QP_NF) = s.Bm[i][c], PG(RC, RC_K + c * 8 + i, k, RC_NF) = s.K[c][i];
        for (int c = 0; c < 3; c++) PG(QP, QP_R + c, k, QP_NF) = s.R[c];
        for (int c = 0; c < 2; c++)
          for (int e = 0; e < 2; e++) PG(RC, RC_Kv + c * 2 + e, k, RC_NF) = s.Kv[c][e];
        for (int f = 0; f < PV_NF; f++) PL(PV, f, k, N) = s.PV[f];
        PL(Upl, 0, k, N) = s.U[0], PL(Upl, 1, k, N) = s.U[1];
      }
      if (k > 0) {
        for (int i = 0; i < 8; i++) {
          for (int l = 0; l <= i; l++) PG(RC, RC_P + sidx(i, l), k, RC_NF) = s.P[i][l];
          for (int c = 0; c < 2; c++) PG(RC, RC_Pxv + i * 2 + c, k, RC_NF) = s.Pxv[i][c];
        }
      }
    }
    THp[(size_t)14 * Bp + orig[b]] = rdu[2 * orig[b]], THp[(size_t)15 * Bp + orig[b]] = rdu[2 * orig[b] + 1];
  }
  W.QP = QP, W.RC = RC, W.U = Upl, W.orig = orig_x, W.TH = THp;
  const double *dth_arg = TH ? dth_x : nullptr, *pv_arg = TH ? PV : nullptr, *up_arg = TH ? uprev_x : nullptr;
  double* jv_arg = TH ? JV : nullptr;
  if (PI) wave64("k_jvp_sweep_pi", Bp / 8, [&] { k_jvp_sweep_pi(W, up_arg, pv_arg, ok_x, dp_x, dth_arg, jv_arg, tX, tU); });
  else wave64("k_jvp_sweep", Bp / 8, [&] { k_jvp_sweep(static_cast<const Work&>(W), r0, r1, up_arg, pv_arg, ok_x, dp_x, dth_arg, jv_arg, tX, tU); });
  // ---- the serial restatement, instance by instance
  typedef long double ld;
  int bad = 0;
  double case_worst = 0.0;
  for (int b = 0; b < B; b++) {
    const int o = orig[b];
    const std::vector<Stage>& s = S[b];
    ld d[PS_NT];
    for (int c = 0; c < PS_NT; c++) d[c] = TH ? dth[(size_t)o * PS_NT + c] : 0.0;
    const ld r2[2] = {2.0L * (PI ? rdu[2 * o] : r0), 2.0L * (PI ? rdu[2 * o + 1] : r1)};
    std::vector<ld> kff(2 * (size_t)N, 0.0L), bb(8 * (size_t)N, 0.0L);
    if (TH) {
      ld pp[8], pv[2] = {0, 0};
      for (int i = 0; i < 8; i++) {
        pp[i] = 0;
        for (int c = 0; c < PS_NDYN + 3; c++) pp[i] += d[c] * s[N - 1].PV[pv_qx(c) + i];
      }
      for (int k = N - 1; k >= 0; k--) {
        const Stage &t = s[k], &n = s[k + 1];
        ld bv[8], q[8], r[2] = {0, 0}, du[2], Pvv[2][2] = {{0, 0}, {0, 0}};
        for (int c = 0; c < 2; c++) du[c] = (ld)t.U[c] - (k > 0 ? (ld)s[k - 1].U[c] : (ld)uprev[2 * o + c]);
        if (k + 1 < N)
          for (int c = 0; c < 2; c++)
            for (int e = 0; e < 2; e++) Pvv[c][e] = (c == e ? r2[c] : 0.0L) - r2[c] * n.Kv[c][e];
        for (int i = 0; i < 8; i++) {
          bv[i] = q[i] = 0;
          for (int c = 0; c < PS_NDYN; c++) bv[i] += d[c] * t.PV[pv_base(c) + PV_b + i], q[i] += d[c] * t.PV[pv_base(c) + PV_q + i];
          for (int c = 0; k > 0 && c < PS_NDYN + 3; c++) q[i] += d[c] * s[k - 1].PV[pv_qx(c) + i];
        }
        for (int e = 0; e < 2; e++)
          for (int c = 0; c < PS_NDYN; c++) r[e] += d[c] * t.PV[pv_base(c) + PV_r + e];
        ld H[2][2];
        for (int c = 0; c < 2; c++)
          for (int e = 0; e < 2; e++) {
            ld v = t.R[sidx(c, e)] + Pvv[c][e] + (c == e ? r2[c] : 0.0L);
            for (int i = 0; i < 8; i++) {
              ld PBie = 0;
              for (int l = 0; l < 8; l++) PBie += (ld)n.P[i][l] * t.Bm[l][e];
              v += t.Bm[i][c] * PBie + (ld)t.Bm[i][c] * n.Pxv[i][e] + (ld)n.Pxv[i][c] * t.Bm[i][e];
            }
            H[c][e] = v;
          }
        const ld det = H[0][0] * H[1][1] - H[0][1] * H[1][0];
        if (!(H[0][0] > 0 && det > 1e-3L * H[0][0] * H[1][1])) return printf("FAIL: the seeded Huu is not well conditioned\n"), 1;
        ld Pb[8], gu[2], gx[8];
        for (int i = 0; i < 8; i++) {
          Pb[i] = pp[i];
          for (int l = 0; l < 8; l++) Pb[i] += (ld)n.P[i][l] * bv[l];
        }
        for (int e = 0; e < 2; e++) {
          gu[e] = r[e] + pv[e] + d[14 + e] * 2.0L * du[e];
          for (int i = 0; i < 8; i++) gu[e] += t.Bm[i][e] * Pb[i] + n.Pxv[i][e] * bv[i];
        }
        for (int i = 0; i < 8; i++) {
          gx[i] = q[i];
          for (int l = 0; l < 8; l++) gx[i] += t.A[l][i] * Pb[l];
        }
        const ld kf[2] = {-(H[1][1] * gu[0] - H[0][1] * gu[1]) / det, -(-H[1][0] * gu[0] + H[0][0] * gu[1]) / det};
        for (int i = 0; i < 8; i++) pp[i] = gx[i] + t.K[0][i] * gu[0] + t.K[1][i] * gu[1];
        for (int e = 0; e < 2; e++) pv[e] = -d[14 + e] * 2.0L * du[e] - r2[e] * kf[e], kff[2 * k + e] = kf[e];
        for (int i = 0; i < 8; i++) bb[8 * k + i] = bv[i];
      }
    }
    std::vector<ld> rX(8 * (size_t)(N + 1)), rU(2 * (size_t)N);
    ld tv[2] = {dp[(size_t)o * JVP_NP + 8], dp[(size_t)o * JVP_NP + 9]};
    for (int i = 0; i < 8; i++) rX[i] = dp[(size_t)o * JVP_NP + i];
    for (int k = 0; k < N; k++) {
      const Stage& t = s[k];
      ld u[2];
      for (int e = 0; e < 2; e++) {
        u[e] = kff[2 * k + e] + t.Kv[e][0] * tv[0] + t.Kv[e][1] * tv[1];
        for (int i = 0; i < 8; i++) u[e] += t.K[e][i] * rX[8 * k + i];
      }
      for (int i = 0; i < 8; i++) {
        ld v = bb[8 * k + i] + t.Bm[i][0] * u[0] + t.Bm[i][1] * u[1];
        for (int l = 0; l < 8; l++) v += t.A[i][l] * rX[8 * k + l];
        rX[8 * (k + 1) + i] = v;
      }
      rU[2 * k] = tv[0] = u[0], rU[2 * k + 1] = tv[1] = u[1];
    }
    // ---- compare (caller's order), exact zeros where ok = 0, block 0 bit for bit
    const double *gX = tX + (size_t)o * (N + 1) * 8, *gU = tU + (size_t)o * N * 2;
    ld scale = 1.0L, err = 0.0L;
    for (ld v : rX) scale = fmaxl(scale, fabsl(v));
    for (ld v : rU) scale = fmaxl(scale, fabsl(v));
    for (size_t e = 0; e < rX.size(); e++) {
      if (!ok[o]) bad += !(gX[e] == 0.0);
      else if (!std::isfinite(gX[e])) bad++;
      else err = fmaxl(err, fabsl(gX[e] - rX[e]));
    }
    for (size_t e = 0; e < rU.size(); e++) {
      if (!ok[o]) bad += !(gU[e] == 0.0);
      else if (!std::isfinite(gU[e])) bad++;
      else err = fmaxl(err, fabsl(gU[e] - rU[e]));
    }
    for (int i = 0; ok[o] && i < 8; i++) bad += !(gX[i] == dp[(size_t)o * JVP_NP + i]);
    case_worst = fmax(case_worst, (double)(err / scale));
  }
  printf("case B=%d N=%d pi=%d dtheta=%d: max_rel %.3e bad %d\n", B, N, (int)PI, (int)TH, case_worst, bad);
  worst = fmax(worst, case_worst);
  free(QP), free(RC), free(PV), free(Upl), free(THp), free(JV), free(tX), free(tU), free(uprev_x), free(orig_x), free(ok_x), free(dp_x), free(dth_x);
  return bad != 0 || !(case_worst <= REL_BOUND);
}

int main() {
  std::mt19937_64 rng(20240613);
  double worst = 0.0;
  int failed = 0;
  for (int B : {13, 61})
    for (int N : {2, 10})
      for (int PI = 0; PI < 2; PI++)
        for (int TH = 0; TH < 2; TH++) failed += run_case(B, N, PI != 0, TH != 0, rng, worst);
  printf("max_rel %.3e bound %.3e failed %d\n", worst, REL_BOUND, failed);
  return failed ? 1 : 0;
}
