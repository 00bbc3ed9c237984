// pick_harness.cpp — TEST INFRASTRUCTURE: k_pick (csrc/linesearch.h) compiled as host C++ and run on the lock-step 64-lane
// wavefront of hip_shim.h under AddressSanitizer + UndefinedBehaviorSanitizer.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// No solve: the per-instance state, the filter, the step partials and the filter measures of candidates 0 and 1 are read from a
// file (tests/test_host_harness_pick.py writes it) into buffers of exactly the size the kernel may touch, NaN bit patterns
// wherever the kernel has no business reading; one launch of k_pick, phase 0; then what d_pick may have written is printed per
// instance, the whole filter plane included, for the test to compare with its own restatement of the filter rule.
//   usage: pick_harness <file>
//   file:  "B N", then per instance: nfilt theta0 theta_max theta_min mu c00 rho, filter[2 FILTER_MAX], SP[3][N], LS[6][N]
//   out:   per instance "inst b  nfilt lsmore step iters ntiny nlsfail skip_eval  alpha adua force_reg theta0 theta_max theta_min
//          filter[2 FILTER_MAX]", then "list count b..."
// Nothing in the package uses this file.
#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace ltompc;

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

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: pick_harness <file>\n"), 2;
  FILE* f = fopen(argv[1], "r");
  int B, N;
  if (!f || fscanf(f, "%d %d", &B, &N) != 2) return fprintf(stderr, "pick_harness: cannot read %s\n", argv[1]), 2;
  const int Bp = (B + 63) / 64 * 64;
  static Consts K;  // (zero: no tables - the smoothing does not switch in these cases, cost_eval is not reached)
  ltompc_options& o = K.o;
  o.n_linesearch = 8, o.stall_iter = 15, o.max_ls_fail = 8, o.resto_rho = 1000.0, o.mu_init = 0.1, o.smooth_eps_min = 1e-4, o.smooth_scale = 1.0;
  o.resto_shift_retry = 1;
  static Work W;
  W.N = N, W.B = B, W.Bp = Bp;
  W.st = poisoned((size_t)ST_NF * Bp), W.filt = poisoned((size_t)2 * FILTER_MAX * Bp), W.x0 = poisoned((size_t)8 * Bp);
  W.SP = poisoned((size_t)SP_NF * N * Bp), W.LS = poisoned((size_t)3 * (o.n_linesearch + 1) * N * Bp);
  W.si = (int*)malloc(sizeof(int) * SI_NF * Bp);
  memset(W.si, 0, sizeof(int) * SI_NF * Bp);
  W.ls_list = (int*)malloc(sizeof(int) * Bp), W.ls_count = (int*)calloc(4, sizeof(int));
  memset(W.ls_list, 0xFF, sizeof(int) * Bp);
  int *act = (int*)malloc(sizeof(int) * Bp), *nact = (int*)malloc(sizeof(int));
  for (int b = 0; b < Bp; b++) act[b] = b;
  nact[0] = B;
  double* st = W.st;
  int* si = W.si;
  const auto rd = [&]() { double v; if (fscanf(f, "%lf", &v) != 1) fprintf(stderr, "pick_harness: short file\n"), exit(2); return v; };
  for (int b = 0; b < B; b++) {
    STI(SI_NFILT) = (int)rd();
    STD(ST_THETA0) = rd(), STD(ST_THMAX) = rd(), STD(ST_THMIN) = rd(), STD(ST_MU) = rd(), STD(ST_C00) = rd(), STD(ST_RHO) = rd();
    for (int q = 0; q < 2 * FILTER_MAX; q++) {
      const double v = rd();
      if (q < 2 * STI(SI_NFILT)) W.filt[(size_t)q * Bp + b] = v;  // (the pairs beyond nfilt stay NaN: they must not matter)
    }
    for (int q = 0; q < 3; q++)
      for (int k = 0; k < N; k++) PL(W.SP, q, k, N) = rd();
    for (int q = 0; q < 6; q++)
      for (int k = 0; k < N; k++) PL(W.LS, q, k, N) = rd();
    STD(ST_EPS) = STD(ST_EPS_NEXT) = 1e-4, STD(ST_FORCE_REG) = 0.5, STD(ST_ALPHA) = -7.0, STD(ST_ADUA) = -7.0;
    STI(SI_STEP) = 1, STI(SI_NTINY) = 3, STI(SI_ITERS) = 7, STI(SI_SKIP_EVAL) = -7, STI(SI_LSMORE) = -7;
    for (int q = 0; q < 8; q++) W.x0[(size_t)q * Bp + b] = 0.0;
  }
  fclose(f);
  Launch la{};
  la.act = act, la.nact = nact, la.n_pad = Bp, la.force_eval = 0;
  wave64("k_pick", (B * 8 + 63) / 64, [&] { k_pick(&K, &W, la, 0); });
  for (int b = 0; b < B; b++) {
    printf("inst %d  %d %d %d %d %d %d %d  %.17g %.17g %.17g %.17g %.17g %.17g ", b, STI(SI_NFILT), STI(SI_LSMORE), STI(SI_STEP), STI(SI_ITERS),
           STI(SI_NTINY), STI(SI_NLSFAIL), STI(SI_SKIP_EVAL), STD(ST_ALPHA), STD(ST_ADUA), STD(ST_FORCE_REG), STD(ST_THETA0), STD(ST_THMAX),
           STD(ST_THMIN));
    for (int q = 0; q < 2 * FILTER_MAX; q++) printf(" %.17g", W.filt[(size_t)q * Bp + b]);
    printf("\n");
  }
  printf("list %d", W.ls_count[0]);
  for (int j = 0; j < W.ls_count[0]; j++) printf(" %d", W.ls_list[j]);
  printf("\n");
  return 0;
}
