// lut_harness.cpp — TEST INFRASTRUCTURE: the batched table look-up of csrc/model.h (slot_luts_fetch / _pin / _finish) against
// lut_eval, compiled as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// The six table rows are allocated one by one at their exact size, so a knot fetched past either end of a row aborts the run
// (the batched form loads the knots of v_ref / n_left / n_right whether or not the caller uses them).  k_test_lut, the kernel
// behind ltompc_test_lut, runs lane after lane for every smoothing length of the file, its outputs in NaN-poisoned buffers of
// their exact size, and the two forms are compared bit for bit here.
//   usage: lut_harness <file>
//   file:  "n_table periodic n_eps n_points", the eps values, the six rows (s_kappa kappa s_arc n_left n_right v_ref), the points
//   out:   per eps "eps <eps> points <n> mismatches <count>", then "direct <n x 15 numbers of the first eps, %.17g>"
// Nothing in the package uses this file.
#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ltompc;

static double* poisoned(size_t n) {
  double* p = (double*)malloc(n * sizeof(double));
  memset(p, 0xFF, n * sizeof(double));
  return p;
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: lut_harness <file>\n"), 2;
  FILE* f = fopen(argv[1], "r");
  int nt, periodic, n_eps, n;
  if (!f || fscanf(f, "%d %d %d %d", &nt, &periodic, &n_eps, &n) != 4 || nt < 2 || n < 1) return fprintf(stderr, "lut_harness: cannot read %s\n", argv[1]), 2;
  const auto rd = [&]() { double v; if (fscanf(f, "%lf", &v) != 1) fprintf(stderr, "lut_harness: short file\n"), exit(2); return v; };
  std::vector<double> eps(n_eps);
  for (double& e : eps) e = rd();
  double* row[6];
  for (int r = 0; r < 6; r++) {
    row[r] = (double*)malloc(sizeof(double) * nt);
    for (int i = 0; i < nt; i++) row[r][i] = rd();
  }
  double* s = (double*)malloc(sizeof(double) * n);
  for (int t = 0; t < n; t++) s[t] = rd();
  fclose(f);
  static Consts K;
  Tables& T = K.T;
  T.n = nt, T.s_kappa = row[0], T.kappa = row[1], T.s_arc = row[2], T.n_left = row[3], T.n_right = row[4], T.v_ref = row[5];
  T.g0_kappa = row[0][0], T.inv_kappa = (double)(nt - 1) / (row[0][nt - 1] - row[0][0]);
  T.g0_arc = row[2][0], T.inv_arc = (double)(nt - 1) / (row[2][nt - 1] - row[2][0]);
  T.period = periodic ? row[0][nt - 1] - row[0][0] : 0.0;
  int bad = 0;
  for (int e = 0; e < n_eps; e++) {
    double *direct = poisoned((size_t)15 * n), *batched = poisoned((size_t)15 * n);
    blockDim.x = 64, gridDim.x = (n + 63) / 64;
    for (unsigned blk = 0; blk < gridDim.x; blk++)
      for (unsigned l = 0; l < 64; l++) {
        blockIdx.x = blk, threadIdx.x = l;
        k_test_lut(K, n, eps[e], s, direct, batched);
      }
    int mism = 0;
    for (size_t q = 0; q < (size_t)15 * n; q++)
      if (memcmp(&direct[q], &batched[q], sizeof(double))) {
        if (mism++ < 5) fprintf(stderr, "eps %.17g point %zu (s = %.17g / %.17g) number %zu: %.17g != %.17g\n", eps[e], q / 15, s[q / 15], s[n - 1 - q / 15], q % 15, direct[q], batched[q]);
      }
    printf("eps %.17g points %d mismatches %d\n", eps[e], n, mism);
    bad += mism;
    if (e == 0) {
      printf("direct");
      for (size_t q = 0; q < (size_t)15 * n; q++) printf(" %.17g", direct[q]);
      printf("\n");
    }
    free(direct), free(batched);
  }
  for (int r = 0; r < 6; r++) free(row[r]);
  free(s);
  return bad ? 1 : 0;
}
