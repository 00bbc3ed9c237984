// record_harness.cpp — TEST INFRASTRUCTURE: k_rec_save (csrc/record.h) compiled as host C++ and run under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_host_harness_records.py builds and runs it), then the re-linearisation, the head-less
// sweep and the forward pass of sensitivity.h on a Work built from the record and on the handle's own Work.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// No solve and no input file: a seeded iterate (states along a synthetic track, positive slacks and multipliers) in buffers of
// exactly the size the library allocates, NaN bit patterns in the pad lanes, the instances in permuted slots (a packed handle: orig
// and its inverse).  Every array of the record is an allocation of its own at its exact size, NaN-filled.  Checked, bit for bit:
//   - k_rec_save with the inverse map against a plain loop over every carried word, pad lanes included (they are copied slot for
//     slot); with a null map (an unpacked handle) against memcpy;
//   - k_sens_eval + k_sens_riccati8 + k_sens_forward (and the _pi forms) on the record's Work (identity orig) and on the packed
//     Work: the stage blocks and Riccati blocks of every instance, inertia, and du0 / ok / margin / dX / dU in the caller's order.
// Prints one line per check; exit status 1 when one fails.  Nothing in the package uses this file.
#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"
#include "eval8.h"
#include "sensitivity.h"
#include "record.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace ltompc;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { return rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17; }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() >> 11) / 9007199254740992.0; }

template <class T>
static T* poisoned(size_t n) {
  T* p = (T*)malloc((n ? n : 1) * sizeof(T));
  memset(p, 0xFF, (n ? n : 1) * sizeof(T));
  return p;
}
template <typename F>
static void grid_bs(size_t threads, unsigned bs, F&& body) {  // a thread-per-element kernel, lane after lane
  blockDim.x = bs, gridDim.x = (unsigned)((threads + bs - 1) / bs);
  for (unsigned blk = 0; blk < gridDim.x; blk++)
    for (unsigned t = 0; t < bs; t++) blockIdx.x = blk, threadIdx.x = t, body();
  blockDim.x = 64;
}
template <typename F>
static void wave64(const char* name, int blocks, F&& body) {  // a wave kernel on the lock-step wavefront, block after block
  blockDim.x = 64, gridDim.x = blocks;
  for (int blk = 0; blk < blocks; blk++) {
    blockIdx.x = blk;
    LtWave::self().run(name, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, &body);
  }
}

static Consts K;
static int N, B, Bp;

// The planes of a handle or of a record: name, pointer slot in Work, rows, 4-byte words
struct Plane {
  const char* name;
  void* p;
  int rows;
  bool w32;
};
struct Handle {
  WorkPI W{};
  int *orig = nullptr, *inv = nullptr;
  double *TH = nullptr, *pup = nullptr;
  std::vector<Plane> planes() const {
    const int ni = K.bd.ni;
    return {{"NU", W.NU, ni * N, false},      {"T", W.T, (ni + NNL) * N, false}, {"X", W.X, 8 * (N + 1), false}, {"C", W.C, 8 * N, false},
            {"L1", W.L1, 8 * N, false},       {"L2", W.L2, 8 * N, false},        {"U", W.U, 2 * N, false},       {"st", W.st, ST_NF, false},
            {"x0", W.x0, 8, false},           {"uprev", W.uprev, 2, false},      {"si", W.si, SI_NF, true}};
  }
};
static void alloc_planes(Handle& H) {
  Work& W = H.W;
  W.N = N, W.B = B, W.Bp = Bp;
  const size_t n = N, bp = Bp, ni = K.bd.ni;
  W.X = poisoned<double>(8 * (n + 1) * bp), W.C = poisoned<double>(8 * n * bp), W.U = poisoned<double>(2 * n * bp);
  W.L1 = poisoned<double>(8 * n * bp), W.L2 = poisoned<double>(8 * n * bp), W.T = poisoned<double>((ni + NNL) * n * bp);
  W.NU = poisoned<double>(ni * n * bp), W.st = poisoned<double>((size_t)ST_NF * bp), W.x0 = poisoned<double>(8 * bp);
  W.uprev = poisoned<double>(2 * bp), W.si = poisoned<int>((size_t)SI_NF * bp);
  H.orig = poisoned<int>(bp), H.inv = poisoned<int>(bp), H.TH = poisoned<double>((size_t)LTOMPC_NTHETA * bp), H.pup = poisoned<double>(2 * bp);
  W.orig = H.orig, H.W.TH = H.TH;
}
static void seed(Handle& H) {  // a packed handle after a solve: slot b holds instance orig[b]; pad lanes stay NaN
  Work& W = H.W;
  const int ni = K.bd.ni;
  for (int b = 0; b < B; b++) H.orig[b] = b;
  for (int b = B - 1; b > 0; b--) std::swap(H.orig[b], H.orig[rnd() % (b + 1)]);
  for (int b = 0; b < B; b++) H.inv[H.orig[b]] = b;
  const ltompc_params& p = K.p;
  const double t[LTOMPC_NTHETA] = {p.mass, p.inertia_z, p.B_f, p.C_f, p.D_f, p.B_r, p.C_r, p.D_r, p.C_m, p.Cr_0, p.Cr_2, p.q_n, p.q_mu, p.q_B, p.r_du[0], p.r_du[1]};
  for (int j = 0; j < LTOMPC_NTHETA; j++)
    for (int b = 0; b < Bp; b++) H.TH[(size_t)j * Bp + b] = t[j] * (b < B ? uni(0.95, 1.05) : 1.0);
  for (int b = 0; b < 2 * B; b++) H.pup[b] = uni(-0.3, 0.3);
  for (int b = 0; b < B; b++) {
    double x[8] = {uni(5, 100), uni(-0.5, 0.5), uni(-0.1, 0.1), uni(3, 12), uni(-0.2, 0.2), uni(-0.2, 0.2), uni(-0.2, 0.2), uni(-0.5, 0.5)};
    for (int i = 0; i < 8; i++) W.x0[(size_t)i * Bp + b] = x[i];
    for (int k = 0; k <= N; k++)
      for (int i = 0; i < 8; i++) PL(W.X, i, k, N + 1) = x[i] + (i == 0 ? 0.8 * k : 0.0) + uni(-0.01, 0.01);
    for (int k = 0; k < N; k++) {
      for (int i = 0; i < 8; i++) PL(W.C, i, k, N) = x[i] + (i == 0 ? 0.8 * k + 0.3 : 0.0), PL(W.L1, i, k, N) = uni(-1, 1), PL(W.L2, i, k, N) = uni(-1, 1);
      PL(W.U, 0, k, N) = uni(-0.3, 0.3), PL(W.U, 1, k, N) = uni(-0.5, 0.5);
      for (int m = 0; m < ni + NNL; m++) PL(W.T, m, k, N) = uni(0.05, 1.0);
      for (int m = 0; m < ni; m++) PL(W.NU, m, k, N) = uni(1e-3, 0.1);
    }
    W.uprev[b] = uni(-0.3, 0.3), W.uprev[(size_t)Bp + b] = uni(-0.5, 0.5);
    for (int f = 0; f < ST_NF; f++) W.st[(size_t)f * Bp + b] = 0.0;
    W.st[(size_t)ST_MU * Bp + b] = 1e-3, W.st[(size_t)ST_EPS * Bp + b] = 1e-4, W.st[(size_t)ST_TAU * Bp + b] = 0.99;
    for (int f = 0; f < SI_NF; f++) W.si[(size_t)f * Bp + b] = (int)(rnd() % 7);  // (the record must not carry the rows it does not list)
    const int stat[4] = {0, 1, 2, 5};
    int* si = W.si;
    STI(SI_STATUS) = stat[rnd() % 4], STI(SI_NODE0) = STI(SI_STATUS) == 5 ? (int)(rnd() % 3) : 0, STI(SI_REINIT) = rnd() % 9 == 0;
  }
}

// rec_fill's descriptor table (deriv_passes.h)
static RecPlanes descriptors(const Handle& H, const Handle& R, const bool pi) {
  RecPlanes P{};
  const auto add = [&](const void* src, void* dst, const int rows, const int flags) { P.p[P.n++] = RecPlane{src, dst, rows, flags}, P.rows += rows; };
  const std::vector<Plane> hs = H.planes(), rs = R.planes();
  for (size_t i = 0; i + 1 < hs.size(); i++) add(hs[i].p, rs[i].p, hs[i].rows, 0);
  for (const int f : {(int)SI_STATUS, (int)SI_NODE0, (int)SI_REINIT}) add(H.W.si + (size_t)f * Bp, R.W.si + (size_t)f * Bp, 1, REC_W32);
  add(H.pup, R.pup, 2, REC_DIRECT);
  if (pi) add(H.TH, R.TH, LTOMPC_NTHETA, REC_DIRECT);
  return P;
}
static void launch_save(const RecPlanes& P, const int* inv) {  // rec_fill's launch: grid (Bp / 256, rows / REC_ROWS), lane after lane
  blockDim.x = 256, gridDim.x = (Bp + 255) / 256, gridDim.y = (P.rows + REC_ROWS - 1) / REC_ROWS;
  for (unsigned y = 0; y < gridDim.y; y++)
    for (unsigned x = 0; x < gridDim.x; x++)
      for (unsigned t = 0; t < 256; t++) blockIdx.x = x, blockIdx.y = y, threadIdx.x = t, k_rec_save(P, inv, B, Bp);
  blockIdx.y = 0, gridDim.y = 1, blockDim.x = 64;
}
static bool carried_si(const int f) { return f == SI_STATUS || f == SI_NODE0 || f == SI_REINIT; }

static int failures = 0;
static void verdict(const char* what, const bool ok) {
  printf("%s %s\n", what, ok ? "ok" : "FAILED");
  failures += ok ? 0 : 1;
}

// k_rec_save against the plain statement of the record: word (row, b) of every carried plane is the handle's word at the slot of
// instance b (b < B) or at slot b itself (pad lanes); everything else in the record keeps its NaN pattern.
static void check_save(const Handle& H, const bool packed, const bool pi) {
  Handle R, E;
  alloc_planes(R), alloc_planes(E);
  const RecPlanes P = descriptors(H, R, pi);
  launch_save(P, packed ? H.inv : nullptr);
  const std::vector<Plane> hs = H.planes(), rs = R.planes(), es = E.planes();
  bool same = true;
  for (size_t i = 0; i < hs.size(); i++) {
    for (int r = 0; r < hs[i].rows; r++)
      for (int b = 0; b < Bp; b++) {
        const int slot = (packed && b < B) ? H.inv[b] : b;
        const size_t to = (size_t)r * Bp + b, from = (size_t)r * Bp + slot;
        if (hs[i].w32) {
          if (carried_si(r)) ((int*)es[i].p)[to] = ((const int*)hs[i].p)[from];
        } else ((double*)es[i].p)[to] = ((const double*)hs[i].p)[from];
      }
    same = same && !memcmp(rs[i].p, es[i].p, (size_t)hs[i].rows * Bp * (hs[i].w32 ? sizeof(int) : sizeof(double)));
  }
  memcpy(E.pup, H.pup, sizeof(double) * 2 * Bp);
  if (pi) memcpy(E.TH, H.TH, sizeof(double) * LTOMPC_NTHETA * Bp);
  same = same && !memcmp(R.pup, E.pup, sizeof(double) * 2 * Bp) && !memcmp(R.TH, E.TH, sizeof(double) * LTOMPC_NTHETA * Bp);
  char what[64];
  snprintf(what, sizeof what, "save packed=%d pi=%d", (int)packed, (int)pi);
  verdict(what, same);
}

// The three kernels of sens_factorise / sens_compute on Work `Wsrc` (slots by `orig`): stage and Riccati blocks per instance in
// the caller's order, inertia, and the forward pass' outputs.
struct Pass {
  std::vector<double> QP, RC, du0, margin, dX, dU;
  std::vector<int> inertia, ok;
};
static Pass run_pass(const WorkPI& Wsrc, const int* orig, const bool pi) {
  const size_t n = N, bp = Bp;
  WorkPI Ws = Wsrc;  // (sens_buffers: QP, RC, RS, LS of the pass, si zeros)
  Ws.QP = poisoned<double>((size_t)QP_NF * (n + 1) * bp), Ws.RC = poisoned<double>((size_t)RC_NF * (n + 1) * bp);
  Ws.RS = poisoned<double>((size_t)RS_NF * n * bp), Ws.LS = poisoned<double>((size_t)3 * n * bp);
  Ws.si = (int*)calloc((size_t)SI_NF * bp, sizeof(int));
  int *inertia = (int*)calloc(bp, sizeof(int)), *ok = (int*)calloc(bp, sizeof(int));
  Pass R;
  R.du0.assign((size_t)2 * SENS_NP * B, -7.0), R.margin.assign(B, -7.0), R.dX.assign((n + 1) * 8 * SENS_NP * B, -7.0), R.dU.assign(n * 2 * SENS_NP * B, -7.0);
  const Work& Wsu = Ws;
  const int ni = K.bd.ni;
  if (pi) grid_bs(n * bp, 64, [&] { k_sens_eval_pi<BoundsRef>(&K, &Ws); });
  else grid_bs(n * bp, 64, [&] { k_sens_eval<BoundsRef, false>(&K, &Wsu); });
  if (pi) wave64("k_sens_riccati8_pi", Bp / 8, [&] { k_sens_riccati8_pi(K, Ws, Wsrc.si, inertia); });
  else wave64("k_sens_riccati8", Bp / 8, [&] { k_sens_riccati8(K, Wsu, Wsrc.si, inertia); });
  wave64("k_sens_forward", Bp / 8, [&] { k_sens_forward(Wsu, inertia, ni, R.du0.data(), ok, R.margin.data(), nullptr, nullptr, nullptr); });
  wave64("k_sens_forward", Bp / 8, [&] { k_sens_forward(Wsu, inertia, ni, nullptr, nullptr, nullptr, R.dX.data(), R.dU.data(), ok); });
  R.inertia.assign(B, 0), R.ok.assign(ok, ok + B);
  R.QP.assign((size_t)QP_NF * (n + 1) * B, 0.0), R.RC.assign((size_t)RC_NF * (n + 1) * B, 0.0);
  const Work& W = Ws;
  for (int b = 0; b < B; b++) {
    const size_t o = orig[b];
    R.inertia[o] = inertia[b];
    for (int k = 0; k <= N; k++) {
      for (int f = 0; f < QP_NF; f++) R.QP[(o * (n + 1) + k) * QP_NF + f] = PG(W.QP, f, k, QP_NF);
      for (int f = 0; f < RC_NF; f++) R.RC[(o * (n + 1) + k) * RC_NF + f] = PG(W.RC, f, k, RC_NF);
    }
  }
  return R;
}
template <class T>
static bool eq(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * sizeof(T));
}

int main() {
  N = 6, B = 77, Bp = 128;
  ltompc_params& p = K.p;
  memset(&K, 0, sizeof K);
  p.mass = 1000.0, p.inertia_z = 1000.0, p.length_f = 1.5, p.length_r = 1.5, p.width = 2.3, p.B_f = 10.0, p.C_f = 1.3, p.D_f = 1.0, p.B_r = 12.0, p.C_r = 1.2, p.D_r = 1.0;
  p.C_m = 1000.0, p.Cr_0 = 0.01, p.Cr_2 = 0.0003, p.gravity = 9.81, p.q_n = 0.5, p.q_mu = 3.0, p.q_vy = 1.0, p.q_v = 1.0, p.vref_scale = 0.6, p.q_B = 1e-2;
  p.r_du[0] = p.r_du[1] = 1e-2;
  for (int i = 0; i < NX; i++) p.x_lb[i] = -LTOMPC_NO_BOUND, p.x_ub[i] = LTOMPC_NO_BOUND;
  const double pi = 3.14159265358979323846;  // (the reference's bound pattern: the kernels instantiated with BoundsRef)
  p.x_lb[0] = 0.0, p.x_lb[2] = -pi * 0.5, p.x_ub[2] = pi * 0.5, p.x_lb[3] = 0.0, p.x_lb[6] = -pi / 4, p.x_ub[6] = pi / 4, p.x_lb[7] = -1.0, p.x_ub[7] = 1.0;
  p.u_lb[0] = -2 * pi / 4, p.u_ub[0] = 2 * pi / 4, p.u_lb[1] = -1.0, p.u_ub[1] = 1.0;
  K.o.t_step = 0.1, K.o.smooth_eps_min = 1e-4;
  Bounds& bd = K.bd;
  for (int i = 0; i < NX; i++) {  // = build_bounds (ltompc.hip)
    if (p.x_lb[i] > -LTOMPC_NO_BOUND) bd.xb_idx[bd.n_xb] = i, bd.xb_sgn[bd.n_xb] = -1.0, bd.xb_val[bd.n_xb] = p.x_lb[i], bd.n_xb++;
    if (p.x_ub[i] < LTOMPC_NO_BOUND) bd.xb_idx[bd.n_xb] = i, bd.xb_sgn[bd.n_xb] = +1.0, bd.xb_val[bd.n_xb] = p.x_ub[i], bd.n_xb++;
  }
  for (int i = 0; i < NU; i++) {
    bd.ub_idx[bd.n_ub] = i, bd.ub_sgn[bd.n_ub] = -1.0, bd.ub_val[bd.n_ub] = p.u_lb[i], bd.n_ub++;
    bd.ub_idx[bd.n_ub] = i, bd.ub_sgn[bd.n_ub] = +1.0, bd.ub_val[bd.n_ub] = p.u_ub[i], bd.n_ub++;
  }
  bd.ni = bd.n_ub + 2 * bd.n_xb + NNL;
  const int nt = 33;  // a synthetic track: 160 m of gentle curvature, 6 m wide (exact size: a look-up past either end is an ASan error)
  double* tab = poisoned<double>(6 * nt);
  for (int i = 0; i < nt; i++) {
    tab[i] = tab[2 * nt + i] = 5.0 * i;
    tab[nt + i] = 0.01 * sin(0.1 * i), tab[3 * nt + i] = 3.0 + 0.1 * cos(0.2 * i), tab[4 * nt + i] = -3.0 + 0.1 * sin(0.3 * i), tab[5 * nt + i] = 12.0 + sin(0.15 * i);
  }
  Tables& T = K.T;
  T.n = nt, T.s_kappa = tab, T.kappa = tab + nt, T.s_arc = tab + 2 * nt, T.n_left = tab + 3 * nt, T.n_right = tab + 4 * nt, T.v_ref = tab + 5 * nt;
  T.g0_kappa = T.g0_arc = 0.0, T.inv_kappa = T.inv_arc = (nt - 1) / tab[nt - 1], T.period = 0.0;

  Handle H;
  alloc_planes(H), seed(H);
  for (int packed = 0; packed < 2; packed++)
    for (int pi_rows = 0; pi_rows < 2; pi_rows++) check_save(H, packed != 0, pi_rows != 0);

  // the passes on the record (identity orig, its own copy of the value rows) and on the packed handle
  for (int pi_rows = 0; pi_rows < 2; pi_rows++) {
    Handle R;
    alloc_planes(R);
    const RecPlanes P = descriptors(H, R, true);
    launch_save(P, H.inv);
    for (int b = 0; b < Bp; b++) R.orig[b] = b;
    const Pass live = run_pass(H.W, H.orig, pi_rows != 0);
    double* rows = poisoned<double>(4 * nt);  // kappa, n_left, n_right, v_ref: the record's copies
    memcpy(rows, tab + nt, sizeof(double) * nt), memcpy(rows + nt, tab + 3 * nt, sizeof(double) * 3 * nt);
    const Tables keep = K.T;
    K.T.kappa = rows, K.T.n_left = rows + nt, K.T.n_right = rows + 2 * nt, K.T.v_ref = rows + 3 * nt;
    memset(tab + nt, 0xFF, sizeof(double) * nt), memset(tab + 3 * nt, 0xFF, sizeof(double) * 3 * nt);  // (the handle's rows have changed since)
    const Pass rec = run_pass(R.W, R.orig, pi_rows != 0);
    memcpy(tab + nt, rows, sizeof(double) * nt), memcpy(tab + 3 * nt, rows + nt, sizeof(double) * 3 * nt);
    K.T = keep;
    int n_ok = 0;
    for (int v : live.ok) n_ok += v;
    printf("pass pi=%d: ok %d of %d\n", pi_rows, n_ok, B);
    verdict("  stage blocks", eq(live.QP, rec.QP));
    verdict("  riccati blocks", eq(live.RC, rec.RC));
    verdict("  inertia, ok", eq(live.inertia, rec.inertia) && eq(live.ok, rec.ok));
    verdict("  du0, margin", eq(live.du0, rec.du0) && eq(live.margin, rec.margin));
    verdict("  dX, dU", eq(live.dX, rec.dX) && eq(live.dU, rec.dU));
  }
  printf("done failures %d\n", failures);
  return failures ? 1 : 0;
}
