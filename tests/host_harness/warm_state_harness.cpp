// warm_state_harness.cpp — TEST INFRASTRUCTURE: the kernels of csrc/warm_state.h compiled as host C++ and run under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_host_harness_warm_state.py builds and runs it).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// No solve and no input file: seeded state in buffers of exactly the size the library allocates, NaN bit patterns in the pad
// lanes and wherever a kernel has no business reading, a permuted `orig` (a packed handle).  Checked here, bit for bit:
//   - k_load_x0_m + k_init_m(_pi) with per-instance flags against d_load_x0 + the uniform d_init_slot called per instance with that
//     instance's flag; k_roll_mark_m + k_roll_init_m(_pi) the same; k_ws_reset_mark + k_ws_reset_init and k_ws_guess against plain loops;
//   - k_ws_export against a plain loop over every carried word, k_ws_import of that blob into another handle (another permutation,
//     other indices) against the plain loop: every carried word arrives, nothing else changes, pad lanes untouched; a full batch
//     (part-filled tiles in both directions) and 13 scattered instances.
// The LDS-tiled copy kernels run on the lock-step workgroup of hip_shim.h (4 wavefronts); wave_order=asc|desc chooses the order of
// the wavefronts between two barriers, and the printed checksums of both runs must agree (a missing barrier shows as a difference).
//   usage: warm_state_harness [wave_order=asc|desc]
// Nothing in the package uses this file.
#include "hip_shim.h"

#include "layout.h"
#include "linearise.h"
#include "aux_kernels.h"
#include "rollout.h"
#include "warm_state.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace ltompc;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { return rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17; }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() >> 11) / 9007199254740992.0; }

template <typename F>
static void grid_bs(size_t threads, unsigned bs, F&& body) {
  blockDim.x = bs, gridDim.x = (unsigned)((threads + bs - 1) / bs);
  for (unsigned blk = 0; blk < gridDim.x; blk++)
    for (unsigned t = 0; t < bs; t++) blockIdx.x = blk, threadIdx.x = t, body();
}
template <typename F>
static void wg256(const char* name, int blocks, F&& body) {
  blockDim.x = 256, gridDim.x = blocks;
  for (int blk = 0; blk < blocks; blk++) {
    blockIdx.x = blk;
    LtWave::self().run(name, 4, LtWave::STACK_SMALL, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, &body);
  }
}

// One handle's device state: every array at the library's exact size.
struct Buf {
  void** at;
  size_t bytes;
};
struct State {
  WorkPI W{};
  std::vector<Buf> bufs;
  int *orig = nullptr, *inv = nullptr, *cold = nullptr;
  double* th = nullptr;
  State() = default;
  State(const State& A) : W(A.W), orig(A.orig), inv(A.inv), cold(A.cold), th(A.th) {  // a deep copy; bufs point into THIS object, in make_state's order
    void** slots[] = {(void**)&W.X, (void**)&W.C, (void**)&W.U, (void**)&W.L1, (void**)&W.L2, (void**)&W.T, (void**)&W.NU, (void**)&W.BK, (void**)&W.x0,
                      (void**)&W.uprev, (void**)&W.st, (void**)&W.si, (void**)&orig, (void**)&inv, (void**)&cold, (void**)&th};
    for (size_t i = 0; i < A.bufs.size(); i++) {
      void* q = malloc(A.bufs[i].bytes);
      memcpy(q, *A.bufs[i].at, A.bufs[i].bytes);
      *slots[i] = q;
      bufs.push_back(Buf{slots[i], A.bufs[i].bytes});
    }
    W.orig = orig, W.TH = th;
  }
  State& operator=(const State&) = delete;
  template <class T> T* mk(T** p, size_t n) {
    *p = (T*)malloc(n * sizeof(T));
    memset(*p, 0xFF, n * sizeof(T));
    bufs.push_back(Buf{(void**)p, n * sizeof(T)});
    return *p;
  }
};
static Consts K;
static int N, B, Bp;

static void make_state(State& S, const ltompc_params& p) {
  Work& W = S.W;
  W.N = N, W.B = B, W.Bp = Bp;
  const size_t n = N, bp = Bp, ni = K.bd.ni;
  S.mk(&W.X, 8 * (n + 1) * bp), S.mk(&W.C, 8 * n * bp), S.mk(&W.U, 2 * n * bp), S.mk(&W.L1, 8 * n * bp), S.mk(&W.L2, 8 * n * bp);
  S.mk(&W.T, (ni + NNL) * n * bp), S.mk(&W.NU, ni * n * bp), S.mk(&W.BK, 18 * n * bp);
  S.mk(&W.x0, 8 * bp), S.mk(&W.uprev, 2 * bp), S.mk(&W.st, (size_t)ST_NF * bp), S.mk(&W.si, (size_t)SI_NF * bp);
  S.mk(&S.orig, bp), S.mk(&S.inv, bp), S.mk(&S.cold, bp), S.mk(&S.th, (size_t)LTOMPC_NTHETA * bp);
  W.orig = S.orig, S.W.TH = S.th;
  for (int b = 0; b < B; b++) S.orig[b] = b;
  for (int b = B - 1; b > 0; b--) std::swap(S.orig[b], S.orig[rnd() % (b + 1)]);  // a packed handle: slot b holds instance orig[b]
  for (int b = 0; b < B; b++) S.inv[S.orig[b]] = b;
  const double t[LTOMPC_NTHETA] = {p.mass, p.inertia_z, p.B_f, p.C_f, p.D_f, p.B_r, p.C_r, p.D_r, p.C_m, p.Cr_0, p.Cr_2, p.q_n, p.q_mu, p.q_B, p.r_du[0], p.r_du[1]};
  for (int j = 0; j < LTOMPC_NTHETA; j++)
    for (int b = 0; b < Bp; b++) S.th[(size_t)j * Bp + b] = t[j] * (b < B ? uni(0.9, 1.1) : 1.0);
  for (int b = 0; b < B; b++) {  // a plausible previous solution: states near a drive along the track, small multipliers
    double x[8] = {uni(5, 100), uni(-0.5, 0.5), uni(-0.1, 0.1), uni(3, 12), uni(-0.2, 0.2), uni(-0.2, 0.2), uni(-0.2, 0.2), uni(-0.5, 0.5)};
    for (int k = 0; k <= N; k++)
      for (int i = 0; i < 8; i++) PL(W.X, i, k, N + 1) = x[i] + (i == 0 ? 0.8 * k : 0.0) + uni(-0.01, 0.01);
    for (int k = 0; k < N; k++) {
      for (int i = 0; i < 8; i++) PL(W.C, i, k, N) = x[i] + (i == 0 ? 0.8 * k + 0.3 : 0.0), PL(W.L1, i, k, N) = uni(-1, 1), PL(W.L2, i, k, N) = uni(-1, 1);
      PL(W.U, 0, k, N) = uni(-0.3, 0.3), PL(W.U, 1, k, N) = uni(-0.5, 0.5);
    }
    W.uprev[b] = uni(-0.3, 0.3), W.uprev[(size_t)Bp + b] = uni(-0.5, 0.5);
    for (int f = 0; f < SI_NF; f++) W.si[(size_t)f * Bp + b] = 0;
    const int stat[4] = {0, 1, 2, 5};
    int* si = W.si;
    STI(SI_STATUS) = stat[rnd() % 4], STI(SI_NODE0) = STI(SI_STATUS) == 5 ? (int)(rnd() % 3) : 0, STI(SI_NRESTO) = rnd() % 2, STI(SI_STARTEL) = rnd() % 2;
    STI(SI_STICKY) = rnd() % 3, STI(SI_ITERS) = 17, STI(SI_PHASE) = PH_READY;
    S.cold[b] = rnd() % 3 == 0;
  }
}
static uint64_t g_sum = 1469598103934665603ull;
static void same(const State& A, const State& E, const char* what) {
  for (size_t i = 0; i < A.bufs.size(); i++) {
    if (memcmp(*A.bufs[i].at, *E.bufs[i].at, A.bufs[i].bytes)) fprintf(stderr, "warm_state_harness: %s: array %zu differs from its expectation\n", what, i), exit(1);
    const unsigned char* q = (const unsigned char*)*A.bufs[i].at;
    for (size_t j = 0; j < A.bufs[i].bytes; j++) g_sum = (g_sum ^ q[j]) * 1099511628211ull;
  }
  printf("%s ok %016llx\n", what, (unsigned long long)g_sum);
}

// the carried words of the instance in slot `slot`, in blob order: the plain-loop statement of the layout
static void row_of(const State& S, const int slot, const int cold_all, double* row) {
  const Work& W = S.W;
  const int b = slot;
  const int* si = W.si;
  int c = 0;
  row[c++] = ws_header(N);
  row[c++] = STI(SI_STATUS), row[c++] = STI(SI_NODE0), row[c++] = STI(SI_NRESTO), row[c++] = STI(SI_STARTEL), row[c++] = STI(SI_STICKY);
  row[c++] = (cold_all || S.cold[S.orig[slot]]) ? 1.0 : 0.0;
  row[c++] = W.uprev[b], row[c++] = W.uprev[(size_t)Bp + b], row[c++] = 0.0;
  for (int k = 0; k <= N; k++) for (int i = 0; i < 8; i++) row[c++] = PL(W.X, i, k, N + 1);
  for (int k = 0; k < N; k++) for (int i = 0; i < 8; i++) row[c++] = PL(W.C, i, k, N);
  for (int k = 0; k < N; k++) for (int i = 0; i < 2; i++) row[c++] = PL(W.U, i, k, N);
  for (int k = 0; k < N; k++) for (int i = 0; i < 8; i++) row[c++] = PL(W.L1, i, k, N);
  for (int k = 0; k < N; k++) for (int i = 0; i < 8; i++) row[c++] = PL(W.L2, i, k, N);
  if (c != ws_size(N)) fprintf(stderr, "warm_state_harness: ws_size\n"), exit(1);
}
static void row_into(State& S, const int slot, const double* row) {
  Work& W = S.W;
  const int b = slot;
  int* si = W.si;
  int c = 1;
  STI(SI_STATUS) = (int)row[c++], STI(SI_NODE0) = (int)row[c++], STI(SI_NRESTO) = (int)row[c++], STI(SI_STARTEL) = (int)row[c++], STI(SI_STICKY) = (int)row[c++];
  S.cold[S.orig[slot]] = row[c++] != 0.0;
  W.uprev[b] = row[c++], W.uprev[(size_t)Bp + b] = row[c++], c++;
  for (int k = 0; k <= N; k++) for (int i = 0; i < 8; i++) PL(W.X, i, k, N + 1) = row[c++];
  for (int k = 0; k < N; k++) for (int i = 0; i < 8; i++) PL(W.C, i, k, N) = row[c++];
  for (int k = 0; k < N; k++) for (int i = 0; i < 2; i++) PL(W.U, i, k, N) = row[c++];
  for (int k = 0; k < N; k++) for (int i = 0; i < 8; i++) PL(W.L1, i, k, N) = row[c++];
  for (int k = 0; k < N; k++) for (int i = 0; i < 8; i++) PL(W.L2, i, k, N) = row[c++];
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    const std::string s(argv[a]);
    if (s == "wave_order=desc") LtWave::self().desc_waves = true;
    else if (s != "wave_order=asc") return fprintf(stderr, "usage: warm_state_harness [wave_order=asc|desc]\n"), 2;
  }
  N = 6, B = 77, Bp = 128;
  ltompc_params& p = K.p;
  memset(&K, 0, sizeof K);
  p.mass = 1000.0, p.inertia_z = 1000.0, p.length_f = 1.5, p.length_r = 1.5, p.width = 2.3, p.B_f = 10.0, p.C_f = 1.3, p.D_f = 1.0, p.B_r = 12.0, p.C_r = 1.2, p.D_r = 1.0;
  p.C_m = 1000.0, p.Cr_0 = 0.01, p.Cr_2 = 0.0003, p.gravity = 9.81, p.q_n = 0.5, p.q_mu = 3.0, p.q_vy = 1.0, p.q_v = 1.0, p.vref_scale = 0.6, p.q_B = 1e-2;
  p.r_du[0] = p.r_du[1] = 1e-2;
  for (int i = 0; i < NX; i++) p.x_lb[i] = -LTOMPC_NO_BOUND, p.x_ub[i] = LTOMPC_NO_BOUND;
  p.x_lb[0] = 0.0, p.x_lb[2] = -1.5, p.x_ub[2] = 1.5, p.x_lb[3] = 0.0, p.x_lb[6] = -0.78, p.x_ub[6] = 0.78, p.x_lb[7] = -1.0, p.x_ub[7] = 1.0;
  p.u_lb[0] = -1.57, p.u_ub[0] = 1.57, p.u_lb[1] = -1.0, p.u_ub[1] = 1.0;
  ltompc_options& o = K.o;
  o.t_step = 0.1, o.mu_init = 0.1, o.mu_init_warm = 1e-3, o.bound_push = 1e-2, o.smooth_eps_min = 1e-4, o.smooth_scale = 1.0, o.warm_reset_on_fail = 1;
  o.resto_rho = 1000.0, o.resto_rho_max = 1e6, o.resto_sticky = 2, o.infeasible_sticky = 1, o.node0_check = 1, o.warm_fallback_iter = 25, o.resto_shift_retry = 1;
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
  const int nt = 33;  // a synthetic track: 160 m of gentle curvature, 6 m wide
  static double tab[6 * 33];
  for (int i = 0; i < nt; i++) {
    tab[i] = tab[2 * nt + i] = 5.0 * i;
    tab[nt + i] = 0.01 * sin(0.1 * i), tab[3 * nt + i] = 3.0 + 0.1 * cos(0.2 * i), tab[4 * nt + i] = -3.0 + 0.1 * sin(0.3 * i), tab[5 * nt + i] = 12.0 + sin(0.15 * i);
  }
  Tables& T = K.T;
  T.n = nt, T.s_kappa = tab, T.kappa = tab + nt, T.s_arc = tab + 2 * nt, T.n_left = tab + 3 * nt, T.n_right = tab + 4 * nt, T.v_ref = tab + 5 * nt;
  T.g0_kappa = T.g0_arc = 0.0, T.inv_kappa = T.inv_arc = (nt - 1) / tab[nt - 1], T.period = 0.0;

  State A;
  make_state(A, p);
  std::vector<double> x0rm((size_t)B * 8);  // exact size, the caller's order
  for (auto& v : x0rm) v = uni(-0.2, 0.2);
  for (int r = 0; r < B; r++) x0rm[(size_t)r * 8] = uni(5, 100), x0rm[(size_t)r * 8 + 3] = uni(3, 12);
  const int sticky = o.resto_sticky;
  static int act[128], nact[1];
  for (int b = 0; b < Bp; b++) act[b] = b;
  nact[0] = B;
  Launch la{};
  la.act = act, la.nact = nact, la.n_pad = Bp;

  // ---- start of a solve with per-instance flags against the uniform device functions, instance by instance
  for (int pi = 0; pi < 2; pi++) {
    State G(A), E(A);
    grid_bs(B, 64, [&] { k_load_x0_m(G.W, x0rm.data(), sticky, G.cold); });
    if (pi) grid_bs((size_t)N * Bp, 64, [&] { k_init_m_pi(&K, &G.W, G.cold); });
    else grid_bs((size_t)N * Bp, 64, [&] { k_init_m(&K, &G.W, G.cold); });
    for (int b = 0; b < B; b++) {
      const int c = E.cold[E.orig[b]] ? 1 : 0;
      d_load_x0(E.W, x0rm.data(), b, (size_t)E.orig[b], sticky, c ? 0 : 1);
      for (int k = 0; k < N; k++) pi ? d_init_slot<true>(K, E.W, k, b, c) : d_init_slot<false>(K, E.W, k, b, c);
    }
    same(G, E, pi ? "init_m_pi" : "init_m");
  }
  for (int pi = 0; pi < 2; pi++) {  // the rollout's first pass (caller's order: orig = identity)
    State G(A);
    for (int b = 0; b < B; b++) G.orig[b] = G.inv[b] = b;
    State E(G);
    grid_bs(B, 64, [&] { k_roll_mark_m(G.W, x0rm.data(), sticky, G.cold); });
    if (pi) grid_bs((size_t)N * Bp, 64, [&] { k_roll_init_m_pi(&K, &G.W, la, G.cold); });
    else grid_bs((size_t)N * Bp, 64, [&] { k_roll_init_m(&K, &G.W, la, G.cold); });
    for (int b = 0; b < B; b++) {
      const int c = E.cold[b] ? 1 : 0;
      d_load_x0(E.W, x0rm.data(), b, (size_t)b, sticky, c ? 0 : 1);
      E.W.si[(size_t)SI_PHASE * Bp + b] = PH_INIT;
      for (int k = 0; k < N; k++) pi ? d_init_slot<true>(K, E.W, k, b, c) : d_init_slot<false>(K, E.W, k, b, c);
    }
    same(G, E, pi ? "roll_init_m_pi" : "roll_init_m");
  }
  std::vector<int> mask(B);
  for (auto& m : mask) m = rnd() % 4 == 0;
  mask[0] = mask[B - 1] = 1;
  {  // masked reset
    State G(A), E(A);
    grid_bs(B, 64, [&] { k_ws_reset_mark(G.W, mask.data(), x0rm.data(), G.cold); });
    grid_bs((size_t)N * Bp, 64, [&] { k_ws_reset_init(&K, &G.W, mask.data()); });
    for (int b = 0; b < B; b++) {
      const int r = E.orig[b];
      if (!mask[r]) continue;
      d_load_x0(E.W, x0rm.data(), b, (size_t)r, 0, 0);
      E.W.uprev[b] = E.W.uprev[(size_t)Bp + b] = 0.0, E.cold[r] = 1;
      for (int k = 0; k < N; k++) d_init_slot<false>(K, E.W, k, b, 1);
    }
    same(G, E, "reset");
  }
  {  // trajectory guess
    std::vector<double> Xg((size_t)B * (N + 1) * 8), Cg((size_t)B * N * 8), Ug((size_t)B * N * 2), ug((size_t)B * 2);
    for (auto* v : {&Xg, &Cg, &Ug, &ug})
      for (auto& q : *v) q = uni(-1, 1);
    for (int with_u = 0; with_u < 2; with_u++) {
      State G(A), E(A);
      grid_bs((size_t)(N + 1) * Bp, 256, [&] { k_ws_guess(G.W, mask.data(), Xg.data(), Cg.data(), Ug.data(), with_u ? ug.data() : nullptr, G.cold); });
      for (int b = 0; b < B; b++) {
        const size_t r = E.orig[b];
        if (!mask[r]) continue;
        Work& W = E.W;
        int* si = W.si;
        for (int i = 0; i < 8; i++) {
          for (int k = 0; k <= N; k++) PL(W.X, i, k, N + 1) = Xg[(r * (N + 1) + k) * 8 + i];
          for (int k = 0; k < N; k++) PL(W.C, i, k, N) = Cg[(r * N + k) * 8 + i], PL(W.L1, i, k, N) = 0.0, PL(W.L2, i, k, N) = 0.0;
        }
        for (int k = 0; k < N; k++) PL(W.U, 0, k, N) = Ug[(r * N + k) * 2], PL(W.U, 1, k, N) = Ug[(r * N + k) * 2 + 1];
        STI(SI_STATUS) = LTOMPC_STATUS_MAX_ITER, STI(SI_NODE0) = STI(SI_NRESTO) = STI(SI_STARTEL) = STI(SI_STICKY) = 0;
        W.uprev[b] = with_u ? ug[r * 2] : 0.0, W.uprev[(size_t)Bp + b] = with_u ? ug[r * 2 + 1] : 0.0, E.cold[r] = 0;
      }
      same(G, E, with_u ? "guess_uprev" : "guess");
    }
  }

  // ---- export, then import into another handle: the identity on every carried word, nothing else touched
  const int S = ws_size(N);
  const int ncb = (S + WS_TILE - 1) / WS_TILE;
  State C2;
  make_state(C2, p);  // (other data, another permutation)
  for (int round = 0; round < 3; round++) {
    const int n = round == 1 ? 13 : B;
    const int cold_all = round == 2;
    std::vector<int> idx(n), to(n);
    {
      std::vector<int> perm(B), perm2(B);
      for (int b = 0; b < B; b++) perm[b] = perm2[b] = b;
      for (int b = B - 1; b > 0; b--) std::swap(perm[b], perm[rnd() % (b + 1)]), std::swap(perm2[b], perm2[rnd() % (b + 1)]);
      for (int j = 0; j < n; j++) idx[j] = perm[j], to[j] = perm2[j];
    }
    const bool identity = round == 2;  // idx = nullptr: row j = instance j
    double* blob = (double*)malloc(sizeof(double) * n * S);  // exact size
    memset(blob, 0xFF, sizeof(double) * n * S);
    State G(A);
    const int blocks = (n + WS_TILE - 1) / WS_TILE * ncb;
    wg256("k_ws_export", blocks, [&] { k_ws_export(G.W, identity ? nullptr : idx.data(), G.inv, n, blob, G.cold, cold_all); });
    same(G, A, "export leaves the handle");
    std::vector<double> row(S);
    for (int j = 0; j < n; j++) {
      row_of(A, A.inv[identity ? j : idx[j]], cold_all, row.data());
      if (memcmp(row.data(), blob + (size_t)j * S, sizeof(double) * S)) return fprintf(stderr, "warm_state_harness: export round %d: row %d differs\n", round, j), 1;
    }
    for (size_t j = 0; j < sizeof(double) * n * S; j++) g_sum = (g_sum ^ ((const unsigned char*)blob)[j]) * 1099511628211ull;
    State H(C2), E(C2);
    wg256("k_ws_import", blocks, [&] { k_ws_import(H.W, identity ? nullptr : to.data(), H.inv, n, blob, H.cold); });
    for (int j = 0; j < n; j++) row_into(E, E.inv[identity ? j : to[j]], blob + (size_t)j * S);
    same(H, E, round == 0 ? "import all" : round == 1 ? "import 13" : "import identity, cold");
    free(blob);
  }
  printf("done %016llx\n", (unsigned long long)g_sum);
  return 0;
}
