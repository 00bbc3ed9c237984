// harness.cpp — TEST INFRASTRUCTURE: the solver's device code (csrc/*.h) compiled as host C++ and run under AddressSanitizer +
// UndefinedBehaviorSanitizer with every work buffer filled with NaN bit patterns and allocated at its exact size (VERDICT r1 item
// 4: zero-filled device buffers would hide reads of words no kernel has written; the pool's GPUs run no sanitizer).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLTOMPC_HOST_HARNESS -I<csrc> -I<harness> ...
// Reads a problem from a text file (tables, x0 batch, horizon, options; sections `rows`, `cot`, `u`), runs the interior-point
// iterations with the launch sequence of ltompc_make_step_dev, prints status / iterations / u0 per instance.  tests/test_host_harness*.py compare that with the oracle and the dense references.  key=value arguments:
//   riccati=serial|8|1|1q  k_riccati (default; LTOMPC_RICCATI=serial), k_riccati8 over Bp / 8 waves, k_riccati1 one wave per instance,
//                        k_riccati1q one workgroup of four wavefronts per instance (dynamic LDS of exactly ric1q_lds_bytes(N))
//   step=1               k_step1 (320 lanes per listed instance) instead of k_linesearch / k_pick / k_linesearch / k_pick / k_update
//   eval=slot|8          k_eval / k_expand (default) or k_eval8 / k_expand8
//   compact=1|kernel     the instance list is the stable compaction of the unfinished instances after every iteration: made by a
//                        host loop (1) or by k_compact itself with ping-pong lists (kernel)
//   pack=1 pack_min=<n>  re-packing by the library's rule: k_pack_perm + k_pack while the launch is wider than n (the library: 512),
//                        k_compact below; the packed order is kept between ticks; k_pack_inverse + k_pack after the last tick
//   rollout=<ticks>      ltompc_rollout_dev's loop on one stream (k_roll_begin / _mark / _init / _finish / _plant, k_compact on SI_FINAL)
//   wave_order=asc|desc  the order in which the wavefronts of a workgroup run between two barriers (hip_shim.h)
//   final=1              one more block after the last tick: the state the run leaves behind
//   - selftest=<case>, - scan   (no problem file) the executor's self-test; k_compact / k_pack_perm against a plain stable partition
//   section rows         per-instance rows through k_theta_rows, WorkPI and the _pi kernels; param.<field>=<value> for uniform runs
//   derivs=1 dump=<file> after each tick's solve the passes of sens_compute / psens_compute / adj_compute, everything as raw doubles
//   loop=<mode>          with derivs=1: k_loop_begin, per tick k_plant_sens and k_loop_accum
//   plant_sens=<n_sub>   k_plant_sens + k_planes_rows at the states of the batch and the controls of section u
//   model_eps=<eps>, slip=1, ellipse=1   k_test_model / k_slip_forces / k_test_ellipse at given points (tests/test_synthetic_tracks.py)
//   velocity             (the only argument, with a file of its own format: velocity_mode below) k_velocity_profile
// What runs: the thread-per-slot kernels lane after lane; on the lock-step wavefront of hip_shim.h k_riccati8, k_riccati1,
// k_eval8, k_expand8, k_pick, k_sens_eval8, k_sens_riccati8, k_sens_forward, k_psens_sweep, k_adj_sweep; on its lock-step
// workgroup of several wavefronts k_riccati1q, k_step1, k_compact, k_pack_perm; the _pi form of each; k_pack, k_pack_inverse and
// the rollout kernels lane after lane.  Not modelled: several lanes adding to one LDS word in the same instruction, the ordering
// of global memory between workgroups, the rollout's two streams (the plant kernel of a pass runs after the pass).
// NOT a product path and not an oracle: nothing in the package or in bench.py uses it.
#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"
#include "rollout.h"
#include "velocity.h"
#include "eval8.h"
#include "sensitivity.h"
#include "param_sensitivity.h"
#include "adjoint.h"
#include "plant_sensitivity.h"

#include <string>
#include <type_traits>
#include <vector>

using namespace ltompc;

static double* poisoned(size_t n) {
  double* p = (double*)malloc(n * sizeof(double));
  memset(p, 0xFF, n * sizeof(double));  // NaN as doubles (LTOMPC_POISON=1 on the device)
  return p;
}
static int* ipoisoned(size_t n, int fill) {
  int* p = (int*)malloc(n * sizeof(int));
  for (size_t i = 0; i < n; i++) p[i] = fill;
  return p;
}
static void default_params(ltompc_params* p) {  // = ltompc_default_params (ltompc.hip)
  memset(p, 0, sizeof *p);
  p->mass = 1000.0, p->inertia_z = 1000.0, p->length_f = 1.5, p->length_r = 1.5, p->width = 2.3;
  p->B_f = 10.0, p->C_f = 1.3, p->D_f = 1.0, p->B_r = 12.0, p->C_r = 1.2, p->D_r = 1.0;
  p->C_m = 1000.0, p->Cr_0 = 0.01, p->Cr_2 = 0.0003, p->gravity = 9.81;
  p->q_n = 0.5, p->q_mu = 3.0, p->q_vy = 1.0, p->q_v = 1.0, p->vref_scale = 0.6, p->q_B = 1e-2;
  p->r_du[0] = p->r_du[1] = 1e-2;
  for (int i = 0; i < NX; i++) p->x_lb[i] = -LTOMPC_NO_BOUND, p->x_ub[i] = LTOMPC_NO_BOUND;
  const double pi = 3.14159265358979323846;
  p->x_lb[0] = 0.0, p->x_lb[2] = -pi * 0.5, p->x_ub[2] = pi * 0.5, p->x_lb[3] = 0.0;
  p->x_lb[6] = -pi / 4, p->x_ub[6] = pi / 4, p->x_lb[7] = -1.0, p->x_ub[7] = 1.0;
  p->u_lb[0] = -2 * pi / 4, p->u_ub[0] = 2 * pi / 4, p->u_lb[1] = -1.0, p->u_ub[1] = 1.0;
}
static void default_options(ltompc_options* o) {  // = ltompc_default_options
  memset(o, 0, sizeof *o);
  o->t_step = 0.1, o->tol = 1e-8, o->acceptable_tol = 1e-6, o->mu_init = 0.1, o->mu_min = 1e-9;
  o->kappa_eps = 10, o->kappa_mu = 0.2, o->theta_mu = 1.5, o->tau_min = 0.99, o->bound_push = 1e-2;
  o->s_max = 100, o->delta_w_first = 1e-4, o->smooth_eps_min = 1e-4, o->smooth_scale = 1.0;
  o->max_iter = 1000, o->acceptable_iter = 15, o->n_linesearch = 8, o->stall_iter = 15, o->max_ls_fail = 8;
  o->warm_reset_on_fail = 1, o->resto_rho = 1000.0;
  o->resto_rho_max = 1e6, o->resto_rho_factor = 1e3, o->dual_inf_max = 1e4, o->max_mu_stay = 100, o->infeasible_sticky = 1, o->node0_check = 1, o->warm_fallback_iter = 25, o->resto_shift_retry = 1;
}
// further options as key=value arguments (tests of the option paths)
static bool set_option(ltompc_options* o, const char* arg) {
  const char* eq = strchr(arg, '=');
  if (!eq) return false;
  const std::string key(arg, eq - arg);
  const double v = atof(eq + 1);
#define OPT_D(name) if (key == #name) { o->name = v; return true; }
#define OPT_I(name) if (key == #name) { o->name = (int)v; return true; }
  OPT_D(dual_inf_max) OPT_D(resto_rho) OPT_D(resto_rho_max) OPT_D(resto_rho_factor) OPT_D(mu_init_warm) OPT_D(tol) OPT_D(mu_init)
  OPT_I(infeasible_sticky) OPT_I(max_mu_stay) OPT_I(node0_check) OPT_I(warm_fallback_iter) OPT_I(resto_shift_retry) OPT_I(warm_shift) OPT_I(resto_sticky) OPT_I(max_iter)
  OPT_I(warm_reset_on_fail) OPT_I(stall_iter)
#undef OPT_D
#undef OPT_I
  return false;
}
static void build_bounds(const ltompc_params& p, Bounds& b) {  // = build_bounds (ltompc.hip)
  memset(&b, 0, sizeof b);
  for (int i = 0; i < NX; i++) {
    if (p.x_lb[i] > -LTOMPC_NO_BOUND) b.xb_idx[b.n_xb] = i, b.xb_sgn[b.n_xb] = -1.0, b.xb_val[b.n_xb] = p.x_lb[i], b.n_xb++;
    if (p.x_ub[i] < LTOMPC_NO_BOUND) b.xb_idx[b.n_xb] = i, b.xb_sgn[b.n_xb] = +1.0, b.xb_val[b.n_xb] = p.x_ub[i], b.n_xb++;
  }
  for (int i = 0; i < NU; i++) {
    if (p.u_lb[i] > -LTOMPC_NO_BOUND) b.ub_idx[b.n_ub] = i, b.ub_sgn[b.n_ub] = -1.0, b.ub_val[b.n_ub] = p.u_lb[i], b.n_ub++;
    if (p.u_ub[i] < LTOMPC_NO_BOUND) b.ub_idx[b.n_ub] = i, b.ub_sgn[b.n_ub] = +1.0, b.ub_val[b.n_ub] = p.u_ub[i], b.n_ub++;
  }
  b.nel = p.ell_penalty > 0.0 ? NEL : 0;
  b.ni = b.n_ub + 2 * b.n_xb + NNL + b.nel;
}

// run a thread-per-(k, b) kernel body over a grid of `threads` threads, 64 per block
template <typename F>
static void grid64(int threads, F&& body) {
  blockDim.x = 64, gridDim.x = (threads + 63) / 64;
  for (unsigned blk = 0; blk < gridDim.x; blk++)
    for (unsigned t = 0; t < 64; t++) blockIdx.x = blk, threadIdx.x = t, body();
}

// ... with blocks of `bs` threads (kernels that index with blockDim.x)
template <typename F>
static void grid_bs(size_t threads, unsigned bs, F&& body) {
  blockDim.x = bs, gridDim.x = (unsigned)((threads + bs - 1) / bs);
  for (unsigned blk = 0; blk < gridDim.x; blk++)
    for (unsigned t = 0; t < bs; t++) blockIdx.x = blk, threadIdx.x = t, body();
  blockDim.x = 64;
}
static double* zeros(size_t n) { return (double*)calloc(n ? n : 1, sizeof(double)); }  // (what the library allocates without `work`)
// run a kernel body on the lock-step workgroup of hip_shim.h, the blocks one after the other: `threads` lanes (a multiple of 64)
// per block, fiber stacks of `stack` bytes, and `extern __shared__` of lds_bytes (0: none) as a fresh NaN-filled buffer of
// exactly that size for every block
template <typename F>
static void wg(const char* name, int blocks, int threads, size_t lds_bytes, size_t stack, F&& body) {
  blockDim.x = threads, gridDim.x = blocks;
  for (int blk = 0; blk < blocks; blk++) {
    blockIdx.x = blk;
    void* lds = nullptr;
    if (lds_bytes) lds = malloc(lds_bytes), memset(lds, 0xFF, lds_bytes);
    lt_dyn_lds = lds;
    LtWave::self().run(name, threads / 64, stack, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, &body);
    lt_dyn_lds = nullptr;
    free(lds);
  }
  blockDim.x = 64;
}
// ... one wavefront per block
template <typename F>
static void wave64(const char* name, int blocks, F&& body) { wg(name, blocks, 64, 0, LtWave::STACK, body); }
template <typename F>
static void wave64y(const char* name, int bx, int by, F&& body) {  // grid (bx, by)
  gridDim.y = by;
  for (int y = 0; y < by; y++) blockIdx.y = y, wave64(name, bx, body);
  gridDim.y = 1, blockIdx.y = 0;
}
template <typename F>
static void wave64_lds(const char* name, int blocks, size_t lds_bytes, F&& body) { wg(name, blocks, 64, lds_bytes, LtWave::STACK, body); }
// ... the 1024-lane scan kernels (k_compact, k_pack_perm): one block, small stacks
template <typename F>
static void scan1024(const char* name, F&& body) { wg(name, 1, 1024, 0, LtWave::STACK_SMALL, body); }
// the 16 fields of theta (ltompc_get_param_sensitivities' columns): param.<name>=<value>
static const char* const THETA_NAMES[LTOMPC_NTHETA] = {"mass", "inertia_z", "B_f", "C_f", "D_f", "B_r", "C_r", "D_r", "C_m", "Cr_0", "Cr_2",
                                                       "q_n", "q_mu", "q_B", "r_du0", "r_du1"};
static void theta_of(const ltompc_params& p, double* t) {  // = theta_of (ltompc.hip)
  const double v[LTOMPC_NTHETA] = {p.mass, p.inertia_z, p.B_f, p.C_f, p.D_f, p.B_r, p.C_r, p.D_r, p.C_m, p.Cr_0, p.Cr_2,
                                   p.q_n, p.q_mu, p.q_B, p.r_du[0], p.r_du[1]};
  memcpy(t, v, sizeof v);
}
static bool set_param(ltompc_params* p, const char* arg) {
  const char* eq = strchr(arg, '=');
  if (!eq || strncmp(arg, "param.", 6)) return false;
  const std::string key(arg + 6, eq - arg - 6);
  double* const f[LTOMPC_NTHETA] = {&p->mass, &p->inertia_z, &p->B_f, &p->C_f, &p->D_f, &p->B_r, &p->C_r, &p->D_r, &p->C_m, &p->Cr_0, &p->Cr_2,
                                    &p->q_n, &p->q_mu, &p->q_B, &p->r_du[0], &p->r_du[1]};
  for (int j = 0; j < LTOMPC_NTHETA; j++)
    if (key == THETA_NAMES[j]) return *f[j] = atof(eq + 1), true;
  return false;
}

// velocity mode: `harness profiles.txt velocity`.  The file: kind n_map mass friction_coef lam D T C_m Cr_0 Cr_2, map_v[16], map_f[16],
// the number of launches, and per launch n, batch, s [batch][n], k [batch][n], s_max [batch].  k_velocity_profile on exact-size inputs
// and NaN-poisoned exact-size outputs; per launch a `tick` line and one line v[n] v_local[n] v_acclim[n] v_declim[n] per profile.
static int velocity_mode(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  ltompc_vp_vehicle V;
  memset(&V, 0, sizeof V);
  if (fscanf(f, "%d %d %lf %lf %lf %lf %lf %lf %lf %lf", &V.kind, &V.n_map, &V.mass, &V.friction_coef, &V.lam, &V.D, &V.T, &V.C_m, &V.Cr_0, &V.Cr_2) != 10) return 2;
  for (int i = 0; i < 16; i++) if (fscanf(f, "%lf", &V.map_v[i]) != 1) return 2;
  for (int i = 0; i < 16; i++) if (fscanf(f, "%lf", &V.map_f[i]) != 1) return 2;
  int launches;
  if (fscanf(f, "%d", &launches) != 1) return 2;
  for (int l = 0; l < launches; l++) {
    int n, batch;
    if (fscanf(f, "%d %d", &n, &batch) != 2) return 2;
    const size_t m = (size_t)n * batch;
    double *s = (double*)malloc(sizeof(double) * m), *k = (double*)malloc(sizeof(double) * m), *sm = (double*)malloc(sizeof(double) * batch);
    for (size_t i = 0; i < m; i++) if (fscanf(f, "%lf", &s[i]) != 1) return 2;
    for (size_t i = 0; i < m; i++) if (fscanf(f, "%lf", &k[i]) != 1) return 2;
    for (int i = 0; i < batch; i++) if (fscanf(f, "%lf", &sm[i]) != 1) return 2;
    double* out[4];
    for (auto& o : out) o = poisoned(m);
    grid64(batch, [&] { k_velocity_profile(V, n, batch, s, k, sm, out[0], out[1], out[2], out[3]); });
    printf("tick %d\n", l);
    for (int b = 0; b < batch; b++) {
      for (auto& o : out)
        for (int i = 0; i < n; i++) printf("%.17g ", o[(size_t)b * n + i]);
      printf("\n");
    }
    free(s), free(k), free(sm);
    for (auto& o : out) free(o);
  }
  fclose(f);
  return 0;
}

// ---- self-test of the lock-step workgroup (hip_shim.h): `harness - selftest=<case> [wave_order=asc|desc]`.  A kernel of two
// wavefronts, here and not in csrc/: thread 64 (wavefront 1) writes an LDS word, thread 0 (wavefront 0) reads it.
//   barrier           a __syncthreads() between the write and the read: both wavefront orders print `value 7`
//   nobarrier         the barrier compiled out: the orders print different values - how a missing barrier shows
//   diverged_barrier  a barrier inside `if (threadIdx.x < 64)` while the other lanes wait at a later one: MISMATCHED, exit status 3
//   diverged_shfl     a __shfl that half a wavefront reaches while the other half has returned: MISMATCHED, exit status 3
enum { SELF_BARRIER = 0, SELF_NOBARRIER, SELF_DIVERGED_BARRIER, SELF_DIVERGED_SHFL };
template <int CASE>
__global__ void k_selftest(int* out) {
  __shared__ int word;
  const int t = threadIdx.x;
  if (t == 0) word = 0;
  __syncthreads();
  if (CASE == SELF_DIVERGED_SHFL) {
    if ((t & 63) < 32) out[0] = __shfl(t, 0);
    return;
  }
  if (t == 64) word = 7;
  if (CASE == SELF_DIVERGED_BARRIER) {
    if (t < 64) __syncthreads();
  }
  if (CASE != SELF_NOBARRIER) __syncthreads();
  if (t == 0) out[0] = word;
}
static int selftest_mode(const char* which) {
  int out[1] = {-1};
  const std::string c(which);
  if (c == "barrier") wg("k_selftest<barrier>", 1, 128, 0, LtWave::STACK_SMALL, [&] { k_selftest<SELF_BARRIER>(out); });
  else if (c == "nobarrier") wg("k_selftest<nobarrier>", 1, 128, 0, LtWave::STACK_SMALL, [&] { k_selftest<SELF_NOBARRIER>(out); });
  else if (c == "diverged_barrier") wg("k_selftest<diverged_barrier>", 1, 128, 0, LtWave::STACK_SMALL, [&] { k_selftest<SELF_DIVERGED_BARRIER>(out); });
  else if (c == "diverged_shfl") wg("k_selftest<diverged_shfl>", 1, 128, 0, LtWave::STACK_SMALL, [&] { k_selftest<SELF_DIVERGED_SHFL>(out); });
  else return fprintf(stderr, "harness: selftest=barrier|nobarrier|diverged_barrier|diverged_shfl\n"), 2;
  printf("value %d\n", out[0]);
  return 0;
}

// ---- scan mode: `harness - scan [wave_order=asc|desc]`.  k_compact and k_pack_perm outside a solve, on flag arrays of the sizes
// 0, 1, 9, 1023, 1024, 1025 and 2500 (above 1024 a thread's chunk is 2 or 3 elements and the last threads' chunks are empty) with
// the patterns all finished / none finished / alternating / only the last element unfinished / seeded random, against a plain
// stable partition.  Every array at its exact size (the outputs too: dst has as many entries as there are unfinished elements),
// the outputs filled with -1.  One line per case with the outputs' sums; a difference ends the run with exit status 1.
static int* exact_ints(const std::vector<int>& v) {
  int* p = (int*)malloc(v.size() * sizeof(int));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(int));
  return p;
}
static int scan_mode() {
  const int sizes[] = {0, 1, 9, 1023, 1024, 1025, 2500};
  const char* const patterns[] = {"all_finished", "none_finished", "alternating", "last_unfinished", "random"};
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  const auto next = [&] { return rng = rng * 6364136223846793005ull + 1442695040888963407ull, (unsigned)(rng >> 33); };
  int bad = 0;
  for (const int n : sizes)
    for (int pat = 0; pat < 5; pat++) {
      std::vector<int> flag(n);  // finished?
      for (int j = 0; j < n; j++) flag[j] = pat == 0 ? 1 : pat == 1 ? 0 : pat == 2 ? (j & 1) : pat == 3 ? (j != n - 1) : (int)(next() & 1);
      // k_compact: a list of n distinct instances (a seeded permutation of 0 .. n + 6, so that list position != instance index)
      const int M = n + 7;
      std::vector<int> ids(M), src(n), done(M, 1);
      for (int j = 0; j < M; j++) ids[j] = j;
      for (int j = M - 1; j > 0; j--) std::swap(ids[j], ids[next() % (j + 1)]);
      for (int j = 0; j < n; j++) src[j] = ids[j], done[ids[j]] = flag[j];
      std::vector<int> want;
      for (int j = 0; j < n; j++)
        if (!flag[j]) want.push_back(src[j]);
      {
        int *d_src = exact_ints(src), *d_done = exact_ints(done), *d_n = exact_ints({n});
        int *dst = exact_ints(std::vector<int>(want.size(), -1)), *ndst = exact_ints({-1});
        scan1024("k_compact", [&] { k_compact(d_src, d_n, d_done, dst, ndst); });
        bool ok = ndst[0] == (int)want.size();
        long long sum = 0;
        for (size_t j = 0; j < want.size(); j++) ok = ok && dst[j] == want[j], sum += (long long)(j + 1) * dst[j];
        printf("k_compact n=%d %s ndst=%d sum=%lld %s\n", n, patterns[pat], ndst[0], sum, ok ? "ok" : "MISMATCH");
        bad += !ok;
        free(d_src), free(d_done), free(d_n), free(dst), free(ndst);
      }
      // k_pack_perm: the first n slots, unfinished ones first (stable), then the finished ones (stable); act = identity over the unfinished
      std::vector<int> perm_want;
      for (int j = 0; j < n; j++)
        if (!flag[j]) perm_want.push_back(j);
      const int n_act = (int)perm_want.size();
      for (int j = 0; j < n; j++)
        if (flag[j]) perm_want.push_back(j);
      {
        int *d_done = exact_ints(flag), *d_n = exact_ints({n});
        int *perm = exact_ints(std::vector<int>(n, -1)), *act = exact_ints(std::vector<int>(n_act, -1)), *nact = exact_ints({-1});
        scan1024("k_pack_perm", [&] { k_pack_perm(d_n, d_done, perm, act, nact); });
        bool ok = nact[0] == n_act;
        long long sum = 0;
        for (int j = 0; j < n; j++) ok = ok && perm[j] == perm_want[j], sum += (long long)(j + 1) * perm[j];
        for (int j = 0; j < n_act; j++) ok = ok && act[j] == j;
        printf("k_pack_perm n=%d %s nact=%d sum=%lld %s\n", n, patterns[pat], nact[0], sum, ok ? "ok" : "MISMATCH");
        bad += !ok;
        free(d_done), free(d_n), free(perm), free(act), free(nact);
      }
    }
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: harness problem.txt\n"), 2;
  if (argc == 3 && !strcmp(argv[2], "velocity")) return velocity_mode(argv[1]);
  for (int a = 2; a < argc; a++)  // wave_order=asc|desc: the order in which the wavefronts of a workgroup run between two barriers (hip_shim.h)
    if (!strncmp(argv[a], "wave_order=", 11)) {
      const std::string v(argv[a] + 11);
      if (v != "asc" && v != "desc") return fprintf(stderr, "harness: wave_order=asc|desc\n"), 2;
      LtWave::self().desc_waves = v == "desc";
    }
  if (argc >= 3 && !strncmp(argv[2], "selftest=", 9)) return selftest_mode(argv[2] + 9);
  if (argc >= 3 && !strcmp(argv[2], "scan")) return scan_mode();
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int nt, N, B, any_bounds, ticks;
  double soft_rho;
  double ell[4];
  if (fscanf(f, "%d %d %d %d %lf %d %lf %lf %lf %lf", &nt, &N, &B, &any_bounds, &soft_rho, &ticks, &ell[0], &ell[1], &ell[2], &ell[3]) != 10) return 2;
  std::vector<double> tab((size_t)6 * nt), x0((size_t)8 * B);
  for (auto& v : tab) if (fscanf(f, "%lf", &v) != 1) return 2;
  for (auto& v : x0) if (fscanf(f, "%lf", &v) != 1) return 2;
  // optional sections after the batch: `rows` B x 16 per-instance rows; `cot` n, then n cotangents gX [B][N+1][8], gU [B][N][2];
  // `u` B x 2 controls (plant_sens mode)
  std::vector<double> extra, cot, u_in;
  int n_cot = 0;
  for (char tag[64]; fscanf(f, "%63s", tag) == 1;) {
    std::vector<double>* dst = nullptr;
    size_t cnt = 0;
    if (!strcmp(tag, "rows")) dst = &extra, cnt = (size_t)LTOMPC_NTHETA * B;
    else if (!strcmp(tag, "u")) dst = &u_in, cnt = (size_t)2 * B;
    else if (!strcmp(tag, "cot")) {
      if (fscanf(f, "%d", &n_cot) != 1) return 2;
      dst = &cot, cnt = (size_t)n_cot * B * ((size_t)(N + 1) * 8 + (size_t)N * 2);
    } else return fprintf(stderr, "harness: unknown section %s\n", tag), 2;
    dst->resize(cnt);
    for (auto& v : *dst) if (fscanf(f, "%lf", &v) != 1) return 2;
  }
  fclose(f);
  Consts K;
  memset(&K, 0, sizeof K);
  default_params(&K.p), default_options(&K.o);
  K.o.soft_rho = soft_rho;
  double model_eps = -1.0;  // model_eps=<eps>: model mode (below) instead of solves
  int ric = 0;              // riccati=serial|8|1: k_riccati (LTOMPC_RICCATI=serial), k_riccati8 over Bp / 8 waves, k_riccati1 with one wave per listed instance
  bool eval8 = false;       // eval=slot|8: k_eval / k_expand or k_eval8 / k_expand8
  bool derivs = false;      // derivs=1: after each tick's solve the sensitivity, parameter-sensitivity and adjoint passes; everything to dump=<file>
  int loop_mode = 0;        // loop=<mode> (with derivs=1): k_loop_begin, one k_loop_accum per tick
  int plant_sens = 0;       // plant_sens=<n_sub>: k_plant_sens + k_planes_rows at the states of the batch and the controls of section `u`
  const char* dump_path = nullptr;
  bool slip_mode = false, ellipse_mode = false;  // slip=1 / ellipse=1: k_slip_forces / k_test_ellipse at the states of the batch (below)
  bool compact = false;     // compact=1: the instance list is the stable compaction of the unfinished instances (what k_compact computes)
  bool compact_kernel = false;  // compact=kernel: ... made by k_compact itself (1024 lanes), ping-pong lists as in ltompc_make_step_dev
  bool ric1q = false;       // riccati=1q: k_riccati1q, one workgroup of four wavefronts per listed instance
  bool step1 = false;       // step=1: k_step1 (320 lanes per listed instance) instead of k_linesearch / k_pick / k_linesearch / k_pick / k_update
  bool pack = false;        // pack=1: re-packing by the library's rule (k_pack_perm, k_pack; the order is kept between ticks), un-packing at the end
  int pack_min = 512;       // pack_min=<n>: launches wider than this move the instances, narrower ones only compact the list (the library: 512)
  const int pack_num = 6;   // (ltompc.hip: re-pack when at most pack_num / 8 of the launch width is unfinished)
  int rollout = 0;          // rollout=<ticks>: the loop of ltompc_rollout_dev, rendered sequentially, instead of synchronous ticks
  bool final_block = false; // final=1: after the last tick one more block with the state the run leaves behind
  for (int a = 2; a < argc; a++) {
    if (!strncmp(argv[a], "model_eps=", 10)) { model_eps = atof(argv[a] + 10); continue; }
    if (!strncmp(argv[a], "riccati=", 8)) {
      const std::string v(argv[a] + 8);
      ric = v == "serial" ? 0 : v == "8" ? 8 : (v == "1" || v == "1q") ? 1 : -1, ric1q = v == "1q";
      if (ric < 0) return fprintf(stderr, "harness: riccati=serial|8|1|1q\n"), 2;
      continue;
    }
    if (!strncmp(argv[a], "eval=", 5)) {
      const std::string v(argv[a] + 5);
      if (v != "slot" && v != "8") return fprintf(stderr, "harness: eval=slot|8\n"), 2;
      eval8 = v == "8";
      continue;
    }
    if (!strncmp(argv[a], "compact=", 8)) { compact_kernel = !strcmp(argv[a] + 8, "kernel"), compact = atoi(argv[a] + 8) != 0; continue; }
    if (!strncmp(argv[a], "step=", 5)) { step1 = atoi(argv[a] + 5) != 0; continue; }
    if (!strncmp(argv[a], "pack=", 5)) { pack = atoi(argv[a] + 5) != 0; continue; }
    if (!strncmp(argv[a], "pack_min=", 9)) { pack_min = atoi(argv[a] + 9); continue; }
    if (!strncmp(argv[a], "rollout=", 8)) { rollout = atoi(argv[a] + 8); continue; }
    if (!strncmp(argv[a], "final=", 6)) { final_block = atoi(argv[a] + 6) != 0; continue; }
    if (!strncmp(argv[a], "wave_order=", 11)) continue;  // (read before the modes)
    if (!strncmp(argv[a], "derivs=", 7)) { derivs = atoi(argv[a] + 7) != 0; continue; }
    if (!strncmp(argv[a], "loop=", 5)) { loop_mode = atoi(argv[a] + 5); continue; }
    if (!strncmp(argv[a], "plant_sens=", 11)) { plant_sens = atoi(argv[a] + 11); continue; }
    if (!strncmp(argv[a], "dump=", 5)) { dump_path = argv[a] + 5; continue; }
    if (!strncmp(argv[a], "slip=", 5)) { slip_mode = atoi(argv[a] + 5) != 0; continue; }
    if (!strncmp(argv[a], "ellipse=", 8)) { ellipse_mode = atoi(argv[a] + 8) != 0; continue; }
    if (set_param(&K.p, argv[a])) continue;
    if (!set_option(&K.o, argv[a])) return fprintf(stderr, "harness: unknown option %s\n", argv[a]), 2;
  }
  K.p.ell_penalty = ell[0], K.p.ell_rho = ell[1], K.p.ell_D_f = ell[2], K.p.ell_D_r = ell[3];
  build_bounds(K.p, K.bd);
  const int ni = K.bd.ni, Bp = (B + 63) / 64 * 64;
  double* d_tab = (double*)malloc(sizeof(double) * 6 * nt);  // exact size: ASan sees any look-up outside the tables
  memcpy(d_tab, tab.data(), sizeof(double) * 6 * nt);
  Tables& T = K.T;
  T.n = nt, T.s_kappa = d_tab, T.kappa = d_tab + nt, T.s_arc = d_tab + 2 * nt, T.n_left = d_tab + 3 * nt, T.n_right = d_tab + 4 * nt, T.v_ref = d_tab + 5 * nt;
  T.g0_kappa = tab[0], T.inv_kappa = (double)(nt - 1) / (tab[nt - 1] - tab[0]);
  T.g0_arc = tab[2 * (size_t)nt], T.inv_arc = (double)(nt - 1) / (tab[3 * (size_t)nt - 1] - tab[2 * (size_t)nt]);
  T.period = 0.0;
  if (model_eps >= 0.0) {
    // Model mode: the batch is B / 2 states followed by B / 2 rows of multipliers.  k_test_model (the kernel behind
    // ltompc_test_model) at those points with smoothing length model_eps, every output in a NaN-poisoned buffer of its exact
    // size; one line per point: f[8] J[64] H[64] cval[2] cgrad[16] cH[128] gval[3] ggrad[24] gH[192].
    const int n = B / 2;
    const size_t sz[9] = {8, 64, 64, 2, 16, 128, 3, 24, 192};
    double* out[9];
    for (int i = 0; i < 9; i++) out[i] = poisoned(sz[i] * n);
    double *xs = (double*)malloc(sizeof(double) * 8 * n), *ls = (double*)malloc(sizeof(double) * 8 * n);
    memcpy(xs, x0.data(), sizeof(double) * 8 * n), memcpy(ls, x0.data() + (size_t)8 * n, sizeof(double) * 8 * n);
    const Consts Kc = K;
    grid64(n, [&] { k_test_model(Kc, n, model_eps, xs, ls, out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8]); });
    printf("tick 0\n");
    for (int t = 0; t < n; t++) {
      for (int i = 0; i < 9; i++)
        for (size_t j = 0; j < sz[i]; j++) printf("%.17g ", out[i][t * sz[i] + j]);
      printf("\n");
    }
    return 0;
  }
  if (slip_mode || ellipse_mode) {
    // k_slip_forces: one line alpha[2] Fy[2] per state; k_test_ellipse (params.ell_* of the header line): val[2] grad[16] H[128].
    // Inputs and outputs in buffers of their exact sizes, the outputs NaN-poisoned.
    double* xs = (double*)malloc(sizeof(double) * 8 * B);
    memcpy(xs, x0.data(), sizeof(double) * 8 * B);
    const Consts Kc = K;
    const size_t sz[3] = {slip_mode ? (size_t)2 : 2, slip_mode ? (size_t)2 : 16, slip_mode ? (size_t)0 : 128};
    double* out[3];
    for (int i = 0; i < 3; i++) out[i] = poisoned(sz[i] * B + (sz[i] ? 0 : 1));
    if (slip_mode) grid64(B, [&] { k_slip_forces(Kc, B, xs, out[0], out[1]); });
    else grid64(B, [&] { k_test_ellipse(Kc, B, xs, out[0], out[1], out[2]); });
    printf("tick 0\n");
    for (int t = 0; t < B; t++) {
      for (int i = 0; i < 3; i++)
        for (size_t j = 0; j < sz[i]; j++) printf("%.17g ", out[i][t * sz[i] + j]);
      printf("\n");
    }
    return 0;
  }
  Work W;
  memset(&W, 0, sizeof W);
  W.N = N, W.B = B, W.Bp = Bp;
  const size_t n = N, bp = Bp;
  // EXACT sizes (no "+64" slack as in ltompc_create: an over-read past a buffer is an ASan error here)
  W.X = poisoned(8 * (n + 1) * bp), W.C = poisoned(8 * n * bp), W.U = poisoned(2 * n * bp), W.L1 = poisoned(8 * n * bp), W.L2 = poisoned(8 * n * bp);
  const size_t nel = K.bd.nel;
  W.T = poisoned((ni + NNL + nel) * n * bp), W.NU = poisoned(ni * n * bp);
  W.dX = poisoned(8 * (n + 1) * bp), W.dC = poisoned(8 * n * bp), W.dU = poisoned(2 * n * bp), W.nL1 = poisoned(8 * n * bp), W.nL2 = poisoned(8 * n * bp);
  W.dT = poisoned((ni + NNL + nel) * n * bp), W.dNU = poisoned(ni * n * bp);
  W.QP = poisoned((size_t)QP_NF * (n + 1) * bp), W.RC = poisoned((size_t)RC_NF * (n + 1) * bp);
  W.RS = poisoned((size_t)RS_NF * n * bp), W.SP = poisoned((size_t)SP_NF * n * bp), W.LS = poisoned((size_t)3 * (K.o.n_linesearch + 1) * n * bp);
  W.x0 = poisoned(8 * bp), W.uprev = poisoned(2 * bp), W.st = poisoned((size_t)ST_NF * bp), W.filt = poisoned((size_t)2 * FILTER_MAX * bp);
  W.si = ipoisoned((size_t)SI_NF * bp, 0), W.active = ipoisoned(K.o.max_iter + 2, 0), W.ls_list = ipoisoned(bp, -1), W.ls_count = ipoisoned(4, 0);
  W.DBG = nullptr;
  W.BK = poisoned(18 * n * bp);
  int* const d_orig = ipoisoned(bp, -1);  // slot -> caller's index (pack=1 permutes it with the instances)
  for (int b = 0; b < B; b++) d_orig[b] = b;
  W.orig = d_orig;
  int* const d_perm = ipoisoned(bp, -1);
  bool packed = false;
  int n_packs = 0;  // re-packings that moved instances (final=1 prints it: a test of pack=1 that never packed would prove nothing)
  const bool ref = !any_bounds, el = K.bd.nel > 0;
  // Per-instance rows (ltompc_set_instance_params): a [16][Bp] plane with the handle's values in every column (theta_prepare),
  // the rows through k_theta_rows, WorkPI = W + TH (sync_pi_work) and the _pi kernels on every path below.
  const bool PI = !extra.empty();
  WorkPI Wpi;
  memset(&Wpi, 0, sizeof Wpi);
  double* d_th = nullptr;
  if (PI) {
    if (extra.size() != (size_t)LTOMPC_NTHETA * B) return fprintf(stderr, "harness: %zu values after the batch, expected B x 16 rows\n", extra.size()), 2;
    if (el || ric == 0) return fprintf(stderr, "harness: rows need riccati=8|1 and no friction ellipse (as the library)\n"), 2;
    d_th = (double*)malloc(sizeof(double) * LTOMPC_NTHETA * bp);
    double t[LTOMPC_NTHETA];
    theta_of(K.p, t);
    for (int j = 0; j < LTOMPC_NTHETA; j++)
      for (size_t b = 0; b < bp; b++) d_th[j * bp + b] = t[j];
    double* rows = (double*)malloc(sizeof(double) * extra.size());
    memcpy(rows, extra.data(), sizeof(double) * extra.size());
    blockDim.x = 256, gridDim.x = (B * LTOMPC_NTHETA + 255) / 256;
    for (unsigned blk = 0; blk < gridDim.x; blk++)
      for (unsigned t2 = 0; t2 < 256; t2++) blockIdx.x = blk, threadIdx.x = t2, k_theta_rows(rows, d_th, B, Bp);
    free(rows);
    static_cast<Work&>(Wpi) = W, Wpi.TH = d_th;
  }
  std::vector<int> act(Bp), nact(1, B);
  for (int b = 0; b < Bp; b++) act[b] = b;
  // exact sizes for the list as well (the library's lists have Bp entries)
  int* const d_actl[2] = {ipoisoned(bp, -1), ipoisoned(bp, -1)};  // (ping-pong, as the library's d_act / d_nact)
  int* const d_nactl[2] = {ipoisoned(1, B), ipoisoned(1, 0)};
  memcpy(d_actl[0], act.data(), sizeof(int) * bp);
  int cur = 0;
  Launch la{d_actl[0], d_nactl[0], Bp, 0};
  int n_launch = B;
  const auto set_list = [&](const int c, const int n) { cur = c, la.act = d_actl[c], la.nact = d_nactl[c], n_launch = n; };
  // the kernels of one iteration (launch_iteration_t of ltompc.hip)
  const auto run_eval = [&] {
    if (eval8) {
      if (PI) wave64("k_eval8_pi", N * Bp / 8, [&] { k_eval8_pi(&K, &Wpi, la); });
      else wave64("k_eval8", N * Bp / 8, [&] { k_eval8(&K, &W, la); });
    } else if (PI) grid64(N * Bp, [&] { ref ? k_eval_pi<BoundsRef>(&K, &Wpi, la) : k_eval_pi<BoundsAny>(&K, &Wpi, la); });
    else grid64(N * Bp, [&] { el ? (ref ? k_eval<BoundsRef, true>(&K, &W, la) : k_eval<BoundsAny, true>(&K, &W, la)) : (ref ? k_eval<BoundsRef, false>(&K, &W, la) : k_eval<BoundsAny, false>(&K, &W, la)); });
  };
  const auto run_expand = [&] {
    if (eval8) {
      if (PI) wave64("k_expand8_pi", N * Bp / 8, [&] { k_expand8_pi(&K, &Wpi, la); });
      else wave64("k_expand8", N * Bp / 8, [&] { k_expand8(&K, &W, la); });
    } else if (PI) grid64(N * Bp, [&] { ref ? k_expand_pi<BoundsRef>(&K, &Wpi, la) : k_expand_pi<BoundsAny>(&K, &Wpi, la); });
    else grid64(N * Bp, [&] { el ? (ref ? k_expand<BoundsRef, true>(&K, &W, la) : k_expand<BoundsAny, true>(&K, &W, la)) : (ref ? k_expand<BoundsRef, false>(&K, &W, la) : k_expand<BoundsAny, false>(&K, &W, la)); });
  };
  const auto run_linesearch = [&](const int phase, const int jw, const int threads) {
    if (PI) grid64(threads, [&] { ref ? k_linesearch_pi<BoundsRef>(&K, &Wpi, la, phase, jw) : k_linesearch_pi<BoundsAny>(&K, &Wpi, la, phase, jw); });
    else grid64(threads, [&] { el ? (ref ? k_linesearch<BoundsRef, true>(&K, &W, la, phase, jw) : k_linesearch<BoundsAny, true>(&K, &W, la, phase, jw)) : (ref ? k_linesearch<BoundsRef, false>(&K, &W, la, phase, jw) : k_linesearch<BoundsAny, false>(&K, &W, la, phase, jw)); });
  };
  const auto run_pick = [&](const int phase, const int width) {  // 8 lanes per instance, 8 instances per wavefront
    if (PI) wave64("k_pick_pi", (width * 8 + 63) / 64, [&] { k_pick_pi(&K, &Wpi, la, phase); });
    else wave64("k_pick", (width * 8 + 63) / 64, [&] { k_pick(&K, &W, la, phase); });
  };
  const auto run_riccati = [&](const int it) {
    if (ric == 0) grid64(Bp, [&] { k_riccati(&K, &W, la, it); });
    else if (ric == 8) {
      if (PI) wave64("k_riccati8_pi", Bp / 8, [&] { k_riccati8_pi(K, Wpi, la, it, 1); });
      else wave64("k_riccati8", Bp / 8, [&] { k_riccati8(K, W, la, it, 1); });
    } else {  // one wavefront per listed instance; a launch of at most 16 instances repeats failed sweeps (sweeps_width of ltompc.hip)
      const int ms = n_launch <= 16 ? 4 : 1;
      if (ric1q) {  // four wavefronts per listed instance, dynamic LDS of exactly ric1q_lds_bytes(N)
        if (PI) wg("k_riccati1q_pi", n_launch, 256, ric1q_lds_bytes(N), LtWave::STACK, [&] { k_riccati1q_pi(K, Wpi, la, it, ms); });
        else wg("k_riccati1q", n_launch, 256, ric1q_lds_bytes(N), LtWave::STACK, [&] { k_riccati1q(K, W, la, it, ms); });
      } else if (PI) wave64_lds("k_riccati1_pi", n_launch, ric1_lds_bytes(N), [&] { k_riccati1_pi(K, Wpi, la, it, ms); });
      else wave64_lds("k_riccati1", n_launch, ric1_lds_bytes(N), [&] { k_riccati1(K, W, la, it, ms); });
    }
  };
  // the step selection: k_step1 with one workgroup of 320 lanes per listed instance, or the separate launches
  const auto run_step = [&] {
    if (step1) {
      if (PI) wg("k_step1_pi", n_launch, 320, 0, LtWave::STACK, [&] { ref ? k_step1_pi<BoundsRef>(&K, &Wpi, la) : k_step1_pi<BoundsAny>(&K, &Wpi, la); });
      else wg("k_step1", n_launch, 320, 0, LtWave::STACK, [&] { el ? (ref ? k_step1<BoundsRef, true>(&K, &W, la) : k_step1<BoundsAny, true>(&K, &W, la)) : (ref ? k_step1<BoundsRef, false>(&K, &W, la) : k_step1<BoundsAny, false>(&K, &W, la)); });
      return;
    }
    run_linesearch(0, Bp, N * Bp);
    run_pick(0, Bp);
    if (K.o.n_linesearch > 1 && W.ls_count[0] > 0) {
      const int jw = W.ls_count[0];
      run_linesearch(1, jw, (K.o.n_linesearch - 1) * N * jw);
      run_pick(1, jw);
    }
    grid64(N * Bp, [&] { k_update(&K, &W, la); });
  };
  const auto identity_list = [&] {
    for (int b = 0; b < Bp; b++) d_actl[0][b] = b;
    d_nactl[0][0] = B, set_list(0, B);
  };
  // k_compact on the flags `done` (SI_DONE in a solve, SI_FINAL in the rollout): the other list becomes the current one
  const auto compact_by_kernel = [&](const int* done, const int n_new) {
    scan1024("k_compact", [&] { k_compact(d_actl[cur], d_nactl[cur], done, d_actl[cur ^ 1], d_nactl[cur ^ 1]); });
    set_list(cur ^ 1, n_new);
  };
  std::vector<double> x(x0), u0((size_t)2 * B, 0.0), xn((size_t)8 * B);
  // k_plant_sens' planes (psn_prepare / psn_launch of deriv_passes.h): a work plane set, at the rows in effect
  double* psn = poisoned((size_t)PSN_NF * bp);
  const auto run_plant_sens = [&](const double* xs, const double* us, const int n_sub, const int with_theta) {
    const Consts Kc = K;  // (one wavefront = 8 instances x 8 lanes that exchange nothing: no collective, lane after lane)
    if (PI) grid64((B + 7) / 8 * 64, [&] { k_plant_sens_pi(Kc, d_th, B, Bp, xs, us, K.o.t_step, n_sub, with_theta, psn); });
    else grid64((B + 7) / 8 * 64, [&] { k_plant_sens(Kc, B, Bp, xs, us, K.o.t_step, n_sub, with_theta, psn); });
  };
  const auto planes_rows = [&](const double* planes, const int f0, const int F, double* out) {
    grid_bs((size_t)B * F, 256, [&] { k_planes_rows(planes, f0, F, B, Bp, out); });
  };
  if (plant_sens > 0) {
    // Plant-step mode: k_plant_sens (or _pi) and k_planes_rows at the states of the batch and the controls of section `u`, and
    // k_plant's own step; one line per instance: x_next[8] dx[64] du[16] dtheta[128].
    if (u_in.size() != (size_t)2 * B) return fprintf(stderr, "harness: plant_sens needs a section u\n"), 2;
    const Consts Kc = K;
    run_plant_sens(x.data(), u_in.data(), plant_sens, 1);
    double *rx = poisoned((size_t)64 * B), *ru = poisoned((size_t)16 * B), *rt = poisoned((size_t)8 * PS_NT * B);
    planes_rows(psn, PSN_DX, 64, rx), planes_rows(psn, PSN_DU, 16, ru), planes_rows(psn, PSN_DTH, 8 * PS_NT, rt);
    if (PI) grid64(B, [&] { k_plant_pi(Kc, d_th, Bp, B, x.data(), u_in.data(), K.o.t_step, plant_sens, xn.data()); });
    else grid64(B, [&] { k_plant(Kc, B, x.data(), u_in.data(), K.o.t_step, plant_sens, xn.data()); });
    printf("tick 0\n");
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < 8; i++) printf("%.17g ", xn[(size_t)8 * b + i]);
      for (int i = 0; i < 64; i++) printf("%.17g ", rx[(size_t)64 * b + i]);
      for (int i = 0; i < 16; i++) printf("%.17g ", ru[(size_t)16 * b + i]);
      for (int i = 0; i < 8 * PS_NT; i++) printf("%.17g ", rt[(size_t)8 * PS_NT * b + i]);
      printf("\n");
    }
    return 0;
  }
  // The derivative passes (sens_compute, sens_factorise, psens_prepare, psens_condense, psens_compute, adj_compute of deriv_passes.h):
  // Ws = W with the pass's own QP / RC / RS / LS (work planes) and a zeroed si; PV, KF, AJ work planes; outputs zeroed as the
  // library's; Wspi = Ws + TH (sync_pi_work).
  Work Ws = W;
  WorkPI Wspi;
  memset(&Wspi, 0, sizeof Wspi);
  int *sens_inertia = nullptr, *sens_ok = nullptr, *loop_ok = nullptr, *loop_ticks = nullptr;
  double *sens_du0 = nullptr, *sens_margin = nullptr, *sens_dX = nullptr, *sens_dU = nullptr, *uprev_rm = nullptr;
  double *PV = nullptr, *KF = nullptr, *ps_du0 = nullptr, *ps_dX = nullptr, *ps_dU = nullptr, *AJ = nullptr, *adj_gp = nullptr, *adj_gth = nullptr;
  double *d_cot = nullptr, *loop_Sx = nullptr, *loop_Du = nullptr;
  FILE* dump = nullptr;
  const size_t cot_sz = (size_t)B * ((n + 1) * 8 + n * 2);
  if (derivs) {
    if (el) return fprintf(stderr, "harness: derivs=1 without the friction ellipse (the passes over theta refuse it)\n"), 2;
    if (!dump_path || !(dump = fopen(dump_path, "wb"))) return fprintf(stderr, "harness: derivs=1 needs dump=<file>\n"), 2;
    Ws.QP = poisoned((size_t)QP_NF * (n + 1) * bp), Ws.RC = poisoned((size_t)RC_NF * (n + 1) * bp);
    Ws.RS = poisoned((size_t)RS_NF * n * bp), Ws.LS = poisoned((size_t)3 * n * bp);
    Ws.si = ipoisoned((size_t)SI_NF * bp, 0);  // zeros, never written
    sens_inertia = ipoisoned(bp, 0), sens_ok = ipoisoned(bp, 0);
    sens_du0 = zeros((size_t)2 * SENS_NP * B), sens_margin = zeros(B);
    sens_dX = zeros((n + 1) * 8 * SENS_NP * B), sens_dU = zeros(n * 2 * SENS_NP * B);
    uprev_rm = zeros((size_t)2 * B);
    PV = poisoned((size_t)PV_NF * n * bp), KF = poisoned(n * 2 * PS_NT * bp);
    ps_du0 = zeros((size_t)2 * PS_NT * B), ps_dX = zeros((n + 1) * 8 * PS_NT * B), ps_dU = zeros(n * 2 * PS_NT * B);
    AJ = poisoned((size_t)AJ_NF * n * bp), adj_gp = zeros((size_t)ADJ_NP * B), adj_gth = zeros((size_t)PS_NT * B);
    d_cot = (double*)malloc(sizeof(double) * (cot.size() ? cot.size() : 1));
    if (!cot.empty()) memcpy(d_cot, cot.data(), sizeof(double) * cot.size());
    if (PI) static_cast<Work&>(Wspi) = Ws, Wspi.TH = d_th;
    if (loop_mode) {
      if (loop_mode < 1 || loop_mode > 3) return fprintf(stderr, "harness: loop=1|2|3\n"), 2;
      loop_Sx = zeros((size_t)8 * LOOP_NQ * bp), loop_Du = zeros((size_t)2 * LOOP_NQ * bp), loop_ok = ipoisoned(bp, 0), loop_ticks = ipoisoned(bp, 0);
      grid_bs((size_t)LOOP_NQ * Bp, 256, [&] { k_loop_begin(B, Bp, loop_Sx, loop_Du, loop_ok, loop_ticks); });
    }
  }
  const auto put = [&](const double* v, const size_t cnt) { fwrite(v, sizeof(double), cnt, dump); };
  const auto put_planes = [&](const double* base, const int F, const int NK) {  // planes [F][NK][Bp] -> batch-major B x NK x F (planes_to_host)
    std::vector<double> o((size_t)B * NK * F);
    for (int b = 0; b < B; b++)
      for (int k = 0; k < NK; k++)
        for (int fi = 0; fi < F; fi++) o[((size_t)b * NK + k) * F + fi] = base[((size_t)fi * NK + k) * bp + b];
    put(o.data(), o.size());
  };
  const auto put_ints = [&](const int* v, const size_t cnt) {
    std::vector<double> o(cnt);
    for (size_t q = 0; q < cnt; q++) o[q] = v[q];
    put(o.data(), cnt);
  };
  // final=1: what the run leaves behind, per slot (= the caller's instance: the rollout never packs, pack=1 has un-packed):
  // status, iterations, x0[8], u_prev[2], the last node X_N[8], U_0[2], E0, orig, the state after the last plant step, and in
  // the last column the number of re-packings of the run
  const auto print_final = [&] {
    printf("tick final\n");
    for (int b = 0; b < B; b++) {
      printf("%d %d %d", b, W.si[(size_t)SI_STATUS * Bp + b], W.si[(size_t)SI_ITERS * Bp + b]);
      for (int i = 0; i < 8; i++) printf(" %.17g", W.x0[(size_t)i * Bp + b]);
      for (int i = 0; i < 2; i++) printf(" %.17g", W.uprev[(size_t)i * Bp + b]);
      for (int i = 0; i < 8; i++) printf(" %.17g", W.X[((size_t)i * (N + 1) + N) * Bp + b]);
      for (int i = 0; i < 2; i++) printf(" %.17g", W.U[((size_t)i * N + 0) * Bp + b]);
      printf(" %.17g %d", W.st[(size_t)ST_E0 * Bp + b], d_orig[b]);
      for (int i = 0; i < 8; i++) printf(" %.17g", x[(size_t)8 * b + i]);
      printf(" %d\n", n_packs);
    }
  };
  if (rollout > 0) {
    // ltompc_rollout_dev's loop on one stream, without events: k_roll_begin, then per pass k_roll_mark, k_roll_init, the iteration,
    // k_roll_finish, k_roll_plant on the pass's list (the library runs it on another stream, beside the next pass), and k_compact
    // on SI_FINAL by the library's rule.  The logs per tick in the columns of the synchronous run (instance, status, iterations, u0).
    if (eval8 || K.o.warm_shift || derivs) return fprintf(stderr, "harness: rollout with eval=slot, without warm_shift and derivs (as the library)\n"), 2;
    const int T = rollout;
    double* x_rm = (double*)malloc(sizeof(double) * 8 * B);  // exact size
    memcpy(x_rm, x.data(), sizeof(double) * 8 * B);
    double* u_log = poisoned((size_t)2 * T * B);
    int *st_log = ipoisoned((size_t)T * B, -1), *it_log = ipoisoned((size_t)T * B, -1), *cnt = ipoisoned(2, 0), *plist = ipoisoned(bp, -1);
    grid64(B, [&] { k_roll_begin(W, T); });
    grid64(B, [&] { k_zero_uprev(W); });
    W.ls_count[0] = W.ls_count[1] = 0;
    identity_list();
    const Consts Kc = K;
    const long long it_cap = (long long)T * ((long long)K.o.max_iter + 8) + 64;
    for (long long it = 0;; it++) {
      const int first = it == 0;
      cnt[0] = cnt[1] = 0;
      grid64(B, [&] { k_roll_mark(W, x_rm, K.o.resto_sticky, first); });
      if (PI) grid64(N * Bp, [&] { k_roll_init_pi(&K, &Wpi, la, first); });
      else grid64(N * Bp, [&] { k_roll_init(&K, &W, la, first); });
      la.force_eval = 0;
      run_eval(), run_riccati(-1), run_expand(), run_step();
      grid64(Bp, [&] { k_roll_finish(W, la, u_log, st_log, it_log, T, cnt, plist); });
      if (PI) grid64(n_launch, [&] { k_roll_plant_pi(Kc, Wpi, x_rm, K.o.t_step, 100, cnt + 1, plist); });
      else grid64(n_launch, [&] { k_roll_plant(Kc, W, x_rm, K.o.t_step, 100, cnt + 1, plist); });
      const int n_left = cnt[0];  // instances that still had ticks to do (counted before this pass's plant steps)
      if (n_left == 0) break;
      if (it >= it_cap) return fprintf(stderr, "harness: rollout iteration cap reached\n"), 1;
      if (n_left <= (pack_num * n_launch) / 8) compact_by_kernel(W.si + (size_t)SI_FINAL * Bp, n_left);
    }
    for (int t = 0; t < T; t++) {
      printf("tick %d\n", t);
      for (int b = 0; b < B; b++)
        printf("%d %d %d %.17g %.17g\n", b, st_log[(size_t)b * T + t], it_log[(size_t)b * T + t], u_log[((size_t)b * T + t) * 2], u_log[((size_t)b * T + t) * 2 + 1]);
    }
    memcpy(x.data(), x_rm, sizeof(double) * 8 * B);
    if (final_block) print_final();
    return 0;
  }
  for (int tick = 0; tick < ticks; tick++) {
    const int cold = tick == 0;
    grid64(B, [&] { k_load_x0(W, x.data(), packed ? d_orig : nullptr, K.o.resto_sticky, cold ? 0 : 1); });  // (the packed order is kept between ticks)
    if (cold) grid64(B, [&] { k_zero_uprev(W); });
    if (!cold && K.o.warm_shift) {
      grid64((N + 1) * Bp, [&] { k_shift(W, 0); });
      grid64((N + 1) * Bp, [&] { k_shift(W, 1); });
    }
    if (PI) grid64(N * Bp, [&] { k_init_pi(&K, &Wpi, cold); });
    else grid64(N * Bp, [&] { k_init(&K, &W, cold); });
    memset(W.active, 0, sizeof(int) * (K.o.max_iter + 2)), W.ls_count[0] = W.ls_count[1] = 0;
    identity_list();
    bool force_eval_next = false;
    for (int it = 0;; it++) {
      la.force_eval = force_eval_next ? 1 : 0, force_eval_next = false;
      run_eval();
      run_riccati(it);
      if (it >= K.o.max_iter) break;
      run_expand();
      run_step();
      int left = 0;
      for (int b = 0; b < B; b++) left += !W.si[(size_t)SI_DONE * Bp + b];
      if (!left) break;
      int* const done = W.si + (size_t)SI_DONE * Bp;
      if (pack) {  // the library's rule (ltompc_make_step_dev), with the width above which instances are moved as an argument
        if (left > (pack_num * n_launch) / 8) continue;
        if (n_launch > pack_min) {
          if (!packed) grid64(B, [&] { k_act_identity(d_orig, d_perm, B); });
          packed = true, n_packs++;
          scan1024("k_pack_perm", [&] { k_pack_perm(d_nactl[cur], done, d_perm, d_actl[cur ^ 1], d_nactl[cur ^ 1]); });
          for (int pass = 0; pass < 2; pass++)
            grid_bs((size_t)(N + 1) * n_launch, 256, [&] { k_pack(W, d_perm, d_nactl[cur], n_launch, d_orig, ni, (int)nel, pass); });
          force_eval_next = true;
          set_list(cur ^ 1, left);
        } else compact_by_kernel(done, left);
      } else if (compact_kernel) {
        compact_by_kernel(done, left);
      } else if (compact) {  // stable compaction of the unfinished instances of the current list; the rest of the list keeps -1
        int* const d_act = d_actl[cur];
        int n = 0;
        for (int j = 0; j < d_nactl[cur][0]; j++)
          if (!W.si[(size_t)SI_DONE * Bp + d_act[j]]) d_act[n++] = d_act[j];
        for (int j = n; j < Bp; j++) d_act[j] = -1;
        d_nactl[cur][0] = n, n_launch = n;
      }
    }
    if (derivs) grid64(B, [&] { k_psens_keep_uprev(W, uprev_rm, packed ? d_orig : nullptr); });  // (before k_store_u0 makes W.uprev its u0)
    grid64(B, [&] { k_store_u0(W, u0.data(), packed ? d_orig : nullptr); });
    if (pack && packed && tick == ticks - 1) {  // ensure_unpacked (ltompc.hip): slot j goes back to orig[j]
      grid64(B, [&] { k_pack_inverse(d_orig, d_perm, B); });
      for (int pass = 0; pass < 2; pass++)
        grid_bs((size_t)(N + 1) * B, 256, [&] { k_pack(W, d_perm, nullptr, B, d_orig, ni, (int)nel, pass); });
      packed = false;
    }
    printf("tick %d\n", tick);
    std::vector<int> slot_of(B);  // the slot of the caller's instance r (identity unless packed)
    for (int b = 0; b < B; b++) slot_of[d_orig[b]] = b;
    for (int r = 0, b = 0; r < B && (b = slot_of[r], true); r++)
      printf("%d %d %d %.17g %.17g %.17g %d %d %d %.17g %.17g\n", r, W.si[(size_t)SI_STATUS * Bp + b], W.si[(size_t)SI_ITERS * Bp + b], u0[2 * r], u0[2 * r + 1],
             W.st[(size_t)ST_E0 * Bp + b], W.si[(size_t)SI_NRESTO * Bp + b], W.si[(size_t)SI_NSHIFT * Bp + b], W.si[(size_t)SI_NFALLBACK * Bp + b],
             W.st[(size_t)ST_VIOL * Bp + b], W.st[(size_t)ST_G0 * Bp + b]);
    if (derivs) {
      // ---- sens_factorise: the evaluation kernel the solve used, at the final iterate, then the head-less sweep
      if (eval8) {
        if (PI) wave64("k_sens_eval8_pi", N * (Bp / 8), [&] { k_sens_eval8_pi(&K, &Wspi); });
        else wave64("k_sens_eval8", N * (Bp / 8), [&] { k_sens_eval8(&K, &Ws); });
      } else if (PI) grid64(N * Bp, [&] { ref ? k_sens_eval_pi<BoundsRef>(&K, &Wspi) : k_sens_eval_pi<BoundsAny>(&K, &Wspi); });
      else grid64(N * Bp, [&] { ref ? k_sens_eval<BoundsRef, false>(&K, &Ws) : k_sens_eval<BoundsAny, false>(&K, &Ws); });
      if (PI) wave64("k_sens_riccati8_pi", Bp / 8, [&] { k_sens_riccati8_pi(K, Wspi, W.si, sens_inertia); });
      else wave64("k_sens_riccati8", Bp / 8, [&] { k_sens_riccati8(K, Ws, W.si, sens_inertia); });
      // ---- sens_compute: both forward calls
      wave64("k_sens_forward", Bp / 8, [&] { k_sens_forward(Ws, sens_inertia, K.bd.ni, sens_du0, sens_ok, sens_margin, nullptr, nullptr, nullptr); });
      wave64("k_sens_forward", Bp / 8, [&] { k_sens_forward(Ws, sens_inertia, K.bd.ni, nullptr, nullptr, nullptr, sens_dX, sens_dU, sens_ok); });
      // ---- psens_condense + psens_compute with trajectories
      if (PI) grid64(N * Bp, [&] { ref ? k_psens_cond_pi<BoundsRef>(&K, &Wpi, PV) : k_psens_cond_pi<BoundsAny>(&K, &Wpi, PV); });
      else grid64(N * Bp, [&] { ref ? k_psens_cond<BoundsRef>(&K, &W, PV) : k_psens_cond<BoundsAny>(&K, &W, PV); });
      if (PI) wave64y("k_psens_sweep_pi", Bp / 8, 2, [&] { k_psens_sweep_pi(Wspi, uprev_rm, PV, sens_ok, KF, ps_du0, ps_dX, ps_dU); });
      else wave64y("k_psens_sweep", Bp / 8, 2, [&] { k_psens_sweep(Ws, K.p.r_du[0], K.p.r_du[1], uprev_rm, PV, sens_ok, KF, ps_du0, ps_dX, ps_dU); });
      // ---- the record of the tick: iterate, parameters, statuses, pass outputs
      put_planes(W.X, 8, N + 1), put_planes(W.C, 8, N), put_planes(W.U, 2, N), put_planes(W.L1, 8, N), put_planes(W.L2, 8, N);
      put_planes(W.T, ni, N), put_planes(W.NU, ni, N);
      put(x.data(), (size_t)8 * B), put(uprev_rm, (size_t)2 * B), put(u0.data(), (size_t)2 * B);
      {
        std::vector<double> s3((size_t)3 * B);
        for (int b = 0; b < B; b++) {
          const int node0 = W.si[(size_t)SI_NODE0 * Bp + b];
          s3[b] = W.si[(size_t)SI_STATUS * Bp + b], s3[B + b] = node0 ? node0 - 1 : W.si[(size_t)SI_STATUS * Bp + b], s3[2 * (size_t)B + b] = W.st[(size_t)ST_MU * Bp + b];
        }
        put(s3.data(), s3.size());  // status, the solver's status before the node-0 rule, mu
      }
      put(sens_du0, (size_t)2 * SENS_NP * B), put_ints(sens_ok, B), put(sens_margin, B);
      put(sens_dX, (n + 1) * 8 * SENS_NP * B), put(sens_dU, n * 2 * SENS_NP * B);
      put(ps_du0, (size_t)2 * PS_NT * B), put(ps_dX, (n + 1) * 8 * PS_NT * B), put(ps_dU, n * 2 * PS_NT * B);
      // ---- adj_compute with theta: one sweep per cotangent of the file
      for (int c = 0; c < n_cot; c++) {
        const double* gX = d_cot + (size_t)c * cot_sz;
        const double* gU = gX + (size_t)B * (n + 1) * 8;
        if (PI) wave64("k_adj_sweep_pi", Bp / 8, [&] { k_adj_sweep_pi(Wspi, uprev_rm, PV, sens_ok, gX, gU, AJ, adj_gp, adj_gth); });
        else wave64("k_adj_sweep", Bp / 8, [&] { k_adj_sweep(Ws, K.p.r_du[0], K.p.r_du[1], uprev_rm, PV, sens_ok, gX, gU, AJ, adj_gp, adj_gth); });
        put(adj_gp, (size_t)ADJ_NP * B), put(adj_gth, (size_t)PS_NT * B);
      }
      if (loop_mode) {  // ltompc_loop_tick_dev: the plant-step sensitivities at (x_t, u0_t), one tick of the accumulation
        run_plant_sens(x.data(), u0.data(), 100, (loop_mode & 2) != 0);
        grid_bs((size_t)LOOP_NQ * Bp, 256, [&] { k_loop_accum(B, Bp, loop_mode, sens_du0, (loop_mode & 1) ? ps_du0 : nullptr, sens_ok, psn, loop_Sx, loop_Du, loop_ok, loop_ticks); });
        double *rx = poisoned((size_t)64 * B), *ru = poisoned((size_t)16 * B), *rt = zeros((size_t)8 * PS_NT * B);
        planes_rows(psn, PSN_DX, 64, rx), planes_rows(psn, PSN_DU, 16, ru);
        if (loop_mode & 2) planes_rows(psn, PSN_DTH, 8 * PS_NT, rt);
        put(rx, (size_t)64 * B), put(ru, (size_t)16 * B), put(rt, (size_t)8 * PS_NT * B);
        free(rx), free(ru), free(rt);
        put_planes(loop_Sx, 8 * LOOP_NQ, 1), put_planes(loop_Du, 2 * LOOP_NQ, 1), put_ints(loop_ok, B), put_ints(loop_ticks, B);
      }
    }
    // plant step (k_plant) to the next tick's states
    Consts Kc = K;
    if (PI) grid64(B, [&] { k_plant_pi(Kc, d_th, Bp, B, x.data(), u0.data(), K.o.t_step, 100, xn.data()); });
    else grid64(B, [&] { k_plant(Kc, B, x.data(), u0.data(), K.o.t_step, 100, xn.data()); });
    x = xn;
  }
  if (final_block) print_final();
  if (dump) fclose(dump);
  return 0;
}
