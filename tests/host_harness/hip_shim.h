// hip_shim.h — TEST INFRASTRUCTURE (tests/host_harness): just enough of the HIP device vocabulary for the solver's device
// functions and kernels to compile as plain host C++ (g++), so that they can run under AddressSanitizer /
// UndefinedBehaviorSanitizer on the CPU (the pool's GPUs run no sanitizer).  Not a product path: nothing in the package
// includes this file.
//
// What runs on it (harness.cpp):
//   - the thread-per-slot kernels, one lane after the other (no collectives: k_init, k_eval, k_expand, k_linesearch, k_update,
//     k_plant, k_test_model, k_sens_eval, k_psens_cond, k_plant_sens, ...);
//   - the one-wavefront kernels on the lock-step wavefront below (k_riccati8, k_riccati1, k_eval8, k_expand8, k_pick,
//     k_sens_eval8, k_sens_riccati8, k_sens_forward, k_psens_sweep, k_adj_sweep and their _pi forms).
//   - the kernels whose workgroup has several wavefronts on the lock-step workgroup (LtWave::run): k_riccati1q (4 wavefronts,
//     WG_SYNC_LDS), k_step1 (5, __syncthreads), k_compact / k_pack_perm (16, a scan in LDS), and their _pi forms.  Its wavefronts
//     run one after the other between two workgroup barriers, in ascending or in descending order (LtWave::desc_waves); the tests
//     make every such run in both orders and compare the results bit for bit, which is how a missing barrier shows.
// What it cannot model: several lanes adding to ONE LDS word in the same instruction (below); the ordering of global memory
// BETWEEN workgroups (the blocks of a launch run one after the other, each to its end); concurrent streams.
//
// The lock-step wavefront: 64 lanes as 64 cooperative fibers on one OS thread.  A lane runs until it reaches a collective
// (__shfl, __shfl_xor, __any, WAVE_SYNC, grp_*) or returns; when every lane has stopped, the scheduler checks that all lanes of
// the collective stand at the SAME call site, exchanges the values and lets them go on.  Anything else ends the run with a
// message that names the sites (exit status 3): a collective that only some lanes reach while others have returned or wait at
// another site is either a bug in the kernel or, if the hardware allows it, something this file has to model.
//   - __shfl / __shfl_xor / __any / WAVE_SYNC are wave-level: all 64 lanes.
//   - grp_sum / grp_min / grp_max involve the eight lanes (g, i = 0..7), lane = g + 8 i, that share g = lane & 7: xor-shuffles
//     over the lane strides 8, 16, 32 in that order, the floating-point order of layout.h.  They are modelled as GROUP-level
//     collectives: the hardware executes a shuffle under the EXEC mask, and a lane group that is alone in a branch (k_pick:
//     `if (!live) return` per instance, the line search's per-instance candidate loop) reads only lanes of its own group, all of
//     them active.
//   - WAVE_SYNC is wave-level while the wave agrees and falls back to the instance groups in diverged control flow (see advance()).
// Between two collectives the lanes run one after the other in DESCENDING order, so a lane with i = 0 (lanes 0..7), the lane
// that writes an instance's scalars in the kernels, runs after the lanes that have read them "in the same instruction" on the
// device.  The order is fixed: every run of the harness takes the same path.  What this cannot model is several lanes adding to
// ONE LDS word in the same instruction (on the device each reads the old value and stores the same new one): lin8 (eval8.h)
// does that through the model functions and has a harness branch for it.
//
// The lock-step workgroup: W wavefronts of 64 lanes, threadIdx.x = 0 .. 64 W - 1, all fibers of the one OS thread.  The
// collectives above act within each wavefront.  __syncthreads() and WG_SYNC_LDS() (riccati.h) are workgroup collectives: a
// barrier completes when every lane of the workgroup has returned from the kernel or stands at the same barrier site; lanes at
// different barrier sites, or lanes at a barrier while others wait at a wave-level collective that cannot complete, end the run
// with the same report.  Between two barriers each wavefront runs as far as it can before the next one starts, in ascending or
// in descending wavefront order (see run()).
//
// __shared__ is `static`: one object per program, which is one object per workgroup while the blocks of a launch run one after
// the other (they do).  The dynamic LDS of k_riccati1 / k_riccati1q is lt_dyn_lds, set by the harness per block (exact size,
// NaN-filled).
#pragma once
// The harness branches of csrc/ that need the lock-step wavefront (WAVE_SYNC as a collective, lt_dyn_lds, lin8's private copies)
// ask for this; with a shim that does not define it they compile as inert placeholders, as before there was a wavefront.
#define LTOMPC_HARNESS_WAVEFRONT 1
// ... and those that need workgroups of several wavefronts (WG_SYNC_LDS as a workgroup barrier, k_riccati1q's dynamic LDS) for this
#define LTOMPC_HARNESS_WORKGROUP 1
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)

struct dim3 {
  unsigned x = 1, y = 1, z = 1;
};
inline dim3 threadIdx, blockIdx, blockDim, gridDim;  // (one OS thread: the scheduler sets threadIdx when it resumes a lane)

template <class T, class V>
inline T atomicAdd(T* p, V v) { return __atomic_fetch_add(p, (T)v, __ATOMIC_RELAXED); }
inline long long clock64() { return 0; }
inline int min(int a, int b) { return a < b ? a : b; }
inline void __threadfence() {}
#define __builtin_amdgcn_fence(a, b) ((void)0)
#define __builtin_amdgcn_wave_barrier() ((void)0)
#define __builtin_amdgcn_sched_barrier(x) ((void)0)

inline void* lt_dyn_lds = nullptr;  // `extern __shared__` of the block that runs

#if defined(__SANITIZE_ADDRESS__)
extern "C" void __sanitizer_start_switch_fiber(void** fake_stack_save, const void* bottom, size_t size);
extern "C" void __sanitizer_finish_switch_fiber(void* fake_stack_save, const void** bottom_old, size_t* size_old);
#define LT_FIBER_START(save, bottom, size) __sanitizer_start_switch_fiber(save, bottom, size)
#define LT_FIBER_FINISH(save, bottom, size) __sanitizer_finish_switch_fiber(save, bottom, size)
#else
#define LT_FIBER_START(save, bottom, size) ((void)0)
#define LT_FIBER_FINISH(save, bottom, size) ((void)0)
#endif

// The switch between two stacks.  Not swapcontext(): it enters the kernel twice per call for the signal mask, and under ASan
// its interceptor clears the shadow of the whole target stack every time; a solve makes millions of switches.  The callee-saved
// registers of the System V x86-64 ABI are pushed on the old stack and popped from the new one.
#if !defined(__x86_64__)
#error "the host harness's lock-step wavefront switches stacks with x86-64 code"
#endif
extern "C" void lt_switch(void** save_sp, void* load_sp);
asm(R"(
  .text
  .p2align 4
  .globl lt_switch
  .type lt_switch, @function
lt_switch:
  pushq %rbp
  pushq %rbx
  pushq %r12
  pushq %r13
  pushq %r14
  pushq %r15
  movq %rsp, (%rdi)
  movq %rsi, %rsp
  popq %r15
  popq %r14
  popq %r13
  popq %r12
  popq %rbx
  popq %rbp
  ret
  .size lt_switch, .-lt_switch
  .section .note.GNU-stack,"",@progbits
  .text
)");

struct LtWave {
  enum { READY = 0, AT_WAVE, AT_GROUP, AT_BARRIER, DONE };
  static constexpr int NL = 64;     // lanes of a wavefront
  static constexpr int MAXW = 16;   // wavefronts of a workgroup (1024 threads)
  static constexpr int MAXL = NL * MAXW;
  // Stacks: allocated when a lane first runs, at the size the launch asks for.  1 MiB for the solver's kernels (model derivatives
  // with their sanitizer frames); the 1024-lane scan kernels (k_compact, k_pack_perm: a handful of ints per lane) ask for
  // STACK_SMALL, so that their 1024 fibers take 64 MiB of address space instead of 1 GiB.  A word at the low end of every stack is
  // checked whenever its lane stops: a lane that needs more ends the run instead of writing into its neighbour.
  static constexpr size_t STACK = (size_t)1 << 20, STACK_SMALL = (size_t)64 << 10;
  static constexpr uint64_t CANARY = 0x5AFE57ACC0FFEE11ull;
  struct Lane {
    void* sp = nullptr;
    char* stack = nullptr;
    size_t stack_size = 0;
    void* fake = nullptr;
    int state = DONE;
    const char *what = "", *file = "";
    int line = 0;
    uint64_t put = 0;
  };
  Lane lane[MAXL];
  uint64_t got[MAXL];  // the values of the collective a lane has just been released from
  void* sched_sp = nullptr;
  const void* sched_bottom = nullptr;
  size_t sched_size = 0;
  int cur = -1;
  int nw = 1;               // wavefronts of the workgroup that runs
  bool desc_waves = false;  // wave_order=desc: between two barriers the wavefronts run from the last to the first
  void (*body)(void*) = nullptr;
  void* arg = nullptr;
  const char* kernel = "";

  static LtWave& self() {
    static LtWave w;
    return w;
  }
  static void entry() {
    LtWave& w = self();
    LT_FIBER_FINISH(nullptr, &w.sched_bottom, &w.sched_size);
    w.body(w.arg);
    Lane& l = w.lane[w.cur];
    l.state = DONE;
    LT_FIBER_START(nullptr, w.sched_bottom, w.sched_size);  // (this fiber does not come back)
    lt_switch(&l.sp, w.sched_sp);
    abort();
  }
  bool same_place(const int a, const int c) const { return lane[c].state == lane[a].state && lane[c].line == lane[a].line && !strcmp(lane[c].file, lane[a].file); }
  [[noreturn]] void report(const char* why) {
    const int n = nw * NL;
    fprintf(stderr, "lock-step wavefront: MISMATCHED COLLECTIVE in %s, block %u: %s\n", kernel, blockIdx.x, why);
    for (int a = 0; a < n; a++) {  // lanes grouped by where they stand (lane = threadIdx.x; wavefront = lane / 64)
      bool first = true;
      for (int c = 0; c < a && first; c++)
        if (same_place(a, c)) first = false;
      if (!first) continue;
      if (lane[a].state == DONE) fprintf(stderr, "  returned from the kernel: lanes");
      else if (lane[a].state == READY) fprintf(stderr, "  running: lanes");
      else fprintf(stderr, "  at %s, %s:%d: lanes", lane[a].what, lane[a].file, lane[a].line);
      for (int c = a; c < n; c++) {  // as ranges: a workgroup has up to 1024 lanes
        if (!same_place(a, c)) continue;
        int e = c;
        while (e + 1 < n && same_place(a, e + 1)) e++;
        if (e > c + 1) fprintf(stderr, " %d-%d", c, e);
        else if (e > c) fprintf(stderr, " %d %d", c, e);
        else fprintf(stderr, " %d", c);
        c = e;
      }
      fprintf(stderr, "\n");
    }
    fflush(stderr);
    _exit(3);
  }
  bool same_site(const int a, const int b) const { return lane[a].line == lane[b].line && !strcmp(lane[a].file, lane[b].file) && !strcmp(lane[a].what, lane[b].what); }
  // One wavefront (lanes base .. base + 63): its ready lanes run, in descending order, until each stops at a collective or returns;
  // then the wave-level or group-level collectives of the wavefront that can complete do.  False when nothing moved.
  bool advance(const int base) {
    bool moved = false;
    for (int l = base + NL - 1; l >= base; l--) {
      if (lane[l].state != READY) continue;
      cur = l, threadIdx.x = l;
      void* fake = nullptr;
      LT_FIBER_START(&fake, lane[l].stack, lane[l].stack_size);
      lt_switch(&sched_sp, lane[l].sp);
      LT_FIBER_FINISH(fake, nullptr, nullptr);
      uint64_t canary;
      memcpy(&canary, lane[l].stack, sizeof canary);
      if (canary != CANARY) fprintf(stderr, "lock-step wavefront: lane %d of %s has run over its stack of %zu bytes\n", l, kernel, lane[l].stack_size), _exit(3);
      moved = true;
    }
    cur = -1;
    int n_wave = 0, n_group = 0;
    for (int l = base; l < base + NL; l++) n_wave += lane[l].state == AT_WAVE, n_group += lane[l].state == AT_GROUP;
    bool progress = false;
    bool wave_agrees = n_wave == NL;
    for (int l = base + 1; l < base + NL && wave_agrees; l++) wave_agrees = same_site(base, l);
    if (wave_agrees) {
      for (int l = base; l < base + NL; l++) got[l] = lane[l].put, lane[l].state = READY;
      progress = true;
    } else if (n_group) {
      for (int g = base; g < base + 8; g++) {
        int n = 0;
        for (int i = 0; i < 8; i++) n += lane[g + 8 * i].state == AT_GROUP;
        if (n < 8) continue;
        for (int i = 1; i < 8; i++)
          if (!same_site(g, g + 8 * i)) report("the lanes of an instance group stand at different grp_* collectives");
        for (int i = 0; i < 8; i++) got[g + 8 * i] = lane[g + 8 * i].put, lane[g + 8 * i].state = READY;
        progress = true;
      }
    }
    if (!progress && n_wave) {
      // WAVE_SYNC in diverged control flow.  Unlike a shuffle or a vote it is legal there: on the device it is two fences and
      // a scheduling barrier, no instruction that waits for other lanes.  d_eval8 has one inside `if (reinit)`, a branch that
      // the lane groups of some instances take and others do not (it orders lane 0's stores of the re-initialised slot before
      // the loads of the slot's other lanes), and k_eval8's groups exchange through their own LDS slot only.  So when the wave
      // cannot agree, a WAVE_SYNC completes for every instance group whose eight lanes stand at the same site, like a grp_*;
      // the groups then run one collective apart and a group may return while another still works.  Shuffles and votes stay
      // strict, and so does a group whose own lanes disagree or have partly returned.
      for (int g = base; g < base + 8; g++) {
        bool all = true;
        for (int i = 0; i < 8 && all; i++) all = lane[g + 8 * i].state == AT_WAVE && !strcmp(lane[g + 8 * i].what, "WAVE_SYNC") && same_site(g, g + 8 * i);
        if (!all) continue;
        for (int i = 0; i < 8; i++) got[g + 8 * i] = 0, lane[g + 8 * i].state = READY;
        progress = true;
      }
    }
    return moved || progress;
  }
  // One workgroup of n_waves wavefronts (threadIdx.x = 0 .. 64 n_waves - 1).  Every wavefront runs as far as it can, through its
  // own wave-level and group-level collectives, until each of its lanes has returned or waits at a workgroup barrier
  // (__syncthreads, WG_SYNC_LDS); the wavefronts do so ONE AFTER THE OTHER, in ascending order or (desc_waves) in descending
  // order.  A barrier completes when every lane of the workgroup has returned or stands at the same barrier site.  What a
  // wavefront writes before a barrier, another reads after it in both orders; without the barrier one order reads the old word
  // and the other the new one, so a run whose printed values differ between the two orders has a missing barrier (which no
  // sanitizer sees).  Within a wavefront the order stays what it was, descending lanes (see the top of the file): the lanes of
  // a wavefront execute an instruction together, so their order stands for nothing the hardware could do differently.
  void run(const char* name, const int n_waves, const size_t stack_bytes, void (*fn)(void*), void* a) {
    if (cur >= 0) fprintf(stderr, "lock-step wavefront: launch from inside a kernel\n"), _exit(3);
    if (n_waves < 1 || n_waves > MAXW) fprintf(stderr, "lock-step wavefront: a workgroup of %d wavefronts\n", n_waves), _exit(3);
    kernel = name, body = fn, arg = a, nw = n_waves;
    const int n = nw * NL;
    for (int l = 0; l < n; l++) {
      Lane& L = lane[l];
      if (L.stack_size < stack_bytes) free(L.stack), L.stack = (char*)malloc(stack_bytes), L.stack_size = stack_bytes;
      memcpy(L.stack, &CANARY, sizeof CANARY);
      // a fresh stack: six zeroed callee-saved registers, then entry() as the return address of lt_switch, then entry()'s own (null)
      void** top = (void**)(((uintptr_t)L.stack + L.stack_size) & ~(uintptr_t)15);
      top[-1] = nullptr, top[-2] = (void*)&entry;
      for (int q = 3; q <= 8; q++) top[-q] = nullptr;
      L.sp = top - 8;
      L.state = READY, L.what = L.file = "", L.line = 0, L.fake = nullptr;
    }
    for (;;) {
      for (int q = 0; q < nw; q++) {
        const int base = (desc_waves ? nw - 1 - q : q) * NL;
        while (advance(base)) {}
      }
      int n_done = 0, n_bar = 0, first = -1;
      for (int l = 0; l < n; l++) {
        n_done += lane[l].state == DONE;
        if (lane[l].state == AT_BARRIER) n_bar++, first = first < 0 ? l : first;
      }
      if (n_done == n) break;
      if (n_done + n_bar < n) {  // a wavefront is stuck at a wave-level or group-level collective
        for (int w = 0; w < nw; w++) {
          int s_wave = 0, s_done = 0, s_bar = 0;
          for (int l = w * NL; l < (w + 1) * NL; l++) s_wave += lane[l].state == AT_WAVE, s_done += lane[l].state == DONE, s_bar += lane[l].state == AT_BARRIER;
          if (s_done + s_bar == NL) continue;
          if (s_wave == NL) report("the lanes stand at different wave-level collectives");
          if (s_bar || n_bar) report("some lanes wait at a workgroup barrier while others wait at a wave-level collective that cannot complete");
          report(s_done ? "some lanes wait at a collective that the others, having returned or waiting elsewhere, never reach"
                        : "the lanes wait at collectives that cannot complete together");
        }
      }
      for (int l = first; l < n; l++)
        if (lane[l].state == AT_BARRIER && !same_site(first, l)) report("the lanes of the workgroup stand at different barriers");
      for (int l = first; l < n; l++)
        if (lane[l].state == AT_BARRIER) got[l] = 0, lane[l].state = READY;
    }
  }
  void run(const char* name, void (*fn)(void*), void* a) { run(name, 1, STACK, fn, a); }  // one workgroup of one wavefront
  // called by a lane: stop at a collective, come back with got[] filled
  void collective(const int level, const char* what, const char* file, const int line, const uint64_t v) {
    if (cur < 0) fprintf(stderr, "lock-step wavefront: %s at %s:%d outside a wavefront launch\n", what, file, line), _exit(3);
    Lane& L = lane[cur];
    L.state = level, L.what = what, L.file = file, L.line = line, L.put = v;
    LT_FIBER_START(&L.fake, sched_bottom, sched_size);
    lt_switch(&L.sp, sched_sp);
    LT_FIBER_FINISH(L.fake, nullptr, nullptr);
  }
};

template <class T> inline uint64_t lt_bits(const T v) {
  static_assert(sizeof(T) <= 8, "collectives exchange up to 64 bits");
  uint64_t u = 0;
  memcpy(&u, &v, sizeof(T));
  return u;
}
template <class T> inline T lt_unbits(const uint64_t u) {
  T v;
  memcpy(&v, &u, sizeof(T));
  return v;
}
template <class T> inline T lt_shfl(const T v, const int src, const char* file, const int line) {
  LtWave& w = LtWave::self();
  w.collective(LtWave::AT_WAVE, "__shfl", file, line, lt_bits(v));
  if (src < 0 || src >= LtWave::NL) fprintf(stderr, "lock-step wavefront: __shfl from lane %d at %s:%d\n", src, file, line), _exit(3);
  return lt_unbits<T>(w.got[(w.cur & ~(LtWave::NL - 1)) + src]);
}
template <class T> inline T lt_shfl_xor(const T v, const int mask, const char* file, const int line) {
  LtWave& w = LtWave::self();
  w.collective(LtWave::AT_WAVE, "__shfl_xor", file, line, lt_bits(v));
  if (mask < 0 || mask >= LtWave::NL) fprintf(stderr, "lock-step wavefront: __shfl_xor with mask %d at %s:%d\n", mask, file, line), _exit(3);
  return lt_unbits<T>(w.got[w.cur ^ mask]);
}
inline int lt_any(const int p, const char* file, const int line) {
  LtWave& w = LtWave::self();
  w.collective(LtWave::AT_WAVE, "__any", file, line, p ? 1 : 0);
  int r = 0;
  for (int l = 0; l < LtWave::NL; l++) r |= w.got[(w.cur & ~(LtWave::NL - 1)) + l] != 0;
  return r;
}
inline void lt_wave_sync(const char* file, const int line) { LtWave::self().collective(LtWave::AT_WAVE, "WAVE_SYNC", file, line, 0); }
// workgroup barriers: __syncthreads() and WG_SYNC_LDS() (riccati.h)
inline void lt_barrier(const char* what, const char* file, const int line) { LtWave::self().collective(LtWave::AT_BARRIER, what, file, line, 0); }
// one xor-shuffle among the eight lanes that share g = lane & 7 (x = 8, 16, 32)
inline double lt_grp_xchg(const double v, const int x, const char* what, const char* file, const int line) {
  LtWave& w = LtWave::self();
  w.collective(LtWave::AT_GROUP, what, file, line, lt_bits(v));
  return lt_unbits<double>(w.got[w.cur ^ x]);
}
#define LT_X(v, x) lt_grp_xchg(v, x, what, file, line)
inline double lt_grp_max(double v, const char* file, const int line) {
  const char* what = "grp_max";
  v = fmax(v, LT_X(v, 8)), v = fmax(v, LT_X(v, 16)), v = fmax(v, LT_X(v, 32));
  return v;
}
inline double lt_grp_sum(double v, const char* file, const int line) {
  const char* what = "grp_sum";
  v += LT_X(v, 8), v += LT_X(v, 16), v += LT_X(v, 32);
  return v;
}
inline double lt_grp_min(double v, const char* file, const int line) {
  const char* what = "grp_min";
  v = fmin(v, LT_X(v, 8)), v = fmin(v, LT_X(v, 16)), v = fmin(v, LT_X(v, 32));
  return v;
}
#undef LT_X
#define __syncthreads() lt_barrier("__syncthreads", __FILE__, __LINE__)
#define __shfl(v, src) lt_shfl((v), (src), __FILE__, __LINE__)
#define __shfl_xor(v, mask) lt_shfl_xor((v), (mask), __FILE__, __LINE__)
#define __any(p) lt_any((p), __FILE__, __LINE__)
#define grp_max(v) lt_grp_max((v), __FILE__, __LINE__)
#define grp_sum(v) lt_grp_sum((v), __FILE__, __LINE__)
#define grp_min(v) lt_grp_min((v), __FILE__, __LINE__)
