// warm_state.h — per-instance control of the warm start: masked reset (ltompc_reset_instances), trajectory
// guesses (ltompc_set_guess) and export / import of the state an instance carries from solve to solve (ltompc_export_state,
// ltompc_import_state).
//
// One mechanism: a per-instance "starts cold" flag, an int per instance in the CALLER's instance order (indexed by orig[b], as BK
// and TH: re-packing moves instances between slots, not this array), in place of the handle-wide one.  While a flag may be set,
// the start of a solve runs the kernels of this file instead of k_load_x0 / k_init / k_roll_mark / k_roll_init: the same device
// functions (d_load_x0, d_init_slot, which take `cold` at run time) with each instance's own flag.  A handle on which none of the
// new calls was made launches exactly what it launched before; no existing kernel or device function is touched.
//
// What an instance carries from one solve to the next (d_load_x0, d_init_slot, k_shift, k_roll_mark, k_store_u0 / k_roll_finish):
// the planes X, C, U, L1, L2; u_prev; the si words STATUS, NODE0 (together the previous status), NRESTO and STARTEL ("jammed", for
// options.resto_sticky), STICKY; and the cold flag.  Everything else (slacks, inequality multipliers, the st plane, the filter,
// the backup planes, the other si words) is rebuilt by d_init_slot before it is read.  That list is the row of a blob:
//   [WS_HDR] magic | layout version | N   [WS_STATUS .. WS_COLD] the six ints as doubles   [WS_UPREV, +1]   [WS_RSV] 0
//   then X (N+1 x 8), C (N x 8), U (N x 2), L1 (N x 8), L2 (N x 8), each node-major as ltompc_get_iterate returns them.
#pragma once
#include "rollout.h"

namespace ltompc {

enum : int { WS_HDR = 0, WS_STATUS, WS_NODE0, WS_NRESTO, WS_STARTEL, WS_STICKY, WS_COLD, WS_UPREV, WS_RSV = WS_UPREV + 2, WS_META };
constexpr int WS_VERSION = 1;
constexpr int WS_TILE = 64;  // instances x blob columns of one workgroup of k_ws_copy

__host__ __device__ __forceinline__ int ws_size(const int N) { return WS_META + 8 + 34 * N; }  // X: 8 (N + 1), C, L1, L2: 8 N each, U: 2 N
// exactly representable: 'LT' << 32 | version << 16 | N  (N <= 4096)
__host__ __device__ __forceinline__ double ws_header(const int N) { return (double)((0x4C54ll << 32) | ((long long)WS_VERSION << 16) | N); }

// ------------------------------------------------------------------------------------------ start of a solve, per-instance flags
// k_load_x0 with update = !cold of each instance (W.orig is the identity while the instances are not packed)
__global__ void k_load_x0_m(Work W, const double* __restrict__ x0_rm, int sticky, const int* __restrict__ cold) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  const size_t r = W.orig[b];
  d_load_x0(W, x0_rm, b, r, sticky, cold[r] ? 0 : 1);
}
template <bool PI, bool TS = false>
__device__ __forceinline__ void d_init_m(const Consts& K, const Work& W, const int* __restrict__ cold) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B) return;
  d_init_slot<PI, TS>(K, W, k, b, cold[W.orig[b]] ? 1 : 0);
}
__global__ void k_init_m(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, const int* __restrict__ cold) { d_init_m<false>(*Kp, *Wp, cold); }
__global__ void k_init_m_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, const int* __restrict__ cold) { d_init_m<true>(*Kp, *Wp, cold); }
__global__ void k_init_m_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, const int* __restrict__ cold) { d_init_m<true, true>(*Kp, *Wp, cold); }

// the first pass of a rollout (it runs in the caller's order: slot b = instance b)
__global__ void k_roll_mark_m(Work W, const double* x_rm, int sticky, const int* __restrict__ cold) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  volatile int* ph = &W.si[(size_t)SI_PHASE * W.Bp + b];
  if (*ph != PH_READY) return;
  __threadfence();
  d_load_x0(W, x_rm, b, (size_t)b, sticky, cold[b] ? 0 : 1);
  *ph = PH_INIT;
}
template <bool PI, bool TS = false>
__device__ __forceinline__ void d_roll_init_m(const Consts& K, const Work& W, const Launch& la, const int* __restrict__ cold) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int j = tid % la.n_pad, k = tid / la.n_pad;
  if (k >= W.N || j >= la.nact[0]) return;
  const int b = la.act[j];
  if (W.si[(size_t)SI_PHASE * W.Bp + b] != PH_INIT) return;
  d_init_slot<PI, TS>(K, W, k, b, cold[W.orig[b]] ? 1 : 0);
}
__global__ void k_roll_init_m(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, Launch la, const int* __restrict__ cold) {
  d_roll_init_m<false>(*Kp, *Wp, la, cold);
}
__global__ void k_roll_init_m_pi(const Consts* __restrict__ Kp, const WorkPI* __restrict__ Wp, Launch la, const int* __restrict__ cold) {
  d_roll_init_m<true>(*Kp, *Wp, la, cold);
}
__global__ void k_roll_init_m_ts(const Consts* __restrict__ Kp, const WorkTS* __restrict__ Wp, Launch la, const int* __restrict__ cold) {
  d_roll_init_m<true, true>(*Kp, *Wp, la, cold);
}

// ------------------------------------------------------------------------------------------ masked reset
// mask, x0_rm: the caller's order.  One thread per instance: the new x0, u_prev := 0, the flag; then one per (interval, instance):
// the iterate as set_initial_guess fills it (d_init_slot, cold: it also clears the status words and the sticky counter).
__global__ void k_ws_reset_mark(Work W, const int* __restrict__ mask, const double* __restrict__ x0_rm, int* __restrict__ cold) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= W.B) return;
  const size_t r = W.orig[b];
  if (!mask[r]) return;
  d_load_x0(W, x0_rm, b, r, 0, 0);
  W.uprev[b] = 0.0, W.uprev[(size_t)W.Bp + b] = 0.0;
  cold[r] = 1;
}
__global__ void k_ws_reset_init(const Consts* __restrict__ Kp, const Work* __restrict__ Wp, const int* __restrict__ mask) {
  const Consts& K = *Kp;
  const Work& W = *Wp;
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int b = tid % W.Bp, k = tid / W.Bp;
  if (k >= W.N || b >= W.B || !mask[W.orig[b]]) return;
  d_init_slot(K, W, k, b, 1);  // (the uniform rows, as set_initial_guess: the next solve re-initialises the slot with its own)
}

// ------------------------------------------------------------------------------------------ trajectory guess
// The guess stands in for a previous solution that did not converge: planes := guess, L1 = L2 = 0, previous status MAX_ITER,
// node-0 flag and sticky counters cleared, not cold.  Xg (B, N+1, 8), Cg (B, N, 8), Ug (B, N, 2), ug (B, 2) or nullptr (= 0):
// the caller's order.  Thread = (node k, instance): reads whole 64-byte rows, writes coalesced planes.
__global__ void __launch_bounds__(256) k_ws_guess(Work W, const int* __restrict__ mask, const double* __restrict__ Xg, const double* __restrict__ Cg,
                                                  const double* __restrict__ Ug, const double* __restrict__ ug, int* __restrict__ cold) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)(tid % W.Bp), k = (int)(tid / W.Bp), N = W.N;
  if (k > N || b >= W.B) return;
  const size_t r = W.orig[b];
  if (!mask[r]) return;
#pragma unroll
  for (int i = 0; i < 8; i++) PL(W.X, i, k, N + 1) = Xg[(r * (N + 1) + k) * 8 + i];
  if (k < N) {
#pragma unroll
    for (int i = 0; i < 8; i++) PL(W.C, i, k, N) = Cg[(r * N + k) * 8 + i], PL(W.L1, i, k, N) = 0.0, PL(W.L2, i, k, N) = 0.0;
    PL(W.U, 0, k, N) = Ug[(r * N + k) * 2], PL(W.U, 1, k, N) = Ug[(r * N + k) * 2 + 1];
  }
  if (k == 0) {
    int* si = W.si;
    STI(SI_STATUS) = LTOMPC_STATUS_MAX_ITER, STI(SI_NODE0) = 0, STI(SI_NRESTO) = 0, STI(SI_STARTEL) = 0, STI(SI_STICKY) = 0;
    W.uprev[b] = ug ? ug[r * 2] : 0.0, W.uprev[(size_t)W.Bp + b] = ug ? ug[r * 2 + 1] : 0.0;
    cold[r] = 0;
  }
}

// ------------------------------------------------------------------------------------------ export / import
// Word c of the row of the instance in slot `slot` (caller's index `inst`).
struct WsPlane {
  gptr<double> p;
  size_t at;  // offset of slot 0
};
__device__ __forceinline__ WsPlane ws_plane(const Work& W, int q) {  // q: column - WS_META
  const int N = W.N;
  gptr<double> base = W.X;
  int NK = N + 1, F = 8;
  if (q >= 8 * (N + 1)) {
    q -= 8 * (N + 1), NK = N;
    if (q < 8 * N) base = W.C;
    else if ((q -= 8 * N) < 2 * N) base = W.U, F = 2;
    else if ((q -= 2 * N) < 8 * N) base = W.L1;
    else q -= 8 * N, base = W.L2;
  }
  const int k = q / F, f = q % F;
  return WsPlane{base, ((size_t)f * NK + k) * W.Bp};
}
__device__ __forceinline__ int ws_si_field(const int c) {
  return c == WS_STATUS ? SI_STATUS : c == WS_NODE0 ? SI_NODE0 : c == WS_NRESTO ? SI_NRESTO : c == WS_STARTEL ? SI_STARTEL : SI_STICKY;
}
__device__ __forceinline__ double ws_get(const Work& W, const int c, const int slot, const int inst, const int* __restrict__ cold, const int cold_all) {
  if (c >= WS_META) {
    const WsPlane pl = ws_plane(W, c - WS_META);
    return pl.p[pl.at + slot];
  }
  if (c == WS_HDR) return ws_header(W.N);
  if (c >= WS_STATUS && c <= WS_STICKY) return (double)W.si[(size_t)ws_si_field(c) * W.Bp + slot];
  if (c == WS_COLD) return (cold_all || (cold && cold[inst])) ? 1.0 : 0.0;
  if (c == WS_UPREV || c == WS_UPREV + 1) return W.uprev[(size_t)(c - WS_UPREV) * W.Bp + slot];
  return 0.0;
}
__device__ __forceinline__ void ws_put(const Work& W, const int c, const int slot, const int inst, int* __restrict__ cold, const double v) {
  if (c >= WS_META) {
    const WsPlane pl = ws_plane(W, c - WS_META);
    pl.p[pl.at + slot] = v;
  } else if (c >= WS_STATUS && c <= WS_STICKY) W.si[(size_t)ws_si_field(c) * W.Bp + slot] = (int)v;
  else if (c == WS_COLD) cold[inst] = v != 0.0 ? 1 : 0;
  else if (c == WS_UPREV || c == WS_UPREV + 1) W.uprev[(size_t)(c - WS_UPREV) * W.Bp + slot] = v;
}
// The planes are [field][k][Bp], instance fastest; a blob is instance-major.  A thread per (instance, word) in either order
// touches 8 useful bytes per 64-byte sector on one side.  So a workgroup moves a tile of WS_TILE instances x WS_TILE words through
// LDS: on the plane side a wavefront takes one word (wave-uniform: its plane address is scalar arithmetic) of 64 instances, 512
// contiguous bytes when their slots are (idx ascending, handle not packed); on the blob side one instance's 64 consecutive
// words, 512 contiguous bytes always.  The tile's row pitch of WS_TILE + 1 doubles keeps the transposed LDS access free of bank
// conflicts beyond the two passes a 64-bit access takes anyway.  No atomics: every word has one writer.
// blob row j = instance idx[j] (nullptr: j); inv: caller's index -> slot (nullptr: the identity, handle not packed).
// Workgroup (jb, cb) = blockIdx.x: cb fastest.
template <bool IMPORT>
__device__ __forceinline__ void d_ws_copy(const Work& W, const int* __restrict__ idx, const int* __restrict__ inv, const int n,
                                          double* __restrict__ blob, int* __restrict__ cold, const int cold_all) {
  __shared__ double tile[WS_TILE][WS_TILE + 1];
  const int S = ws_size(W.N), ncb = (S + WS_TILE - 1) / WS_TILE;
  const int j0 = (int)(blockIdx.x / ncb) * WS_TILE, c0 = (int)(blockIdx.x % ncb) * WS_TILE;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  // plane side: the lane's instance
  const int jl = j0 + lane;
  int inst = -1, slot = -1;
  if (jl < n) inst = idx ? idx[jl] : jl, slot = inv ? inv[inst] : inst;
  if (IMPORT) {
    for (int r = wv; r < WS_TILE; r += nwv) {
      const int j = j0 + r, c = c0 + lane;
      if (j < n && c < S) tile[lane][r] = blob[(size_t)j * S + c];
    }
    __syncthreads();
    for (int r = wv; r < WS_TILE; r += nwv) {
      const int c = c0 + r;
      if (c < S && slot >= 0) ws_put(W, c, slot, inst, cold, tile[r][lane]);
    }
  } else {
    for (int r = wv; r < WS_TILE; r += nwv) {
      const int c = c0 + r;
      if (c < S && slot >= 0) tile[r][lane] = ws_get(W, c, slot, inst, cold, cold_all);
    }
    __syncthreads();
    for (int r = wv; r < WS_TILE; r += nwv) {
      const int j = j0 + r, c = c0 + lane;
      if (j < n && c < S) blob[(size_t)j * S + c] = tile[lane][r];
    }
  }
}
__global__ void __launch_bounds__(256) k_ws_export(Work W, const int* __restrict__ idx, const int* __restrict__ inv, int n, double* __restrict__ blob,
                                                   const int* __restrict__ cold, int cold_all) {
  d_ws_copy<false>(W, idx, inv, n, blob, const_cast<int*>(cold), cold_all);
}
__global__ void __launch_bounds__(256) k_ws_import(Work W, const int* __restrict__ idx, const int* __restrict__ inv, int n, const double* __restrict__ blob,
                                                   int* __restrict__ cold) {
  d_ws_copy<true>(W, idx, inv, n, const_cast<double*>(blob), cold, 0);
}

}  // namespace ltompc
