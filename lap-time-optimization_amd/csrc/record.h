// record.h — solve records: k_rec_save copies everything the derivative passes read from the live handle into the
// buffers of a record, so that the passes can run on that solve after the handle has gone on (ltompc_record_save / _select).
//
// A record has the planes' own layout, [field][k][Bp], with its instances in the CALLER's order (identity `orig`): it does not
// depend on any later re-packing.  What it carries, from the kernels that the passes launch:
//   d_eval / d_eval8 (sens form)   X, C, U, L1, L2, T (slacks, elastic and ellipse planes), NU; st; x0; uprev; si (a zeroed set: Ws.si)
//   d_sens_riccati8                the stage blocks of the pass; of the solver's si the words STATUS, NODE0 and REINIT; U, uprev
//   k_sens_forward                 T, NU (margin), orig
//   k_psens_cond, k_tab_cond       the iterate planes, st (EPS, RHO, MU), uprev, orig, TH, the table value rows (through Consts)
//   k_psens_sweep, k_adj_sweep, k_adj_sweep_tab, k_jvp_sweep   X, U, uprev, orig, TH and d_psens_uprev (caller's order already)
//   k_tab_scatter                  X, st (EPS), orig, the grids (the handle's, immutable)
// The pad lanes [B, Bp) of every plane are copied slot for slot, so that a wavefront that touches them sees what it saw live.
#pragma once
#include "layout.h"

namespace ltompc {

constexpr int REC_MAX_PLANES = 16;
enum : int { REC_W32 = 1, REC_DIRECT = 2 };  // rows of 4-byte words (si); rows already in the caller's order (no gather)

// One plane set: `rows` rows of Bp words at src, to dst.
struct RecPlane {
  gptr<const void> src;
  gptr<void> dst;
  int rows, flags;
};
struct RecPlanes {
  RecPlane p[REC_MAX_PLANES];
  int n, rows;  // planes in use, the sum of their rows
};

constexpr int REC_ROWS = 4;  // rows of one thread

// Thread = (REC_ROWS consecutive rows, instance), instance fastest: the write side is contiguous, the read side too unless the
// handle is packed (inv: caller's index -> slot; nullptr on an unpacked handle, where the kernel is a streaming copy).  Every word
// has one writer.  Grid (Bp / 256, rows / REC_ROWS): the rows of a block, and with them its descriptors, are uniform (scalar
// registers, no division), and a thread has REC_ROWS loads in flight before its first store.
__global__ void __launch_bounds__(256) k_rec_save(const RecPlanes P, const int* __restrict__ inv, const int B, const int Bp) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= Bp) return;
  const int gathered = (inv && b < B) ? inv[b] : b;
  unsigned long long v[REC_ROWS];
  gptr<void> to[REC_ROWS];
  size_t at[REC_ROWS];
  int fl[REC_ROWS];
#pragma unroll
  for (int j = 0; j < REC_ROWS; j++) {
    int r = blockIdx.y * REC_ROWS + j;
    fl[j] = r < P.rows ? 0 : -1;  // (-1: past the last row)
    gptr<const void> src = P.p[0].src;
    to[j] = P.p[0].dst;
    int flags = P.p[0].flags, row = r;
    r -= P.p[0].rows;
#pragma unroll
    for (int d = 1; d < REC_MAX_PLANES; d++) {  // (constant indices: the table stays in scalar registers)
      if (d < P.n && r >= 0) src = P.p[d].src, to[j] = P.p[d].dst, flags = P.p[d].flags, row = r;
      r -= d < P.n ? P.p[d].rows : 0;
    }
    at[j] = (size_t)row * Bp;
    if (fl[j] < 0) continue;
    fl[j] = flags;
    const size_t from = at[j] + ((flags & REC_DIRECT) ? b : gathered);
    v[j] = (flags & REC_W32) ? (unsigned long long)(unsigned)((gptr<const int>)src)[from] : ((gptr<const unsigned long long>)src)[from];
  }
#pragma unroll
  for (int j = 0; j < REC_ROWS; j++) {
    if (fl[j] < 0) continue;
    if (fl[j] & REC_W32) ((gptr<int>)to[j])[at[j] + b] = (int)(unsigned)v[j];
    else ((gptr<unsigned long long>)to[j])[at[j] + b] = v[j];
  }
}

}  // namespace ltompc
