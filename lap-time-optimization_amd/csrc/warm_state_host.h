// warm_state_host.h — host side of warm_state.h, part of ltompc.hip only: ltompc_reset_instances, ltompc_set_guess,
// ltompc_export_state, ltompc_import_state and their _dev forms (include/ltompc.h).
#pragma once

namespace {

// The flags (and the inverse of `orig`, for the index lists of a packed handle) exist from the first of the new calls on.
int ws_alloc(ltompc_solver* h) {
  if (h->d_cold) return 0;
  if (h->dalloc(&h->d_cold, h->Bp) || h->dalloc(&h->d_inv, h->Bp)) return -1;
  return 0;
}
// Before a call that changes single instances: the handle-wide "next solve is cold" becomes every instance's flag, and the
// start of the next solve reads the flags.
int ws_begin(ltompc_solver* h) {
  if (ws_alloc(h)) return -1;
  if (h->cold_next) {
    HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)h->d_cold, 1, h->B, h->stream));
    h->cold_next = false;
  }
  h->cold_pending = true;
  h->dv.discard();  // (an iterate changes: no solve to differentiate)
  return 0;
}
int ws_usable(ltompc_solver* h, const char* who) {
  if (!h) return fail(std::string(who) + ": null handle");
  if (h->dv.loop_mode) return fail(std::string(who) + ": not available inside an open loop (it would break the chain of the loop's instances; ltompc_loop_end first)");
  return 0;
}
// caller's index -> slot, when the instances are packed
const int* ws_inverse(ltompc_solver* h) {
  if (!h->packed) return nullptr;
  hipLaunchKernelGGL(k_pack_inverse, dim3((h->B + 63) / 64), dim3(64), 0, h->stream, h->d_orig, h->d_inv, h->B);
  return h->d_inv;
}
// staging of the host forms: n rows of a blob (or a guess, which is smaller) and Bp ints
int ws_stage(ltompc_solver* h) {
  if (h->d_ws_stage) return 0;
  return (h->dalloc(&h->d_ws_stage, (size_t)ws_size(h->N) * h->B) || h->dalloc(&h->d_ws_int, h->Bp)) ? -1 : 0;
}
int ws_check_idx(ltompc_solver* h, const int* idx, const int n, const bool unique, const char* who) {
  if (n < 0 || (!idx && n > h->B)) return fail(std::string(who) + ": n out of range");
  if (!idx) return 0;
  std::vector<char> seen(unique ? h->B : 0, 0);
  for (int j = 0; j < n; j++) {
    if (idx[j] < 0 || idx[j] >= h->B) return fail(std::string(who) + ": idx[" + std::to_string(j) + "] = " + std::to_string(idx[j]) + " is out of range");
    if (unique && seen[idx[j]]++) return fail(std::string(who) + ": instance " + std::to_string(idx[j]) + " appears twice in idx");
  }
  return 0;
}
unsigned ws_copy_blocks(const ltompc_solver* h, const int n) {
  return (unsigned)(((n + WS_TILE - 1) / WS_TILE) * ((ws_size(h->N) + WS_TILE - 1) / WS_TILE));
}

}  // namespace

extern "C" {

int ltompc_warm_state_size(ltompc_handle h) {
  if (!h) return fail("null handle");
  return ws_size(h->N);
}

int ltompc_reset_instances_dev(ltompc_handle h, const int* mask_dev, const double* x0_dev) {
  const char* who = "ltompc_reset_instances";
  if (ws_usable(h, who)) return -1;
  if (!mask_dev || !x0_dev) return fail(std::string(who) + ": null argument");
  HIPCHECK(hipSetDevice(h->device));
  if (ws_begin(h)) return -1;
  hipLaunchKernelGGL(k_ws_reset_mark, dim3((h->B + 63) / 64), dim3(64), 0, h->stream, h->W, mask_dev, x0_dev, h->d_cold);
  hipLaunchKernelGGL(k_ws_reset_init, dim3((h->N * h->Bp + 63) / 64), dim3(64), 0, h->stream, h->d_K, h->d_W, mask_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

int ltompc_reset_instances(ltompc_handle h, const int* mask, const double* x0) {
  const char* who = "ltompc_reset_instances";
  if (ws_usable(h, who)) return -1;
  if (!mask || !x0) return fail(std::string(who) + ": null argument");
  int n_set = 0;
  for (int b = 0; b < h->B; b++) {
    if (!mask[b]) continue;
    n_set++;
    for (int i = 0; i < 8; i++)
      if (!std::isfinite(x0[(size_t)b * 8 + i])) return fail(std::string(who) + ": non-finite x0 of instance " + std::to_string(b));
  }
  if (!n_set) return 0;
  HIPCHECK(hipSetDevice(h->device));
  if (ws_stage(h)) return -1;
  HIPCHECK(hipMemcpyAsync(h->d_ws_int, mask, sizeof(int) * h->B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->d_x0_rm, x0, sizeof(double) * 8 * h->B, hipMemcpyHostToDevice, h->stream));
  if (ltompc_reset_instances_dev(h, h->d_ws_int, h->d_x0_rm)) return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_set_guess_dev(ltompc_handle h, const int* mask_dev, const double* X_dev, const double* C_dev, const double* U_dev, const double* u_prev_dev) {
  const char* who = "ltompc_set_guess";
  if (ws_usable(h, who)) return -1;
  if (!mask_dev || !X_dev || !C_dev || !U_dev) return fail(std::string(who) + ": null argument");
  HIPCHECK(hipSetDevice(h->device));
  if (ws_begin(h)) return -1;
  const size_t nthreads = (size_t)(h->N + 1) * h->Bp;
  hipLaunchKernelGGL(k_ws_guess, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, h->stream, h->W, mask_dev, X_dev, C_dev, U_dev, u_prev_dev,
                     h->d_cold);
  HIPCHECK(hipGetLastError());
  return 0;
}

int ltompc_set_guess(ltompc_handle h, const int* mask, const double* X, const double* C, const double* U, const double* u_prev) {
  const char* who = "ltompc_set_guess";
  if (ws_usable(h, who)) return -1;
  if (!mask || !X || !C || !U) return fail(std::string(who) + ": null argument");
  const size_t N = h->N, B = h->B, nX = 8 * (N + 1), nC = 8 * N, nU = 2 * N;
  int n_set = 0;
  const auto finite = [](const double* p, const size_t n) {
    for (size_t i = 0; i < n; i++)
      if (!std::isfinite(p[i])) return false;
    return true;
  };
  for (size_t b = 0; b < B; b++) {
    if (!mask[b]) continue;
    n_set++;
    if (!finite(X + b * nX, nX) || !finite(C + b * nC, nC) || !finite(U + b * nU, nU) || (u_prev && !finite(u_prev + b * 2, 2)))
      return fail(std::string(who) + ": non-finite entry in the guess of instance " + std::to_string(b));
  }
  if (!n_set) return 0;
  HIPCHECK(hipSetDevice(h->device));
  if (ws_stage(h)) return -1;
  double *dX = h->d_ws_stage, *dC = dX + B * nX, *dU = dC + B * nC;  // (B (34 N + 8) > B (18 N + 8) doubles)
  HIPCHECK(hipMemcpyAsync(h->d_ws_int, mask, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(dX, X, sizeof(double) * B * nX, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(dC, C, sizeof(double) * B * nC, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(dU, U, sizeof(double) * B * nU, hipMemcpyHostToDevice, h->stream));
  if (u_prev) HIPCHECK(hipMemcpyAsync(h->d_u0_rm, u_prev, sizeof(double) * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (ltompc_set_guess_dev(h, h->d_ws_int, dX, dC, dU, u_prev ? h->d_u0_rm : nullptr)) return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int ltompc_export_state_dev(ltompc_handle h, const int* idx_dev, int n, double* blob_dev) {
  const char* who = "ltompc_export_state";
  if (!h || !blob_dev) return fail(std::string(who) + ": null argument");
  if (n < 0 || (!idx_dev && n > h->B)) return fail(std::string(who) + ": n out of range");
  if (n == 0) return 0;
  HIPCHECK(hipSetDevice(h->device));
  if (ws_alloc(h)) return -1;
  const int* inv = ws_inverse(h);
  hipLaunchKernelGGL(k_ws_export, dim3(ws_copy_blocks(h, n)), dim3(256), 0, h->stream, h->W, idx_dev, inv, n, blob_dev, (const int*)h->d_cold,
                     h->cold_next ? 1 : 0);
  HIPCHECK(hipGetLastError());
  return 0;
}

int ltompc_export_state(ltompc_handle h, const int* idx, int n, double* blob) {
  const char* who = "ltompc_export_state";
  if (!h || !blob) return fail(std::string(who) + ": null argument");
  if (ws_check_idx(h, idx, n, false, who)) return -1;
  if (n == 0) return 0;
  HIPCHECK(hipSetDevice(h->device));
  const size_t S = ws_size(h->N);
  for (int j0 = 0; j0 < n; j0 += h->B) {  // (idx may name an instance more than once: chunks of the staging's B rows)
    const int m = std::min(h->B, n - j0);
    if (ws_stage(h)) return -1;
    if (idx) HIPCHECK(hipMemcpyAsync(h->d_ws_int, idx + j0, sizeof(int) * m, hipMemcpyHostToDevice, h->stream));
    if (ltompc_export_state_dev(h, idx ? h->d_ws_int : nullptr, m, h->d_ws_stage)) return -1;
    HIPCHECK(hipMemcpyAsync(blob + (size_t)j0 * S, h->d_ws_stage, sizeof(double) * S * m, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int ltompc_import_state_dev(ltompc_handle h, const int* idx_dev, int n, const double* blob_dev) {
  const char* who = "ltompc_import_state";
  if (ws_usable(h, who)) return -1;
  if (!blob_dev) return fail(std::string(who) + ": null argument");
  if (n < 0 || (!idx_dev && n > h->B)) return fail(std::string(who) + ": n out of range");
  if (n == 0) return 0;
  HIPCHECK(hipSetDevice(h->device));
  if (ws_begin(h)) return -1;
  const int* inv = ws_inverse(h);
  hipLaunchKernelGGL(k_ws_import, dim3(ws_copy_blocks(h, n)), dim3(256), 0, h->stream, h->W, idx_dev, inv, n, blob_dev, h->d_cold);
  HIPCHECK(hipGetLastError());
  return 0;
}

int ltompc_import_state(ltompc_handle h, const int* idx, int n, const double* blob) {
  const char* who = "ltompc_import_state";
  if (ws_usable(h, who)) return -1;
  if (!blob) return fail(std::string(who) + ": null argument");
  if (ws_check_idx(h, idx, n, true, who)) return -1;
  if (n > h->B) return fail(std::string(who) + ": n out of range");
  const size_t S = ws_size(h->N);
  for (int j = 0; j < n; j++) {
    const double* row = blob + (size_t)j * S;
    const std::string at = " in row " + std::to_string(j);
    if (!(row[WS_HDR] == ws_header(h->N)))
      return fail(std::string(who) + ": wrong header" + at + " (a blob of another horizon, another layout version, or not a blob)");
    for (int c = WS_STATUS; c <= WS_COLD; c++)
      if (!(row[c] >= 0.0 && row[c] <= 1e6 && row[c] == std::floor(row[c]))) return fail(std::string(who) + ": bad state word " + std::to_string(c) + at);
    if (!(row[WS_STATUS] <= 7.0) || !(row[WS_NODE0] <= 8.0)) return fail(std::string(who) + ": bad status" + at);
    // (the planes of an instance that starts cold are overwritten before they are read: a never-solved handle may export anything)
    for (size_t c = WS_UPREV; c < (row[WS_COLD] != 0.0 ? (size_t)WS_META : S); c++)
      if (!std::isfinite(row[c])) return fail(std::string(who) + ": non-finite payload" + at + ", word " + std::to_string(c));
  }
  if (n == 0) return 0;
  HIPCHECK(hipSetDevice(h->device));
  if (ws_stage(h)) return -1;
  if (idx) HIPCHECK(hipMemcpyAsync(h->d_ws_int, idx, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->d_ws_stage, blob, sizeof(double) * S * n, hipMemcpyHostToDevice, h->stream));
  if (ltompc_import_state_dev(h, idx ? h->d_ws_int : nullptr, n, h->d_ws_stage)) return -1;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
