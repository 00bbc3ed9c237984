"""BatchedMPC: thin Python owner of one ltompc handle (B independent MPC instances on one MI355X)."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import LOOP_NAMES, NLOOP, NTHETA, NX, NU, TABLE_ROW_NAMES, TABLE_SLOT_NAMES, THETA_NAMES, Options, Params, check, dptr, iptr, lib
from .tables import TrackTables

KERNEL_CLASSES = ("eval", "riccati", "expand", "linesearch", "pick", "update", "riccati1", "step1")  # include/ltompc.h
NP = NX + NU  # columns of a derivative w.r.t. p = (x0[0..7], u_prev[0..1])
NSLOT = len(TABLE_SLOT_NAMES)  # table look-up results of one interval
INT32_ROWS = ("flag", "i_log")  # the names of row_shape whose elements are int32; every other one holds doubles


def row_shape(name, N=0, n=0):
    """The shape of one instance's row of the (B, ...) array `name` of the C ABI (include/ltompc.h), for horizon N and, for a log,
    n ticks.  The one place that spells them: BatchedMPC allocates and checks by it, SplitMPC offsets device pointers by it."""
    return {"x": (NX,), "u": (NU,), "X": (N + 1, NX), "U": (N, NU), "C": (N, NX), "p": (NP,), "theta": (NTHETA,),
            "du0_dp": (NU, NP), "dX_dp": (N + 1, NX, NP), "dU_dp": (N, NU, NP),
            "du0_dtheta": (NU, NTHETA), "dX_dtheta": (N + 1, NX, NTHETA), "dU_dtheta": (N, NU, NTHETA),
            "slot": (N, NSLOT), "K": (N, NU, NX), "Kv": (N, NU, NU),
            "plant_dx": (NX, NX), "plant_du": (NX, NU), "plant_dtheta": (NX, NTHETA), "loop_dx": (NX, NLOOP), "loop_du": (NU, NLOOP),
            "u_log": (n, NU), "x_log": (n, NX), "i_log": (n,),  # (policy_run_dev and rollout_dev logs; status and iterations)
            "flag": ()}[name]  # (ok, a mask, the table-set index)


class SolveRecord:
    """One saved solve of a BatchedMPC (BatchedMPC.record), or one per part of a SplitMPC (`parts`).  release() hands it back to
    the handle's free list: idempotent, and a no-op once the handle is closed (ltompc_destroy frees its records)."""

    def __init__(self, mpc, rec=None, parts=None):
        self._mpc, self._rec, self.parts, self._released = mpc, rec, parts, False

    @property
    def released(self) -> bool:
        return self._released

    def release(self):
        if self._released:
            return
        self._released = True
        if self.parts is not None:
            for r in self.parts:
                r.release()
        elif getattr(self._mpc, "_h", None) is not None and self._mpc._h.value:
            check(lib().ltompc_record_release(self._mpc._h, self._rec))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class BatchedMPC:
    """B receding-horizon NLPs of the reference's controller (src/mpc/controller.py:9-103), solved on the GPU.

    make_step(x0 (B,8)) -> u0 (B,2): the batched form of `controller.mpc.make_step(x0)` (src/mpc.py:142).
    """

    def __init__(self, tables: TrackTables, n_horizon: int = 10, batch: int = 1, params: Params | None = None,
                 options: Options | None = None, device: int = 0):
        self.tables = tables
        self.N, self.B = int(n_horizon), int(batch)
        self.params = params or _lib.default_params()
        self.options = options or _lib.default_options()
        self._tab = tables.packed()
        self.n_table = int(self._tab.shape[1])  # knots per table row (autograd.py checks `tables` against it)
        self._h = C.c_void_p()
        check(lib().ltompc_create(C.byref(self.params), C.byref(self.options), dptr(self._tab), self._tab.shape[1],
                                  self.N, self.B, int(device), C.byref(self._h)))
        # the parameters p = (x0, u_prev) of the last solve and its u0 (feedback()); the next solve's u_prev is this u0, or 0
        # after an initial guess.  None where the host does not see them (make_step_dev, rollout_dev).
        self._solved = None
        self._fb = None  # (du0_dx0, du0_duprev, ok) of that solve, fetched by the first feedback()
        self._pfb = None  # du0_dtheta of that solve, fetched by the first feedback(theta=...)
        self._theta_rows = None  # per-instance rows set (set_theta), (B, 16), None: the handle's params, _DEV_ROWS: set_theta_dev
        self._theta_solved = None  # ... those of the last solve (feedback(theta=...) expands around them)
        self.n_table_sets = 0  # per-instance table sets in effect (set_table_sets; 0: the handle's own tables)
        self._set_index_for = 1  # ... the number of sets their index was written for (1: the zeros it starts with)
        self._uprev_next = np.zeros((self.B, NU))
        self.device = f"cuda:{int(device)}"  # torch's name of the handle's device (the one device check of autograd.py)
        self.solve_count = 0  # solves and initial guesses so far: what a derivative of "the last solve" refers to (autograd.py)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().ltompc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference surface, batched -------------------------------------------------------------
    def set_initial_guess(self, x0):
        x0 = self._x(x0)
        check(lib().ltompc_set_initial_guess(self._h, dptr(x0)))
        self._solved, self._uprev_next = None, np.zeros((self.B, NU))
        self._fb = self._pfb = None
        self.solve_count += 1

    def set_u_prev(self, u_prev):
        """The previous input (B,2) of the NEXT solve's Delta-u cost, in place of the one the handle makes itself (0 after
        set_initial_guess, else the last u0); checked finite.  For that solve only; the warm start and the last solve's cached
        derivatives stay.  solved_parameters() / feedback() then report it as that solve's u_prev."""
        u = np.ascontiguousarray(np.asarray(u_prev, dtype=np.float64).reshape(-1, NU))
        if u.shape[0] != self.B:
            raise ValueError(f"set_u_prev: expected {self.B} inputs of dimension {NU}, got array of shape {u.shape}")
        check(lib().ltompc_set_u_prev(self._h, dptr(u)))
        self._uprev_next = u.copy()

    def set_u_prev_dev(self, u_prev_ptr: int):
        """set_u_prev from a device array of (B,2) float64 (ltompc_set_u_prev_dev): enqueued on the handle's stream, NOT checked.
        The host then does not see the next solve's u_prev: solved_parameters() is None after it."""
        check(lib().ltompc_set_u_prev_dev(self._h, C.c_void_p(u_prev_ptr)))
        self._uprev_next = None

    def make_step(self, x0):
        x0 = self._x(x0)
        u0 = np.empty((self.B, NU))
        self.status = np.empty(self.B, dtype=np.int32)
        self.iters = np.empty(self.B, dtype=np.int32)
        self._solved = None
        self._fb = self._pfb = None
        # (rows set from device memory: read back the ones this solve is about to use, for feedback(theta=...))
        theta_solve = self.instance_theta() if self._theta_rows is _DEV_ROWS else self._theta_rows
        self.solve_count += 1
        check(lib().ltompc_make_step(self._h, dptr(x0), dptr(u0), iptr(self.status), iptr(self.iters)))
        self._theta_solved = theta_solve
        if self._uprev_next is not None:
            self._solved = (x0.copy(), self._uprev_next.copy(), u0.copy())
        self._uprev_next = u0.copy()
        return u0

    # ---- device-pointer variants (bench, closed loop on the GPU) --------------------------------
    def set_stream(self, hip_stream: int | None):
        check(lib().ltompc_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def set_initial_guess_dev(self, x0_ptr: int):
        check(lib().ltompc_set_initial_guess_dev(self._h, C.c_void_p(x0_ptr)))
        self._solved, self._uprev_next = None, np.zeros((self.B, NU))
        self._fb = self._pfb = None
        self.solve_count += 1

    def make_step_dev(self, x0_ptr: int, u0_ptr: int):
        self._solved = self._uprev_next = None
        self._fb = self._pfb = None
        self.solve_count += 1
        check(lib().ltompc_make_step_dev(self._h, C.c_void_p(x0_ptr), C.c_void_p(u0_ptr)))
        self._theta_solved = None  # (feedback() needs a host make_step)

    def rollout_dev(self, x_ptr: int, n_ticks: int, n_sub: int = 400, u_log_ptr: int = 0, status_log_ptr: int = 0, iters_log_ptr: int = 0):
        """Closed-loop rollout with free-running instances (ltompc_rollout_dev): n_ticks of make_step + plant step per instance."""
        self._solved = self._uprev_next = None
        self._fb = self._pfb = None
        self.solve_count += 1
        check(lib().ltompc_rollout_dev(self._h, C.c_void_p(x_ptr), int(n_ticks), int(n_sub), C.c_void_p(u_log_ptr or None),
                                       C.c_void_p(status_log_ptr or None), C.c_void_p(iters_log_ptr or None)))
        self._theta_solved = None  # (feedback() needs a host make_step)
        it, ln = C.c_longlong(), C.c_longlong()
        check(lib().ltompc_rollout_info(self._h, C.byref(it), C.byref(ln)))
        return dict(iterations=it.value, launches=ln.value)

    def plant_step_dev(self, x_ptr: int, u_ptr: int, xn_ptr: int, n_sub: int = 400):
        check(lib().ltompc_plant_step_dev(self._h, C.c_void_p(x_ptr), C.c_void_p(u_ptr), int(n_sub), C.c_void_p(xn_ptr)))

    # ---- per-instance control of the warm start (ltompc_reset_instances, ...) ----------------------------------
    def _instances_changed(self, rows=None, u_prev=None):
        """After a call that changed the iterate of some instances: no solve to expand around or to differentiate
        (solve_count: autograd.py refuses the graph of the solve before it), and the next solve's u_prev of `rows` is
        u_prev (None: the host does not see it any more)."""
        self._solved = None
        self._fb = self._pfb = None
        self.solve_count += 1
        if rows is None or u_prev is None or self._uprev_next is None:
            self._uprev_next = None
        else:
            self._uprev_next[rows] = u_prev

    def reset(self, mask, x0):
        """Cold-start the instances where mask (B,) is true from x0 (B,8; the other rows are ignored): their next solve is bit
        for bit the first solve of a fresh handle (u_prev 0, no previous status, counters cleared); every other instance
        keeps its warm start to the bit.  iterate() shows the guess.  ltompc_reset_instances."""
        m, x0 = _mask(mask, self.B), self._x(x0)
        check(lib().ltompc_reset_instances(self._h, iptr(m), dptr(x0)))
        self._instances_changed(m != 0, 0.0)

    def reset_dev(self, mask_ptr: int, x0_ptr: int):
        """reset from device arrays of (B,) int32 and (B,8) float64: enqueued on the handle's stream, NOT checked."""
        check(lib().ltompc_reset_instances_dev(self._h, C.c_void_p(mask_ptr), C.c_void_p(x0_ptr)))
        self._instances_changed()

    def set_guess(self, mask, X, U, C=None, u_prev=None):
        """A primal starting point for the instances where mask (B,) is true: X (B,N+1,8), U (B,N,2), C (B,N,8) collocation
        states (None: x_k + (x_{k+1} - x_k) / 3, the Radau point at tau = 1/3), u_prev (B,2) or None (= 0).  The guess stands
        in for a previous solution that did not converge (status MAX_ITER, multipliers 0): the next solve warm-starts from it
        under the handle's warm-start options.  ltompc_set_guess."""
        m = _mask(mask, self.B)
        X = _shaped("set_guess", "X", X, self._shape("X"))
        U = _shaped("set_guess", "U", U, self._shape("U"))
        Cc = guess_collocation(X) if C is None else _shaped("set_guess", "C", C, self._shape("C"))
        up = _shaped_or_none("set_guess", "u_prev", u_prev, self._shape("u"))
        check(lib().ltompc_set_guess(self._h, iptr(m), dptr(X), dptr(Cc), dptr(U), dptr(up) if up is not None else None))
        self._instances_changed(m != 0, 0.0 if up is None else up[m != 0])

    def set_guess_dev(self, mask_ptr: int, X_ptr: int, C_ptr: int, U_ptr: int, u_prev_ptr: int = 0):
        """set_guess from device arrays (C is always given): enqueued on the handle's stream, NOT checked."""
        check(lib().ltompc_set_guess_dev(self._h, C.c_void_p(mask_ptr), C.c_void_p(X_ptr), C.c_void_p(C_ptr), C.c_void_p(U_ptr),
                                         C.c_void_p(u_prev_ptr or None)))
        self._instances_changed()

    @property
    def warm_state_size(self) -> int:
        """Doubles per instance of an export_state() row."""
        n = lib().ltompc_warm_state_size(self._h)
        if n < 0:
            check(n)
        return int(n)

    def export_state(self, idx=None):
        """The warm start of the instances idx (None: all, in order) as a (n, warm_state_size) array: everything their next
        solve depends on (planes X, C, U, L1, L2, u_prev, previous status, counters, the pending-cold flag), not the theta
        rows and tables.  Valid for import_state on handles of equal N, options and library build.  ltompc_export_state."""
        ix = _indices(idx, self.B, unique=False)
        n = self.B if ix is None else ix.size
        blob = np.empty((n, self.warm_state_size))
        check(lib().ltompc_export_state(self._h, iptr(ix) if ix is not None else None, n, dptr(blob)))
        return blob

    def export_state_dev(self, idx_ptr: int, n: int, blob_ptr: int):
        """export_state into a device array (n, warm_state_size) for a device list of n int32 indices (0: the first n
        instances): enqueued on the handle's stream."""
        check(lib().ltompc_export_state_dev(self._h, C.c_void_p(idx_ptr or None), int(n), C.c_void_p(blob_ptr)))

    def import_state(self, blob, idx=None):
        """Make the rows of an export_state() array the warm start of the instances idx (None: instance j from row j; no index
        twice): their next solve is bit for bit the one the exporting instance would have made.  iterate() / prediction()
        show the imported point; the per-solve statistics stay those of the slot's last solve.  ltompc_import_state."""
        ix = _indices(idx, self.B, unique=True)
        blob = np.ascontiguousarray(blob, dtype=np.float64)
        n = blob.shape[0] if blob.ndim == 2 else -1
        if blob.ndim != 2 or blob.shape[1] != self.warm_state_size or (ix is not None and ix.size != n) or n > self.B:
            raise ValueError(f"import_state: blob must be (n <= {self.B}, {self.warm_state_size}) with one row per index, got {blob.shape}")
        check(lib().ltompc_import_state(self._h, iptr(ix) if ix is not None else None, n, dptr(blob)))
        self._instances_changed(np.arange(n) if ix is None else ix, blob[:, WS_UPREV:WS_UPREV + NU])

    def import_state_dev(self, idx_ptr: int, n: int, blob_ptr: int):
        """import_state from a device array (n, warm_state_size) and a device list of n distinct int32 indices (0: the first n
        instances): enqueued on the handle's stream, NOT checked."""
        check(lib().ltompc_import_state_dev(self._h, C.c_void_p(idx_ptr or None), int(n), C.c_void_p(blob_ptr)))
        self._instances_changed()

    # ---- solve records (ltompc_record_*) -------------------------------------------
    def record(self, into: "SolveRecord | None" = None) -> "SolveRecord":
        """A device copy of everything the derivative passes read of the last solve (the one they would refer to now), so that
        they can run on it after the handle has gone on: select_record / differentiating.  into: a record of this handle to
        overwrite.  From the handle's free list when it has one, else allocated (one synchronisation); reuse and overwrite only
        enqueue.  Read-only on the handle (solve_count stays).  Release it (SolveRecord.release, or drop it) when done."""
        if into is not None and (into._mpc is not self or into._released):
            raise ValueError("record(into=): a live record of this handle, or None")
        rec = C.c_void_p(into._rec.value) if into is not None else C.c_void_p()
        check(lib().ltompc_record_save(self._h, C.byref(rec)))
        return into if into is not None else SolveRecord(self, rec)

    def select_record(self, rec: "SolveRecord | None"):
        """The derivative passes (sensitivities, param_sensitivities, adjoint, adjoint_tables, jvp, jvp_tables and their _dev forms) run on
        `rec` from now on, bit for bit as right after the recorded solve; None: back to the live solve.  Everything else keeps
        working on the live handle.  The first pass after a change re-linearises and re-factorises (about one iteration)."""
        if rec is not None and (not isinstance(rec, SolveRecord) or rec._mpc is not self):
            raise ValueError("select_record: a record of this handle, or None")
        if rec is not None and rec._released:
            raise ValueError("select_record: the record has been released")
        check(lib().ltompc_record_select(self._h, rec._rec if rec is not None else None))

    def differentiating(self, rec: "SolveRecord"):
        """Context manager: select_record(rec) on enter, select_record(None) on exit, whatever the body does."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.select_record(rec)
            try:
                yield rec
            finally:
                self.select_record(None)
        return scope()

    @property
    def record_size(self) -> int:
        """Device bytes of one record of this handle."""
        n = lib().ltompc_record_size(self._h)
        if n < 0:
            check(-1)
        return int(n)

    def trim_records(self):
        """Free the device memory of the released records (synchronises)."""
        check(lib().ltompc_record_trim(self._h))

    def record_stats(self):
        """(records in use, records on the free list)."""
        a, b = C.c_int(), C.c_int()
        check(lib().ltompc_record_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- parametric sensitivities (ltompc_get_sensitivities) -----------------------
    def sensitivities(self, trajectory: bool = False):
        """Derivatives of the last solve's solution w.r.t. p = (x0, u_prev), at its final iterate (include/ltompc.h).

        Returns du0_dx0 (B,2,8), du0_duprev (B,2,2), ok (B,) bool, margin (B,) and, with trajectory=True, dX (B,N+1,8,10) and
        dU (B,N,2,10) (columns: x0[0..7], u_prev[0..1]).  Where ok is False every output of the instance is 0."""
        du0, ok, margin = self._empty("du0_dp"), self._empty("flag"), np.empty(self.B)
        dX = self._empty("dX_dp") if trajectory else None
        dU = self._empty("dU_dp") if trajectory else None
        check(lib().ltompc_get_sensitivities(self._h, dptr(du0), dptr(dX) if trajectory else None, dptr(dU) if trajectory else None,
                                             iptr(ok), dptr(margin)))
        out = dict(du0_dx0=du0[:, :, :NX].copy(), du0_duprev=du0[:, :, NX:].copy(), ok=ok != 0, margin=margin)
        if trajectory:
            out.update(dX=dX, dU=dU)
        return out

    def sensitivities_dev(self, du0_dp_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue the sensitivities of the last solve into device buffers (B,2,10) doubles / (B,) int32, on the handle's stream."""
        check(lib().ltompc_sensitivities_dev(self._h, C.c_void_p(du0_dp_ptr or None), C.c_void_p(ok_ptr or None)))

    def solved_parameters(self):
        """(x0, u_prev, u0) of the last make_step, (B,8), (B,2), (B,2); None after make_step_dev / rollout_dev / set_initial_guess."""
        return self._solved

    # ---- sensitivities w.r.t. the vehicle and cost parameters (ltompc_get_param_sensitivities) -------
    def param_sensitivities(self, trajectory: bool = False):
        """Derivatives of the last solve's solution w.r.t. theta = THETA_NAMES (mass, inertia_z, the Pacejka B/C/D of both axles,
        C_m, Cr_0, Cr_2, q_n, q_mu, q_B, r_du[0], r_du[1]) in natural units, at its final iterate (include/ltompc.h).

        Returns du0_dtheta (B,2,16), names (the 16 column names), ok (B,) bool (the same as sensitivities()' ok) and, with
        trajectory=True, dX (B,N+1,8,16, block 0 is 0) and dU (B,N,2,16).  Where ok is False every output of the instance is 0."""
        du0, ok = self._empty("du0_dtheta"), self._empty("flag")
        dX = self._empty("dX_dtheta") if trajectory else None
        dU = self._empty("dU_dtheta") if trajectory else None
        check(lib().ltompc_get_param_sensitivities(self._h, dptr(du0), dptr(dX) if trajectory else None,
                                                   dptr(dU) if trajectory else None, iptr(ok)))
        out = dict(du0_dtheta=du0, names=THETA_NAMES, ok=ok != 0)
        if trajectory:
            out.update(dX=dX, dU=dU)
        return out

    def param_sensitivities_dev(self, du0_dth_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue the parameter sensitivities of the last solve into device buffers (B,2,16) doubles / (B,) int32, on the
        handle's stream."""
        check(lib().ltompc_param_sensitivities_dev(self._h, C.c_void_p(du0_dth_ptr or None), C.c_void_p(ok_ptr or None)))

    # ---- adjoint sensitivities: the gradient of a loss of the prediction (ltompc_get_adjoint) -----------
    def adjoint(self, gX=None, gU=None, theta: bool = True):
        """Gradient of a scalar loss L(X, U) of the last solve's predicted trajectory w.r.t. (x0, u_prev) and, with theta=True,
        the 16 parameters THETA_NAMES, from its cotangents gX = dL/dX (B,N+1,8) and gU = dL/dU (B,N,2) (None: zeros; not both):
        the contraction of sensitivities(trajectory=True) and param_sensitivities(trajectory=True) with (gX, gU), in one sweep
        and without the Jacobians.

        Returns grad_x0 (B,8), grad_uprev (B,2), grad_theta (B,16, only with theta=True), names, ok (B,) bool (the same as
        sensitivities()' ok).  Where ok is False every output of the instance is 0."""
        gX, gU = _shaped_or_none("adjoint", "gX", gX, self._shape("X")), _shaped_or_none("adjoint", "gU", gU, self._shape("U"))
        gp, ok = self._empty("p"), self._empty("flag")
        gth = self._empty("theta") if theta else None
        check(lib().ltompc_get_adjoint(self._h, dptr(gX) if gX is not None else None, dptr(gU) if gU is not None else None,
                                       dptr(gp), dptr(gth) if theta else None, iptr(ok)))
        out = dict(grad_x0=gp[:, :NX].copy(), grad_uprev=gp[:, NX:].copy(), names=THETA_NAMES, ok=ok != 0)
        if theta:
            out["grad_theta"] = gth
        return out

    def adjoint_dev(self, gX_ptr: int, gU_ptr: int, grad_p_ptr: int = 0, grad_theta_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue the adjoint pass of the last solve on the handle's stream: cotangents from device arrays (B,N+1,8) / (B,N,2)
        of doubles (0: zeros; not both, NOT checked for finiteness), results into device buffers (B,10) (x0[0..7], u_prev[0..1])
        / (B,16) doubles / (B,) int32; grad_theta_ptr = 0 skips the parameter part of the pass."""
        check(lib().ltompc_adjoint_dev(self._h, C.c_void_p(gX_ptr or None), C.c_void_p(gU_ptr or None), C.c_void_p(grad_p_ptr or None),
                                       C.c_void_p(grad_theta_ptr or None), C.c_void_p(ok_ptr or None)))

    # ---- adjoint gradients w.r.t. the track tables (ltompc_get_adjoint_tables) -----------------------------------
    def adjoint_tables(self, gX=None, gU=None, slots: bool = False):
        """Gradient of a scalar loss L(X, U) of the last solve's predicted trajectory w.r.t. the knot values of the four value
        rows TABLE_ROW_NAMES (kappa, n_left, n_right, v_ref), from its cotangents gX = dL/dX (B,N+1,8) and gU = dL/dU (B,N,2)
        (None: zeros; not both), summed over the instances of the handle.

        Returns grad_tables (4, n_table), names, ok (B,) bool (the same as sensitivities()' ok; an instance where it is False
        contributes 0) and, with slots=True, slot_grad (B,N,10): the gradient w.r.t. the ten look-up results of every interval
        (slot_names = TABLE_SLOT_NAMES), which is deterministic and what a table parametrisation of the caller's own chains
        through.  The last bits of grad_tables can differ between two calls (atomic adds over the instances)."""
        return self._adjoint_tables("adjoint_tables", lib().ltompc_get_adjoint_tables, "grad_tables", (), gX, gU, slots)

    def _adjoint_tables(self, who, fn, key, blocks, gX, gU, slots):
        """adjoint_tables and adjoint_table_sets: the gradient `key` has the leading shape `blocks` (one block per table set)."""
        gX, gU = _shaped_or_none(who, "gX", gX, self._shape("X")), _shaped_or_none(who, "gU", gU, self._shape("U"))
        g, ok = np.empty(blocks + (len(TABLE_ROW_NAMES), self._tab.shape[1])), self._empty("flag")
        sg = self._empty("slot") if slots else None
        check(fn(self._h, *(dptr(a) if a is not None else None for a in (gX, gU)), dptr(g), dptr(sg) if slots else None, iptr(ok)))
        out = {key: g, "names": TABLE_ROW_NAMES, "ok": ok != 0}
        if slots:
            out.update(slot_grad=sg, slot_names=TABLE_SLOT_NAMES)
        return out

    def adjoint_tables_dev(self, gX_ptr: int, gU_ptr: int, grad_tables_ptr: int = 0, slot_grad_ptr: int = 0, ok_ptr: int = 0, add: bool = False):
        """Enqueue the table-gradient pass of the last solve on the handle's stream: cotangents from device arrays (B,N+1,8) /
        (B,N,2) of doubles (0: zeros; not both, NOT checked for finiteness), results into device arrays (4,n_table) / (B,N,10)
        doubles / (B,) int32 (0: not wanted).  add=True: grad_tables is added to the array instead of overwriting it
        (ltompc_adjoint_tables_add_dev: the parts of a split batch)."""
        fn = lib().ltompc_adjoint_tables_add_dev if add else lib().ltompc_adjoint_tables_dev
        check(fn(self._h, C.c_void_p(gX_ptr or None), C.c_void_p(gU_ptr or None), C.c_void_p(grad_tables_ptr or None),
                 C.c_void_p(slot_grad_ptr or None), C.c_void_p(ok_ptr or None)))

    # ---- directional sensitivities: the Jacobians times one direction (ltompc_get_jvp) ----------------------
    def jvp(self, dp=None, dtheta=None):
        """Directional derivative of the last solve's predicted trajectory along dp (B,10: x0[0..7], u_prev[0..1]) and dtheta
        (B,16, THETA_NAMES order, natural units) (None: zeros; not both): the contraction of sensitivities(trajectory=True) and
        param_sensitivities(trajectory=True) with the direction, in one sweep and without the Jacobians.

        Returns tX (B,N+1,8; block 0 is dp[:, :8]), tU (B,N,2), ok (B,) bool (the same as sensitivities()' ok).  Where ok is
        False every output of the instance is 0."""
        dp, dtheta = _shaped_or_none("jvp", "dp", dp, self._shape("p")), _shaped_or_none("jvp", "dtheta", dtheta, self._shape("theta"))
        tX, tU, ok = self._empty("X"), self._empty("U"), self._empty("flag")
        check(lib().ltompc_get_jvp(self._h, *(dptr(a) if a is not None else None for a in (dp, dtheta)), dptr(tX), dptr(tU), iptr(ok)))
        return dict(tX=tX, tU=tU, ok=ok != 0)

    def jvp_dev(self, dp_ptr: int, dtheta_ptr: int, tX_ptr: int = 0, tU_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue the directional pass of the last solve on the handle's stream: directions from device arrays (B,10) / (B,16)
        of doubles (0: zeros; not both, NOT checked for finiteness), results into device arrays (B,N+1,8) / (B,N,2) doubles /
        (B,) int32; dtheta_ptr = 0 skips the parameter part of the pass."""
        check(lib().ltompc_jvp_dev(self._h, C.c_void_p(dp_ptr or None), C.c_void_p(dtheta_ptr or None), C.c_void_p(tX_ptr or None),
                                   C.c_void_p(tU_ptr or None), C.c_void_p(ok_ptr or None)))

    # ---- directional sensitivities along a direction in the track tables (ltompc_get_jvp_tables) ---------------
    def _jvp_tables(self, who, fn, n_blocks, dp, dtables, dslot):
        n = self._tab.shape[1]
        if dp is None and dtables is None and dslot is None:
            raise ValueError(f"{who}: dp, dtables and dslot are all None (no direction)")
        dp = _shaped_or_none(who, "dp", dp, self._shape("p"))
        dtables = _shaped_or_none(who, "dtables", dtables, (len(TABLE_ROW_NAMES), n) if n_blocks is None else (n_blocks, len(TABLE_ROW_NAMES), n))
        dslot = _shaped_or_none(who, "dslot", dslot, self._shape("slot"))
        tX, tU, ok = self._empty("X"), self._empty("U"), self._empty("flag")
        check(fn(self._h, *(dptr(a) if a is not None else None for a in (dp, dtables, dslot)), dptr(tX), dptr(tU), iptr(ok)))
        return dict(tX=tX, tU=tU, ok=ok != 0)

    def jvp_tables(self, dp=None, dtables=None, dslot=None):
        """Directional derivative of the last solve's predicted trajectory along a direction in the track tables, the forward
        twin of adjoint_tables: dtables (4, n_table), one direction in the knot values of the rows TABLE_ROW_NAMES shared by
        all instances, and / or dslot (B,N,10), the tangents of the ten look-up results of every interval (TABLE_SLOT_NAMES,
        the forward twin of slot_grad), summed; dp (B,10: x0[0..7], u_prev[0..1]) is added in the same sweep.  None: zeros;
        not all three.  A direction in theta is jvp()'s: the map is linear, add the two results.

        Returns tX (B,N+1,8; block 0 is dp[:, :8] or 0), tU (B,N,2), ok (B,) bool (the same as sensitivities()' ok).  Where
        ok is False every output of the instance is 0.  Deterministic (no atomic adds)."""
        return self._jvp_tables("jvp_tables", lib().ltompc_get_jvp_tables, None, dp, dtables, dslot)

    def jvp_tables_dev(self, dp_ptr: int = 0, dtables_ptr: int = 0, dslot_ptr: int = 0, tX_ptr: int = 0, tU_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue the directional pass in the tables of the last solve on the handle's stream: directions from device arrays
        (B,10) / (4,n_table) / (B,N,10) of doubles (0: zeros; not all three, NOT checked for finiteness), results into device
        arrays (B,N+1,8) / (B,N,2) doubles / (B,) int32 (0: not wanted)."""
        check(lib().ltompc_jvp_tables_dev(self._h, *(C.c_void_p(a or None) for a in (dp_ptr, dtables_ptr, dslot_ptr, tX_ptr, tU_ptr, ok_ptr))))

    def jvp_table_sets(self, dp=None, dtables=None, dslot=None):
        """jvp_tables on a handle with table sets: dtables is (n_sets, 4, n_table), one direction per set, and instance b moves
        along the block of its own set, on that set's rows; dp, dslot and the results as there."""
        if not self.n_table_sets:
            raise ValueError("jvp_table_sets: the handle has no table sets (set_table_sets); its directional pass in the tables is jvp_tables()")
        return self._jvp_tables("jvp_table_sets", lib().ltompc_get_jvp_table_sets, self.n_table_sets, dp, dtables, dslot)

    def jvp_table_sets_dev(self, dp_ptr: int = 0, dtables_ptr: int = 0, dslot_ptr: int = 0, tX_ptr: int = 0, tU_ptr: int = 0, ok_ptr: int = 0):
        """jvp_tables_dev on a handle with table sets: dtables is (n_sets,4,n_table) doubles."""
        check(lib().ltompc_jvp_table_sets_dev(self._h, *(C.c_void_p(a or None) for a in (dp_ptr, dtables_ptr, dslot_ptr, tX_ptr, tU_ptr, ok_ptr))))

    def prediction_dev(self, X_ptr: int = 0, U_ptr: int = 0):
        """Enqueue a copy of the last solve's prediction into device arrays (B,N+1,8) / (B,N,2) of doubles in the caller's
        order, on the handle's stream (prediction() without the host; the instances stay packed as they are)."""
        check(lib().ltompc_get_prediction_dev(self._h, C.c_void_p(X_ptr or None), C.c_void_p(U_ptr or None)))

    # ---- the feedback policy of the last solve (ltompc_get_policy, ltompc_policy_*) --------------------------
    def policy(self):
        """The time-varying feedback law of the last solve (or of the selected record), for every stage of the horizon:
        pi_k(x, v) = U_k + K_k (x - X_k) + Kv_k (v - V_k) with X, U = prediction(), V_0 the u_prev of that solve, V_k = U_{k-1}.

        Returns K (B,N,2,8), Kv (B,N,2,2) - the stage gains of the delta_w = 0 factorisation at the final iterate, K[:, 0] =
        du0_dx0 and Kv[:, 0] = du0_duprev of sensitivities() bit for bit - and ok (B,) bool (the same as sensitivities()' ok).
        Where ok is False the gains are 0: the policy is the open-loop plan."""
        K, Kv, ok = self._empty("K"), self._empty("Kv"), self._empty("flag")
        check(lib().ltompc_get_policy(self._h, dptr(K), dptr(Kv), iptr(ok)))
        return dict(K=K, Kv=Kv, ok=ok != 0)

    def policy_dev(self, K_ptr: int = 0, Kv_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue policy() into device arrays (B,N,2,8) / (B,N,2,2) doubles / (B,) int32 (0: not wanted), on the handle's stream."""
        check(lib().ltompc_policy_dev(self._h, C.c_void_p(K_ptr or None), C.c_void_p(Kv_ptr or None), C.c_void_p(ok_ptr or None)))

    def policy_step(self, k: int, x, v=None, clip: bool = False):
        """u (B,2) = pi_k(x (B,8), v (B,2)) of the last solve; v=None: V_k (no correction in that direction).  clip=True
        saturates u at the bounds of delta and T one t_step ahead, then at the input bounds (include/ltompc.h).  A non-finite x
        or v is refused."""
        x = self._x(x)
        vv = _shaped_or_none("policy_step", "v", v, self._shape("u"))
        u = self._empty("u")
        check(lib().ltompc_policy_step(self._h, int(k), dptr(x), dptr(vv) if vv is not None else None, int(bool(clip)), dptr(u)))
        return u

    def policy_step_dev(self, k: int, x_ptr: int, v_ptr: int, u_ptr: int, clip: bool = False):
        """Enqueue policy_step on the handle's stream: device arrays x (B,8), v (B,2; 0: V_k) in, u (B,2) out.  NOT checked.  It
        reads prediction and gains where they are: no gather, the instances stay packed as they are."""
        check(lib().ltompc_policy_step_dev(self._h, int(k), C.c_void_p(x_ptr), C.c_void_p(v_ptr or None), int(bool(clip)), C.c_void_p(u_ptr)))

    def policy_run_dev(self, k0: int, n: int, x_ptr: int, v_ptr: int = 0, n_sub: int = 400, clip: bool = False, u_log_ptr: int = 0,
                       x_log_ptr: int = 0):
        """n solve-free ticks in ONE launch on the handle's stream: for j < n, u_j = pi_{k0+j}(x, v); x <- plant step (the bits
        of plant_step_dev); v <- u_j.  x (B,8) device array, in and out; v (B,2) the input before the first tick (0: V_k0);
        u_log (B,n,2) and x_log (B,n,8; the state after each tick) or 0.  k0 + n <= N."""
        check(lib().ltompc_policy_run_dev(self._h, int(k0), int(n), C.c_void_p(x_ptr), C.c_void_p(v_ptr or None), int(n_sub), int(bool(clip)),
                                          C.c_void_p(u_log_ptr or None), C.c_void_p(x_log_ptr or None)))

    def policy_last_dev(self, n: int, u_log_ptr: int, u_ptr: int):
        """Enqueue, on the handle's stream, the copy of the last tick's controls of a policy_run_dev log (B,n,2) into a device
        array (B,2): what set_u_prev_dev and plant_step_dev take."""
        check(lib().ltompc_policy_last_dev(self._h, int(n), C.c_void_p(u_log_ptr), C.c_void_p(u_ptr)))

    def policy_run(self, k0: int, n: int, x, v=None, n_sub: int = 400, clip: bool = False):
        """Host convenience for policy_run_dev: the same loop written with policy_step and plant_step (the same kernels' device
        functions, so the same bits), from x (B,8) and v (B,2) or None (V_k0).  Returns dict(u=(B,n,2), x=(B,n,8) the state
        after each tick)."""
        k0, n = int(k0), int(n)
        if k0 < 0 or n < 1 or k0 + n > self.N:
            raise ValueError(f"policy_run: need 0 <= k0, 1 <= n and k0 + n <= {self.N}, got k0 = {k0}, n = {n}")
        x = self._x(x)
        v = _shaped_or_none("policy_run", "v", v, self._shape("u"))
        ul, xl = self._empty("u_log", n), self._empty("x_log", n)
        for j in range(n):
            v = self.policy_step(k0 + j, x, v, clip)
            x = self.plant_step(x, v, n_sub)
            ul[:, j], xl[:, j] = v, x
        return dict(u=ul, x=xl)

    # ---- plant-step and closed-loop sensitivities (ltompc_plant_sensitivities, ltompc_loop_*) ---------------
    def plant_sensitivities(self, x, u, n_sub: int = 400, theta: bool = True):
        """The plant step and the derivative of its discrete RK4 map at (x (B,8), u (B,2)): x_next (B,8, the bits of
        plant_step), dx (B,8,8), du (B,8,2) and, with theta=True, dtheta (B,8,16; columns THETA_NAMES, the cost columns 0);
        names.  With per-instance rows: at the rows in effect, as plant_step."""
        x, u = self._x(x), np.ascontiguousarray(np.asarray(u, float).reshape(self.B, NU))
        xn, dx, du = np.empty_like(x), self._empty("plant_dx"), self._empty("plant_du")
        dth = self._empty("plant_dtheta") if theta else None
        check(lib().ltompc_plant_sensitivities(self._h, dptr(x), dptr(u), int(n_sub), dptr(xn), dptr(dx), dptr(du),
                                               dptr(dth) if theta else None))
        out = dict(x_next=xn, dx=dx, du=du, names=THETA_NAMES)
        if theta:
            out["dtheta"] = dth
        return out

    def plant_sensitivities_dev(self, x_ptr: int, u_ptr: int, xn_ptr: int = 0, dx_ptr: int = 0, du_ptr: int = 0, dtheta_ptr: int = 0,
                                n_sub: int = 400):
        """Enqueue plant_sensitivities on the handle's stream: device arrays x (B,8), u (B,2) in; x_next (B,8), dx (B,8,8),
        du (B,8,2), dtheta (B,8,16) out (0: not wanted)."""
        check(lib().ltompc_plant_sensitivities_dev(self._h, C.c_void_p(x_ptr), C.c_void_p(u_ptr), int(n_sub), C.c_void_p(xn_ptr or None),
                                                   C.c_void_p(dx_ptr or None), C.c_void_p(du_ptr or None), C.c_void_p(dtheta_ptr or None)))

    def loop_begin(self, mode: int = 3):
        """Start accumulating the closed-loop sensitivities dx_t/dq, q = (x_init, theta): mode bit 1 - theta enters the
        controller, bit 2 - theta enters the plant."""
        check(lib().ltompc_loop_begin(self._h, int(mode)))

    def loop_tick_dev(self, x_ptr: int, u_ptr: int, xn_ptr: int, n_sub: int = 400):
        """After make_step(_dev) at x that gave u: the plant step into xn (as plant_step_dev) and one tick of the accumulation,
        enqueued on the handle's stream."""
        check(lib().ltompc_loop_tick_dev(self._h, C.c_void_p(x_ptr), C.c_void_p(u_ptr), int(n_sub), C.c_void_p(xn_ptr)))

    def loop_tick(self, x, u0, n_sub: int = 400):
        """Host form of loop_tick_dev; returns x_next (B,8)."""
        x, u0 = self._x(x), np.ascontiguousarray(np.asarray(u0, float).reshape(self.B, NU))
        xn = np.empty_like(x)
        check(lib().ltompc_loop_tick(self._h, dptr(x), dptr(u0), int(n_sub), dptr(xn)))
        return xn

    def loop_sensitivities(self):
        """dx (B,8,24) = dx_t/dq and du (B,2,24) = du_{t-1}/dq after the ticks so far, columns names = LOOP_NAMES (x_init[0..7],
        then THETA_NAMES); ok (B,) bool, ticks (B,) (the ticks accumulated while ok).  Where ok is False dx and du are 0."""
        dx, du = self._empty("loop_dx"), self._empty("loop_du")
        ok, ticks = self._empty("flag"), self._empty("flag")
        check(lib().ltompc_get_loop_sensitivities(self._h, dptr(dx), dptr(du), iptr(ok), iptr(ticks)))
        return dict(dx=dx, du=du, ok=ok != 0, ticks=ticks, names=LOOP_NAMES)

    def loop_sensitivities_dev(self, dx_ptr: int = 0, du_ptr: int = 0, ok_ptr: int = 0):
        """Enqueue a copy of the loop sensitivities into device arrays (B,8,24) / (B,2,24) doubles / (B,) int32."""
        check(lib().ltompc_loop_sensitivities_dev(self._h, C.c_void_p(dx_ptr or None), C.c_void_p(du_ptr or None), C.c_void_p(ok_ptr or None)))

    def loop_end(self):
        check(lib().ltompc_loop_end(self._h))

    def theta(self):
        """The handle's values of the 16 parameters of param_sensitivities(), in THETA_NAMES order."""
        p = self.params
        return np.array([getattr(p, n) for n in THETA_NAMES[:-2]] + [p.r_du[0], p.r_du[1]])

    # ---- settable table values (ltompc_set_table_values) ----------------------------------------------------------------
    def set_table_values(self, row, values):
        """Overwrite one value row of the handle's look-up tables: row = "kappa", "n_left", "n_right" or "v_ref" (or its index
        in TABLE_ROW_NAMES), values (n_table,) finite.  The grids stay.  From the next solve, plant step and rollout on; the
        warm start is kept; the last solve's derivatives are discarded (a derivative request before the next solve raises, and
        solved_parameters() is None).  `self.tables` stays the creation-time TrackTables; table_values() reads the rows in effect."""
        r = _table_row(row)
        v = _table_values(values, self._tab.shape[1])
        check(lib().ltompc_set_table_values(self._h, r, dptr(v)))
        self._tables_changed()

    def set_table_values_dev(self, row, values_ptr: int):
        """set_table_values from a device array of (n_table,) float64 (ltompc_set_table_values_dev): enqueued on the handle's
        stream, NOT checked."""
        check(lib().ltompc_set_table_values_dev(self._h, _table_row(row), C.c_void_p(values_ptr)))
        self._tables_changed()

    def _tables_changed(self):
        self._solved = None
        self._fb = self._pfb = None
        self.solve_count += 1  # (autograd.py: the derivatives of the solve before the set are gone)

    def table_values(self):
        """The value rows in effect, (4, n_table) in TABLE_ROW_NAMES order."""
        out = np.empty((len(TABLE_ROW_NAMES), self._tab.shape[1]))
        for r in range(out.shape[0]):
            check(lib().ltompc_get_table_values(self._h, r, dptr(out[r])))
        return out

    # ---- per-instance table sets (ltompc_set_table_sets) ---------------------------------------------------
    def set_table_sets(self, values=None, index=None):
        """Per-instance track tables: values (n_sets, 4, n_table) finite, the value rows TABLE_ROW_NAMES of every set on the
        handle's own grids, and index (B,) integers in [0, n_sets), the set of every instance.  Instance b then solves, steps
        its plant and rolls out exactly (bit for bit) as on a handle created with set index[b] written into the tables'
        value rows (in thread-per-slot evaluation mode, latency_mode = 2, which handles with sets always run).
        values=None: the sets stay, only the index changes; index=None: the index stays (all zeros before the first one);
        both None: back to the handle's own tables, which set_table_values keeps writing meanwhile.
        Timing as set_table_values: from the next solve, plant step and rollout on; the warm start is kept; the last solve's
        derivatives are discarded.  With sets in effect the derivatives w.r.t. theta, plant_sensitivities, the loop_* passes
        and adjoint_tables raise; adjoint_table_sets gives one table gradient per set."""
        if values is None and index is None:
            check(lib().ltompc_set_table_sets(self._h, 0, None, None))
            self.n_table_sets = 0
            self._tables_changed()
            return
        n_sets = self.n_table_sets
        if values is not None:
            values = _table_sets(values, self._tab.shape[1])
            n_sets = values.shape[0]
        elif not n_sets:
            raise ValueError("set_table_sets: values=None keeps the sets in effect, and there are none")
        if index is not None:
            index = _set_index(index, self.B, n_sets)
        elif n_sets < self._set_index_for:
            raise ValueError(f"set_table_sets: index=None keeps the index, which was written for {self._set_index_for} sets (now {n_sets})")
        check(lib().ltompc_set_table_sets(self._h, n_sets, dptr(values) if values is not None else None,
                                          iptr(index) if index is not None else None))
        self.n_table_sets = n_sets
        if index is not None:
            self._set_index_for = n_sets
        self._tables_changed()

    def set_table_sets_dev(self, n_sets: int, values_ptr: int = 0, index_ptr: int = 0):
        """set_table_sets from device arrays (ltompc_set_table_sets_dev): (n_sets, 4, n_table) float64 and (B,) int32, either 0
        to keep what is there (values only with n_sets unchanged); n_sets = 0 drops the sets.  Enqueued on the handle's stream.
        The values are NOT checked; the index is clamped into [0, n_sets) by the kernel that copies it."""
        n_sets = int(n_sets)
        if n_sets < 0:
            raise ValueError(f"set_table_sets_dev: n_sets must be >= 0, got {n_sets}")
        if n_sets and not values_ptr and n_sets != self.n_table_sets:
            raise ValueError(f"set_table_sets_dev: values_ptr=0 keeps the sets in effect and needs n_sets unchanged ({self.n_table_sets} in effect, {n_sets} given)")
        if n_sets and not index_ptr and n_sets < self._set_index_for:
            raise ValueError(f"set_table_sets_dev: index_ptr=0 keeps the index, which was written for {self._set_index_for} sets (now {n_sets})")
        check(lib().ltompc_set_table_sets_dev(self._h, n_sets, C.c_void_p(values_ptr or None), C.c_void_p(index_ptr or None)))
        self.n_table_sets = n_sets
        if n_sets and index_ptr:
            self._set_index_for = n_sets
        self._tables_changed()

    def table_sets(self):
        """The sets in effect: (values (n_sets, 4, n_table) in TABLE_ROW_NAMES order, index (B,) int32), or None without sets."""
        n = C.c_int(0)
        check(lib().ltompc_get_table_sets(self._h, C.byref(n), None, None))
        if not n.value:
            return None
        values, index = np.empty((n.value, len(TABLE_ROW_NAMES), self._tab.shape[1])), np.empty(self.B, dtype=np.int32)
        check(lib().ltompc_get_table_sets(self._h, C.byref(n), dptr(values), iptr(index)))
        return values, index

    def adjoint_table_sets(self, gX=None, gU=None, slots: bool = False):
        """adjoint_tables on a handle with table sets: grad_sets (n_sets, 4, n_table), block g summed over the ok instances of
        set g (zeros for a set without instances), in place of grad_tables; names, ok and, with slots=True, slot_grad as there."""
        if not self.n_table_sets:
            raise ValueError("adjoint_table_sets: the handle has no table sets (set_table_sets); its table gradient is adjoint_tables()")
        return self._adjoint_tables("adjoint_table_sets", lib().ltompc_get_adjoint_table_sets, "grad_sets", (self.n_table_sets,), gX, gU, slots)

    def adjoint_table_sets_dev(self, gX_ptr: int, gU_ptr: int, grad_sets_ptr: int = 0, slot_grad_ptr: int = 0, ok_ptr: int = 0, add: bool = False):
        """adjoint_tables_dev on a handle with table sets: grad_sets (n_sets,4,n_table) doubles in place of grad_tables
        (add=True: added to the array, ltompc_adjoint_table_sets_add_dev)."""
        fn = lib().ltompc_adjoint_table_sets_add_dev if add else lib().ltompc_adjoint_table_sets_dev
        check(fn(self._h, C.c_void_p(gX_ptr or None), C.c_void_p(gU_ptr or None), C.c_void_p(grad_sets_ptr or None),
                 C.c_void_p(slot_grad_ptr or None), C.c_void_p(ok_ptr or None)))

    # ---- per-instance vehicle and cost parameters (ltompc_set_instance_params) ----------------------------
    def set_theta(self, theta):
        """Per-instance values of the 16 parameters THETA_NAMES, from the next make_step / make_step_dev / rollout_dev / plant_step
        on (the warm start is kept; sensitivities until then stay those of the last solve).  theta: a (B, 16) array in THETA_NAMES
        order; or a dict name -> scalar or (B,) array, the other columns from the handle's params; or None: the handle's params
        again.  Every other field of Params stays the handle's.  Instance b then solves exactly (bit for bit) the NLP of a handle
        created with row b written into its params."""
        if theta is None:
            check(lib().ltompc_set_instance_params(self._h, None))
            self._theta_rows = None
            return
        rows = self._theta_array(theta)
        check(lib().ltompc_set_instance_params(self._h, dptr(rows)))
        self._theta_rows = rows

    def set_theta_dev(self, theta_ptr: int):
        """set_theta from a device array of (B, 16) float64 in THETA_NAMES order (ltompc_set_instance_params_dev): enqueued on
        the handle's stream, NOT checked.  0 = set_theta(None).  The next host make_step reads the rows back once, so that
        feedback(theta=...) expands around them."""
        if not theta_ptr:
            self.set_theta(None)
            return
        check(lib().ltompc_set_instance_params_dev(self._h, C.c_void_p(theta_ptr)))
        self._theta_rows = _DEV_ROWS

    def _theta_array(self, theta):
        return _theta_rows(theta, self.B, self.theta())

    def instance_theta(self):
        """The rows in effect, (B, 16) in THETA_NAMES order (the handle's values in every row when none are set)."""
        out = np.empty((self.B, NTHETA))
        check(lib().ltompc_get_instance_params(self._h, dptr(out)))
        return out

    def feedback(self, x, u_prev=None, *, theta=None):
        """Tangential predictor of the last make_step: u0 + du0_dx0 (x - x0_solved) + du0_duprev (u_prev - u_prev_solved), and u0
        where ok is False.  u_prev=None: the u_prev of that solve (no change in those directions).  theta: a dict name -> value
        (a scalar or a (B,) array) of parameters of param_sensitivities() (names in THETA_NAMES); adds du0_dtheta (theta -
        theta_solved), theta_solved = each instance's row of that solve (set_theta / set_theta_dev), else the handle's values.
        theta=None: no change in those directions (and no parameter pass)."""
        if theta is not None:
            u = self.feedback(x, u_prev)
            if self._pfb is None:  # one host copy per solve, not per call
                self._pfb = self.param_sensitivities()["du0_dtheta"]
            for name in theta:
                if name not in THETA_NAMES:
                    raise ValueError(f"feedback: unknown parameter {name!r} (one of {THETA_NAMES})")
            if self._theta_solved is None and all(np.ndim(v) == 0 for v in theta.values()):  # uniform handle, one value per name
                d = np.zeros(NTHETA)
                cur = self.theta()
                for name, v in theta.items():
                    j = THETA_NAMES.index(name)
                    d[j] = float(v) - cur[j]
                return u + np.einsum("bij,j->bi", self._pfb, d)  # (rows with ok False are 0)
            # around each instance's solved row; a value per name: a scalar or a (B,) array
            cur = self._theta_solved if self._theta_solved is not None else np.tile(self.theta(), (self.B, 1))
            d = np.zeros((self.B, NTHETA))
            for name, v in theta.items():
                j = THETA_NAMES.index(name)
                v = np.asarray(v, dtype=np.float64)
                if v.shape not in ((), (self.B,)):
                    raise ValueError(f"feedback: {name} must be a scalar or a ({self.B},) array, got shape {v.shape}")
                d[:, j] = v - cur[:, j]
            return u + np.einsum("bij,bj->bi", self._pfb, d)
        if self._solved is None:
            raise _lib.LtompcError("feedback: no make_step to expand around (the last solve was not a host make_step, or an "
                                   "initial guess came after it)")
        x0s, ups, u0 = self._solved
        x = self._x(x)
        up = ups if u_prev is None else np.asarray(u_prev, dtype=np.float64).reshape(self.B, NU)
        if self._fb is None:  # one host copy per solve, not per call
            S = self.sensitivities()
            self._fb = (S["du0_dx0"], S["du0_duprev"], S["ok"])
        Jx, Ju, ok = self._fb
        u = u0 + np.einsum("bij,bj->bi", Jx, x - x0s) + np.einsum("bij,bj->bi", Ju, up - ups)
        return np.where(ok[:, None], u, u0)

    # ---- results --------------------------------------------------------------------------------
    def prediction(self):
        X, U = self._empty("X"), self._empty("U")
        check(lib().ltompc_get_prediction(self._h, dptr(X), dptr(U)))
        return X, U

    def iterate(self):
        X, U = self._empty("X"), self._empty("U")
        Cc, L1, L2 = (self._empty("C") for _ in range(3))
        check(lib().ltompc_get_iterate(self._h, dptr(X), dptr(Cc), dptr(U), dptr(L1), dptr(L2)))
        ni = C.c_int()
        check(lib().ltompc_get_ineq(self._h, None, None, C.byref(ni)))
        Tt, Nu = np.empty((self.B, self.N, ni.value)), np.empty((self.B, self.N, ni.value))
        check(lib().ltompc_get_ineq(self._h, dptr(Tt), dptr(Nu), C.byref(ni)))
        return dict(X=X, C=Cc, U=U, L1=L1, L2=L2, T=Tt, NU=Nu)

    def stats(self):
        st, it = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        kkt, obj, mu = np.empty(self.B), np.empty(self.B), np.empty(self.B)
        check(lib().ltompc_get_stats(self._h, iptr(st), iptr(it), dptr(kkt), dptr(obj), dptr(mu)))
        nr, nf = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        check(lib().ltompc_get_counters(self._h, iptr(nr), iptr(nf)))
        nre, viol = np.empty(self.B, dtype=np.int32), np.empty(self.B)
        check(lib().ltompc_get_restoration(self._h, iptr(nre), dptr(viol)))
        nsh, nfb, sst = (np.empty(self.B, dtype=np.int32) for _ in range(3))
        g0, pen = np.empty(self.B), np.empty(self.B)
        check(lib().ltompc_get_recovery(self._h, iptr(nsh), iptr(nfb), dptr(g0), iptr(sst), dptr(pen)))
        return dict(status=st, iters=it, kkt=kkt, obj=obj, mu=mu, n_reg=nr, n_lsfail=nf, n_resto=nre, viol=viol,
                    n_shift=nsh, n_fallback=nfb, g0=g0, status_solver=sst, penalty=pen)

    def plant_step(self, x, u, n_sub: int = 400):
        x, u = self._x(x), np.ascontiguousarray(np.asarray(u, float).reshape(self.B, NU))
        xn = np.empty_like(x)
        check(lib().ltompc_plant_step(self._h, dptr(x), dptr(u), int(n_sub), dptr(xn)))
        return xn

    def slip_forces(self, x):
        x = np.ascontiguousarray(np.asarray(x, float).reshape(-1, NX))
        a, F = np.empty((x.shape[0], 2)), np.empty((x.shape[0], 2))
        check(lib().ltompc_slip_forces(self._h, dptr(x), x.shape[0], dptr(a), dptr(F)))
        return a, F

    def synchronize(self):
        check(lib().ltompc_synchronize(self._h))

    def set_profiling(self, on, only: str | None = None):
        """on: False / True (every launch).  only='eval' | 'riccati' | ...: bracket the launches of that kernel class only."""
        mode = int(bool(on))
        if on and only is not None:
            mode = 2 + KERNEL_CLASSES.index(only)
        check(lib().ltompc_set_profiling(self._h, mode))

    def set_poll_every(self, n: int):
        check(lib().ltompc_set_poll_every(self._h, int(n)))

    def set_narrow_width(self, width: int):
        """Widest launch (unfinished instances) that uses the one-instance-per-workgroup kernels (default 512); scheduling only."""
        check(lib().ltompc_set_narrow_width(self._h, int(width)))

    def timing(self):
        ms, ln = np.zeros(8), np.zeros(8, dtype=np.int32)
        launches, its = C.c_int(), C.c_int()
        check(lib().ltompc_get_timing(self._h, dptr(ms), iptr(ln), C.byref(launches), C.byref(its)))
        names = KERNEL_CLASSES
        return dict(ms={n: float(m) for n, m in zip(names, ms)}, launches_by_kernel={n: int(v) for n, v in zip(names, ln)},
                    launches=launches.value, ip_iterations=its.value)

    def launch_log(self, with_iterations: bool = False):
        """(kind, width, ms[, iteration]) arrays of every kernel launch of the profiled make_steps (set_profiling(True))."""
        L = lib()
        n = L.ltompc_get_launch_log(self._h, None, None, None, 0)
        kind, width, ms = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n)
        L.ltompc_get_launch_log(self._h, iptr(kind), iptr(width), dptr(ms), n)
        if not with_iterations:
            return kind, width, ms
        it = np.empty(n, dtype=np.int32)
        L.ltompc_get_launch_log_iterations(self._h, iptr(it), n)
        return kind, width, ms, it

    def active_history(self):
        """Unfinished instances after every interior-point iteration of the last make_step."""
        n = lib().ltompc_get_active_history(self._h, None, 0)
        a = np.zeros(max(n, 1), dtype=np.int32)
        lib().ltompc_get_active_history(self._h, iptr(a), n)
        return a[:n]

    def status_counts(self):
        """(histogram of the statuses of the last solve [8], sum of the iteration counts), reduced on the device."""
        c, s = np.zeros(8, dtype=np.int32), C.c_longlong()
        check(lib().ltompc_get_status_counts(self._h, iptr(c), C.byref(s)))
        return c, int(s.value)

    def solver_status_counts(self):
        """Histogram [8] of the solver's own statuses (before the node-0 rule), as reduced by the last status_counts() call."""
        c = np.zeros(8, dtype=np.int32)
        check(lib().ltompc_get_solver_status_counts(self._h, iptr(c)))
        return c

    def history(self):
        buf = np.zeros((4096, 3), dtype=np.int32)
        n = lib().ltompc_get_history(self._h, iptr(buf), 4096)
        return buf[:max(0, min(n, 4096))]

    def debug_fetch(self, which: int):
        L = lib(); L.ltompc_debug_fetch.restype = C.c_longlong
        n = L.ltompc_debug_fetch(self._h, int(which), None, C.c_longlong(0))
        buf = np.empty(n // (4 if which == 13 else 8), dtype=np.int32 if which == 13 else np.float64)
        L.ltompc_debug_fetch(self._h, int(which), buf.ctypes.data_as(C.c_void_p), C.c_longlong(n))
        return buf

    def test_model(self, x, lam, eps: float = 0.0):
        x = np.ascontiguousarray(np.asarray(x, float).reshape(-1, NX))
        lam = np.ascontiguousarray(np.asarray(lam, float).reshape(-1, NX))
        n = x.shape[0]
        out = dict(f=np.empty((n, 8)), J=np.empty((n, 8, 8)), H=np.empty((n, 8, 8)), cval=np.empty((n, 2)),
                   cgrad=np.empty((n, 2, 8)), cH=np.empty((n, 2, 8, 8)), gval=np.empty((n, 3)),
                   ggrad=np.empty((n, 3, 8)), gH=np.empty((n, 3, 8, 8)))
        check(lib().ltompc_test_model(self._h, n, C.c_double(eps), dptr(x), dptr(lam),
                                      *(dptr(out[k]) for k in ("f", "J", "H", "cval", "cgrad", "cH", "gval", "ggrad", "gH"))))
        return out

    def test_lut(self, s, eps: float = 0.0):
        """The five table look-ups of a slot (kappa at s[t]; kappa, v_ref, n_left, n_right at s[n - 1 - t]; value, slope, second
        derivative each) through lut_eval and through the batched halves: two (n, 5, 3) arrays."""
        s = np.ascontiguousarray(np.asarray(s, float).ravel())
        n = s.shape[0]
        direct, batched = np.empty((n, 5, 3)), np.empty((n, 5, 3))
        check(lib().ltompc_test_lut(self._h, n, C.c_double(eps), dptr(s), dptr(direct), dptr(batched)))
        return direct, batched

    def test_ellipse(self, x):
        x = np.ascontiguousarray(np.asarray(x, float).reshape(-1, NX))
        n = x.shape[0]
        v, g, H = np.empty((n, 2)), np.empty((n, 2, 8)), np.empty((n, 2, 8, 8))
        check(lib().ltompc_test_ellipse(self._h, n, dptr(x), dptr(v), dptr(g), dptr(H)))
        return v, g, H

    def _shape(self, name, n=0):
        """(B,) + row_shape: the whole-batch shape of the array `name`."""
        return (self.B,) + row_shape(name, self.N, n)

    def _empty(self, name, n=0):
        return np.empty(self._shape(name, n), dtype=np.int32 if name in INT32_ROWS else np.float64)

    def _x(self, x0):
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(-1, NX))
        if x0.shape[0] != self.B:
            raise ValueError(f"expected {self.B} states of dimension {NX}, got array of shape {x0.shape}")
        return x0


WS_UPREV = 7  # column of u_prev in a row of export_state() (csrc/warm_state.h)


def guess_collocation(X):
    """The collocation states of a guess from its node states X (..., N+1, 8): x_k + (x_{k+1} - x_k) / 3, the Radau point at
    tau = 1/3 on the straight line between two nodes."""
    X = np.asarray(X, dtype=np.float64)
    return np.ascontiguousarray(X[..., :-1, :] + (X[..., 1:, :] - X[..., :-1, :]) / 3.0)


def _mask(mask, B):
    """(B,) int32 0/1 from a boolean or integer mask; the shape is checked here, before any call."""
    m = np.asarray(mask)
    if m.shape != (B,):
        raise ValueError(f"mask must have shape ({B},), got {m.shape}")
    return np.ascontiguousarray(m != 0, dtype=np.int32)


def _indices(idx, B, unique):
    """int32 instance indices (None stays None: all, in order); range and, for an import, uniqueness are checked here."""
    if idx is None:
        return None
    ix = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    if ix.size and (ix.min() < 0 or ix.max() >= B):
        raise ValueError(f"instance index out of range [0, {B})")
    if unique and np.unique(ix).size != ix.size:
        raise ValueError("an instance index appears twice")
    return ix.astype(np.int32)


def _shaped(who, name, a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{who}: {name} must have shape {shape}, got {a.shape}")
    return a


def _shaped_or_none(who, name, a, shape):
    """_shaped for an optional argument: None (not given) stays None."""
    return None if a is None else _shaped(who, name, a, shape)


_DEV_ROWS = object()  # BatchedMPC._theta_rows after set_theta_dev: the rows are in device memory only


def _theta_rows(theta, B, base):
    """(B, 16) float64 rows from set_theta's argument; shapes, names and values are checked here, before any call."""
    if isinstance(theta, dict):
        rows = np.tile(base, (B, 1))
        for name, v in theta.items():
            if name not in THETA_NAMES:
                raise ValueError(f"set_theta: unknown parameter {name!r} (one of {THETA_NAMES})")
            v = np.asarray(v, dtype=np.float64)
            if v.shape not in ((), (B,)):
                raise ValueError(f"set_theta: {name} must be a scalar or a ({B},) array, got shape {v.shape}")
            rows[:, THETA_NAMES.index(name)] = v
    else:
        rows = np.asarray(theta, dtype=np.float64)
        if rows.shape != (B, NTHETA):
            raise ValueError(f"set_theta: theta must be ({B}, {NTHETA}) in THETA_NAMES order, got shape {rows.shape}")
    rows = np.array(rows, dtype=np.float64, order="C", copy=True)  # (a copy: the caller may reuse its array for the next rows)
    bad = ~np.isfinite(rows)
    bad[:, :2] |= ~(rows[:, :2] > 0)
    bad[:, 11:] |= ~(rows[:, 11:] >= 0)
    if bad.any():
        b, j = map(int, np.argwhere(bad)[0])
        raise ValueError(f"set_theta: row {b}, {THETA_NAMES[j]} = {rows[b, j]!r} (finite values; mass, inertia_z > 0; q_n, q_mu, q_B, "
                         f"r_du >= 0)")
    return rows


def _table_row(row):
    """index of a value row (set_table_values) from its name or index"""
    if isinstance(row, str):
        if row not in TABLE_ROW_NAMES:
            raise ValueError(f"set_table_values: unknown row {row!r} (one of {TABLE_ROW_NAMES})")
        return TABLE_ROW_NAMES.index(row)
    r = int(row)
    if not 0 <= r < len(TABLE_ROW_NAMES):
        raise ValueError(f"set_table_values: row must be in 0 .. {len(TABLE_ROW_NAMES) - 1} ({TABLE_ROW_NAMES}), got {row!r}")
    return r


def _table_values(values, n):
    """(n,) float64 values of one table row; shape and values are checked here, before any call."""
    v = np.array(values, dtype=np.float64, order="C", copy=True)
    if v.shape != (n,):
        raise ValueError(f"set_table_values: values must have shape ({n},), got {v.shape}")
    if not np.isfinite(v).all():
        raise ValueError(f"set_table_values: non-finite value at knot {int(np.argwhere(~np.isfinite(v))[0][0])}")
    return v


def _table_sets(values, n):
    """(n_sets, 4, n) float64 value rows of set_table_sets; shape and values are checked here, before any call."""
    v = np.array(values, dtype=np.float64, order="C", copy=True)
    if v.ndim != 3 or v.shape[0] < 1 or v.shape[1:] != (len(TABLE_ROW_NAMES), n):
        raise ValueError(f"set_table_sets: values must have shape (n_sets >= 1, {len(TABLE_ROW_NAMES)}, {n}), got {v.shape}")
    if not np.isfinite(v).all():
        g, r, i = map(int, np.argwhere(~np.isfinite(v))[0])
        raise ValueError(f"set_table_sets: non-finite value in set {g} ({TABLE_ROW_NAMES[r]}, knot {i})")
    return v


def _set_index(index, B, n_sets):
    """(B,) int32 set of every instance; shape, type and range are checked here, before any call."""
    ix = np.asarray(index)
    if ix.shape != (B,) or ix.dtype.kind not in "iu":
        raise ValueError(f"set_table_sets: index must be ({B},) integers, got shape {ix.shape}, dtype {ix.dtype}")
    bad = (ix < 0) | (ix >= n_sets)
    if bad.any():
        b = int(np.argwhere(bad)[0][0])
        raise ValueError(f"set_table_sets: index[{b}] = {int(ix[b])} is outside [0, {n_sets})")
    return np.array(ix, dtype=np.int32, order="C", copy=True)


class _Rows(NamedTuple):
    """An argument of SplitMPC._forward_dev: the device pointer of a (B, ...) array of which every part gets its own rows (0: no
    array, for every part); name and n as in row_shape."""
    ptr: int
    name: str
    n: int = 0


def _f64(a):
    """A per-instance host input as float64, for slicing by rows; None (not given) stays None."""
    return None if a is None else np.asarray(a, dtype=np.float64)


def _stitch(r, first=(), summed=()):
    """One dict from the result dicts r of the parts: a key in `first` is the same for all parts and taken from the first one; a
    key in `summed` is added up in part order, into a copy of the first part's array; every other one holds one row per
    instance and is concatenated in part order, which is the caller's."""
    out = {}
    for k in r[0]:
        if k in first:
            out[k] = r[0][k]
        elif k in summed:
            out[k] = r[0][k].copy()
            for q in r[1:]:
                out[k] += q[k]
        else:
            out[k] = np.concatenate([q[k] for q in r])
    return out


class SplitMPC:
    """The batch as `n_parts` handles of batch / n_parts instances, each on its own HIP stream and driven by its own host thread
    (ctypes releases the GIL during a call).  Instances are independent NLPs, so the parts need not tick together: while one
    part is in the narrow tail of its tick - the 1 % of its instances that need 2 - 10 times the iterations of the rest, a chain
    of one-wavefront launches on an otherwise idle chip - the other part's full-width launches fill the GPU.  Results are the
    single handle's, bit for bit (an instance's result does not depend on the batch it is solved in); 8192 instances at N = 40:
    134 k solves/s with two parts and 142 k with four against 124 k (five or more lose: the HIP runtime serves a process's streams
    with four hardware queues, and a narrow launch then waits behind another part's full-width launches in the same queue).

    The device-pointer interface of BatchedMPC for contiguous row blocks: part p owns rows [lo_p, hi_p) of every (B, .) array."""

    def __init__(self, tables: TrackTables, n_horizon: int = 10, batch: int = 1, n_parts: int = 4, params: Params | None = None,
                 options: Options | None = None, device: int = 0, narrow_width: int | None = None):
        from concurrent.futures import ThreadPoolExecutor
        self.N, self.B, self.n_parts = int(n_horizon), int(batch), int(n_parts)
        base, rem = divmod(self.B, self.n_parts)
        self.bounds = []
        lo = 0
        for p in range(self.n_parts):
            hi = lo + base + (1 if p < rem else 0)
            self.bounds.append((lo, hi)); lo = hi
        self.parts = [BatchedMPC(tables, n_horizon, hi - lo, params=params, options=options, device=device) for lo, hi in self.bounds]
        self.options, self.params = self.parts[0].options, self.parts[0].params
        self.n_table = self.parts[0].n_table
        # three or more parts beside each other: their one-instance workgroups queue for the same CUs, so the parts switch to the
        # one-instance kernels later (ltompc_set_narrow_width; scheduling only, same bits): 128 instead of 512, +2 % with four parts
        if narrow_width is None and self.n_parts >= 3:
            narrow_width = 128
        if narrow_width is not None:
            for p in self.parts:
                p.set_narrow_width(narrow_width)
        self._pool = ThreadPoolExecutor(max_workers=self.n_parts)

    def close(self):
        for p in self.parts:
            p.close()
        self._pool.shutdown(wait=True)

    def _each(self, fn):
        """fn(part, lo, hi) on every part, each in its own host thread; returns the results in part order."""
        futs = [self._pool.submit(fn, p, lo, hi) for p, (lo, hi) in zip(self.parts, self.bounds)]
        return [f.result() for f in futs]

    def _forward_dev(self, method, *args, sum_into=None):
        """BatchedMPC.`method` on every part, in part order and in the caller's thread; each part enqueues on its own stream.  A
        _Rows argument is advanced to the part's first row (a 0 pointer stays 0); any other argument - the pointer of an array
        that all parts share, a plain value - reaches every part as it is.  This is where the class offsets pointers (the timed
        loop's set_initial_guess_dev, make_step_dev, run_ticks and rollout_dev apart).
        sum_into: the pointer of an array that the parts add up in (adjoint_tables_dev).  The first part overwrites it, every
        later one is called with add=True, after the part before it has finished (the handle is synchronised in between, so the
        sum is the same from call to call up to each part's own atomic order); 0: no such array, nothing to wait for."""
        for i, (p, (lo, hi)) in enumerate(zip(self.parts, self.bounds)):
            def at(a):
                item = 4 if a.name in INT32_ROWS else 8
                return a.ptr + item * math.prod(row_shape(a.name, self.N, a.n)) * lo if a.ptr else 0
            mine = [at(a) if isinstance(a, _Rows) else a for a in args]
            if sum_into is None:
                getattr(p, method)(*mine)
            else:
                if i and sum_into:
                    self.parts[i - 1].synchronize()
                getattr(p, method)(*mine, add=i > 0)

    _shape = BatchedMPC._shape  # (the whole-batch shapes of the checks made before any part is touched)

    def _rows_of(self, *arrays):
        """(part, its rows of every array) for every part in order; an array that is None (not given) stays None."""
        for p, (lo, hi) in zip(self.parts, self.bounds):
            yield (p, *(None if a is None else a[lo:hi] for a in arrays))

    def set_initial_guess_dev(self, x0_ptr: int):
        self._each(lambda p, lo, hi: (p.set_initial_guess_dev(x0_ptr + 8 * NX * lo), p.synchronize()))

    def make_step_dev(self, x0_ptr: int, u0_ptr: int):
        self._each(lambda p, lo, hi: p.make_step_dev(x0_ptr + 8 * NX * lo, u0_ptr + 8 * NU * lo))

    def run_ticks(self, x_ptr: int, u_ptr, xn_ptr: int, n_ticks: int, n_sub: int = 400, after_tick=None, before_tick=None,
                  loop: bool = False, solve_every: int = 1, u_log_ptr: int = 0):
        """n_ticks of the closed loop [make_step; plant step] for every part at its own pace: x (B, 8) and xn (B, 8) are swapped
        after every tick (the states end in x if n_ticks is even, else in xn), u (B, 2) holds the last controls.  u_ptr may be a
        sequence of pointers: tick t then writes its controls to u_ptr[t % len(u_ptr)] (a ring: somebody else - a gather over the
        ranks, a logger - reads the controls of tick t while the parts are one tick further).
        before_tick(part_index, tick) / after_tick(part_index, tick) run in the part's thread around each of its ticks (before_tick
        may block: that is how a consumer of the ring holds a part back).  loop=True: loop_tick_dev in place of plant_step_dev
        (after loop_begin): the same states, and the closed-loop sensitivities accumulate.  Returns when all parts are done.

        solve_every=m > 1: the ticks come in groups of m.  The first tick of a group is make_step_dev +
        plant_step_dev as above; the m - 1 ticks after it (fewer in a last, shorter group) are ONE policy_run_dev(k0=1, n=m-1,
        clip=True) of that solve's feedback policy, started from its u0, which advances the states where the solve tick left
        them.  x and xn are therefore swapped once per GROUP (the states end in x if the number of groups is even), u_ptr (the
        ring: by group) receives the last control of each group, and set_u_prev_dev(that control) runs before the next solve.
        before_tick / after_tick run around each group, with the index of its first tick.  u_log_ptr: a device array (B, m-1, 2)
        that receives the policy controls of each part's current group, required for m > 2 (the last control of a group is
        gathered from it).  m must not exceed the horizon.  The warm start of the next solve is left as it is: the last
        solution shifted by ONE interval, so m intervals old for a solve m ticks later - it costs iterations; a caller who
        wants a better one sets it with set_guess_dev.  loop=True with solve_every != 1 is a ValueError (the policy ticks have
        no closed-loop sensitivities)."""
        ring = [int(u_ptr)] if isinstance(u_ptr, int) else [int(q) for q in u_ptr]
        m = int(solve_every)
        if m != 1:
            if loop:
                raise ValueError("run_ticks: loop=True needs solve_every=1 (the policy ticks have no closed-loop sensitivities)")
            if m < 1 or m > self.N:
                raise ValueError(f"run_ticks: solve_every must be in [1, {self.N}] (the policy ends with the horizon), got {solve_every}")
            if m > 2 and not u_log_ptr:
                raise ValueError("run_ticks: solve_every > 2 needs u_log_ptr, a device array (B, solve_every - 1, 2)")
            def group_body(p, lo, hi):
                a, b = x_ptr + 8 * NX * lo, xn_ptr + 8 * NX * lo
                pi = self.parts.index(p)
                for g, t in enumerate(range(0, n_ticks, m)):
                    if before_tick is not None:
                        before_tick(pi, t)
                    u = ring[g % len(ring)] + 8 * NU * lo
                    p.make_step_dev(a, u)
                    p.plant_step_dev(a, u, b, n_sub)
                    a, b = b, a
                    n = min(m, n_ticks - t) - 1
                    if n == 1:  # (a (B,1,2) log is the (B,2) array itself: v is read before u is written, by the same thread)
                        p.policy_run_dev(1, 1, a, u, n_sub, True, u_log_ptr=u)
                    elif n > 1:
                        log = u_log_ptr + 8 * NU * (m - 1) * lo
                        p.policy_run_dev(1, n, a, u, n_sub, True, u_log_ptr=log)
                        p.policy_last_dev(n, log, u)
                    if n >= 1:
                        p.set_u_prev_dev(u)
                    if after_tick is not None:
                        after_tick(pi, t)
                p.synchronize()
            self._each(group_body)
            return
        def body(p, lo, hi):
            a, b = x_ptr + 8 * NX * lo, xn_ptr + 8 * NX * lo
            pi = self.parts.index(p)
            for t in range(n_ticks):
                if before_tick is not None:
                    before_tick(pi, t)
                u = ring[t % len(ring)] + 8 * NU * lo
                p.make_step_dev(a, u)
                (p.loop_tick_dev if loop else p.plant_step_dev)(a, u, b, n_sub)
                a, b = b, a
                if after_tick is not None:
                    after_tick(pi, t)
            p.synchronize()
        self._each(body)

    def rollout_dev(self, x_ptr: int, n_ticks: int, n_sub: int = 400, u_log_ptr: int = 0, status_log_ptr: int = 0, iters_log_ptr: int = 0):
        """BatchedMPC.rollout_dev on every part at once (the logs are (B, n_ticks, .) arrays: part p fills its rows).  Returns the
        longest chain of passes over the parts and the launches of all of them."""
        def body(p, lo, hi):
            return p.rollout_dev(x_ptr + 8 * NX * lo, n_ticks, n_sub, u_log_ptr + 8 * NU * n_ticks * lo if u_log_ptr else 0,
                                 status_log_ptr + 4 * n_ticks * lo if status_log_ptr else 0, iters_log_ptr + 4 * n_ticks * lo if iters_log_ptr else 0)
        r = self._each(body)
        return dict(iterations=max(q["iterations"] for q in r), launches=sum(q["launches"] for q in r), per_part=r)

    def synchronize(self):
        for p in self.parts:
            p.synchronize()

    def set_poll_every(self, n: int):
        for p in self.parts:
            p.set_poll_every(n)

    def set_profiling(self, on, only: str | None = None):
        for p in self.parts:
            p.set_profiling(on, only)

    def status_counts(self):
        r = [p.status_counts() for p in self.parts]
        return sum(c for c, _ in r), sum(s for _, s in r)

    def solver_status_counts(self):
        return sum(p.solver_status_counts() for p in self.parts)

    def stats(self):
        return _stitch([p.stats() for p in self.parts])

    def iterate(self):
        return _stitch([p.iterate() for p in self.parts])

    # ---- per-instance control of the warm start: masks and global indices split across the parts, parts with nothing to do skipped
    def reset(self, mask, x0):
        """BatchedMPC.reset with the rows split across the parts."""
        m = _mask(mask, self.B)
        x0 = np.asarray(x0, dtype=np.float64).reshape(-1, NX)
        if x0.shape[0] != self.B:
            raise ValueError(f"reset: expected {self.B} states of dimension {NX}, got array of shape {x0.shape}")
        if not np.isfinite(x0[m != 0]).all():  # (the whole batch checked first: a bad row changes no part)
            raise ValueError("reset: non-finite x0 in a masked row")
        for p, mp, xp in self._rows_of(m, x0):
            if mp.any():
                p.reset(mp, xp)

    def reset_dev(self, mask_ptr: int, x0_ptr: int):
        """BatchedMPC.reset_dev of every part on its rows of (B,) int32 / (B,8) doubles, each on its part's stream."""
        self._forward_dev("reset_dev", _Rows(mask_ptr, "flag"), _Rows(x0_ptr, "x"))

    def set_guess(self, mask, X, U, C=None, u_prev=None):
        """BatchedMPC.set_guess with the rows split across the parts."""
        m = _mask(mask, self.B)
        X, U = _shaped("set_guess", "X", X, self._shape("X")), _shaped("set_guess", "U", U, self._shape("U"))
        Cc = guess_collocation(X) if C is None else _shaped("set_guess", "C", C, self._shape("C"))
        up = _shaped_or_none("set_guess", "u_prev", u_prev, self._shape("u"))
        on = m != 0
        if not (np.isfinite(X[on]).all() and np.isfinite(U[on]).all() and np.isfinite(Cc[on]).all() and (up is None or np.isfinite(up[on]).all())):
            raise ValueError("set_guess: non-finite entry in a masked row")  # (checked first: a bad row changes no part)
        for p, mp, *guess in self._rows_of(m, X, U, Cc, up):
            if mp.any():
                p.set_guess(mp, *guess)

    def set_guess_dev(self, mask_ptr: int, X_ptr: int, C_ptr: int, U_ptr: int, u_prev_ptr: int = 0):
        """BatchedMPC.set_guess_dev of every part on its rows, each on its part's stream."""
        self._forward_dev("set_guess_dev", _Rows(mask_ptr, "flag"), _Rows(X_ptr, "X"), _Rows(C_ptr, "C"), _Rows(U_ptr, "U"), _Rows(u_prev_ptr, "u"))

    @property
    def warm_state_size(self) -> int:
        return self.parts[0].warm_state_size

    def _by_part(self, ix):
        """(part, rows of the list, the part's own indices) for the parts that own an index of the global list ix."""
        for p, (lo, hi) in zip(self.parts, self.bounds):
            rows = np.flatnonzero((ix >= lo) & (ix < hi))
            if rows.size:
                yield p, rows, ix[rows] - lo

    def export_state(self, idx=None):
        """BatchedMPC.export_state by global index: row j = instance idx[j] of the whole batch (None: all, in order)."""
        ix = np.arange(self.B, dtype=np.int32) if idx is None else _indices(idx, self.B, unique=False)
        blob = np.empty((ix.size, self.warm_state_size))
        for p, rows, local in self._by_part(ix):
            blob[rows] = p.export_state(local)
        return blob

    def import_state(self, blob, idx=None):
        """BatchedMPC.import_state by global index (a blob row may come from any part, or from a BatchedMPC)."""
        blob = np.asarray(blob, dtype=np.float64)
        ix = np.arange(blob.shape[0], dtype=np.int32) if idx is None else _indices(idx, self.B, unique=True)
        if blob.ndim != 2 or blob.shape != (ix.size, self.warm_state_size) or ix.size > self.B:
            raise ValueError(f"import_state: blob must be (n <= {self.B}, {self.warm_state_size}) with one row per index, got {blob.shape}")
        for p, rows, local in self._by_part(ix):
            p.import_state(blob[rows], local)

    def set_theta(self, theta):
        """BatchedMPC.set_theta with the rows split across the parts (a (B, 16) array, a dict of scalars / (B,) arrays, or None)."""
        if theta is None:
            self._each(lambda p, lo, hi: p.set_theta(None))
            return
        rows = _theta_rows(theta, self.B, self.parts[0].theta())  # (the whole batch checked first: a bad row changes no part)
        for p, mine in self._rows_of(rows):
            p.set_theta(mine)

    def instance_theta(self):
        return np.concatenate([p.instance_theta() for p in self.parts])

    def set_table_values(self, row, values):
        """BatchedMPC.set_table_values on every part (row and values checked first: a bad set changes no part)."""
        r, v = _table_row(row), _table_values(values, self.n_table)
        for p in self.parts:
            p.set_table_values(r, v)

    def set_table_values_dev(self, row, values_ptr: int):
        """BatchedMPC.set_table_values_dev on every part: each copies the same (n_table,) device array on its own stream."""
        r = _table_row(row)
        for p in self.parts:
            p.set_table_values_dev(r, values_ptr)

    def table_values(self):
        """The value rows in effect (every part holds the same ones): those of the first part."""
        return self.parts[0].table_values()

    @property
    def n_table_sets(self):
        return self.parts[0].n_table_sets

    def set_table_sets(self, values=None, index=None):
        """BatchedMPC.set_table_sets: the values go to every part, the index is split by rows (both checked first: a bad set
        changes no part)."""
        if values is None and index is None:
            for p in self.parts:
                p.set_table_sets(None, None)
            return
        n_sets = self.n_table_sets
        if values is not None:
            values = _table_sets(values, self.n_table)
            n_sets = values.shape[0]
        elif not n_sets:
            raise ValueError("set_table_sets: values=None keeps the sets in effect, and there are none")
        if index is not None:
            index = _set_index(index, self.B, n_sets)
        for p, mine in self._rows_of(index):
            p.set_table_sets(values, mine)

    def set_table_sets_dev(self, n_sets: int, values_ptr: int = 0, index_ptr: int = 0):
        """BatchedMPC.set_table_sets_dev on every part: each copies the same values and its rows of the (B,) int32 index on its
        own stream."""
        self._forward_dev("set_table_sets_dev", n_sets, values_ptr, _Rows(index_ptr, "flag"))

    def table_sets(self):
        """The sets in effect: the values of the first part (every part holds the same ones), the index stitched by rows."""
        r = [p.table_sets() for p in self.parts]
        return None if r[0] is None else (r[0][0], np.concatenate([q[1] for q in r]))

    def adjoint_table_sets(self, gX=None, gU=None, slots: bool = False):
        """BatchedMPC.adjoint_table_sets of every part with its rows of the cotangents: grad_sets summed over the parts in part
        order (on the host), slot_grad and ok stitched in the caller's order."""
        r = [p.adjoint_table_sets(gXp, gUp, slots) for p, gXp, gUp in self._rows_of(_f64(gX), _f64(gU))]
        return _stitch(r, first=("names", "slot_names"), summed=("grad_sets",))

    def adjoint_table_sets_dev(self, gX_ptr: int, gU_ptr: int, grad_sets_ptr: int = 0, slot_grad_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.adjoint_table_sets_dev with the same arrays, as adjoint_tables_dev: grad_sets (n_sets,4,n_table) summed over
        the parts in part order (the first part overwrites, every later one adds after the part before it has finished)."""
        self._forward_dev("adjoint_table_sets_dev", _Rows(gX_ptr, "X"), _Rows(gU_ptr, "U"), grad_sets_ptr, _Rows(slot_grad_ptr, "slot"),
                          _Rows(ok_ptr, "flag"), sum_into=grad_sets_ptr)

    # ---- solve records: one record per part (BatchedMPC.record)
    def record(self, into: SolveRecord | None = None) -> SolveRecord:
        if into is not None and (into._mpc is not self or into._released):
            raise ValueError("record(into=): a live record of this handle, or None")
        if into is not None:
            for p, r in zip(self.parts, into.parts):
                p.record(into=r)
            return into
        return SolveRecord(self, parts=[p.record() for p in self.parts])

    def select_record(self, rec: SolveRecord | None):
        if rec is not None and (not isinstance(rec, SolveRecord) or rec._mpc is not self or rec._released):
            raise ValueError("select_record: a live record of this handle, or None")
        for i, p in enumerate(self.parts):
            p.select_record(rec.parts[i] if rec is not None else None)

    def differentiating(self, rec: SolveRecord):
        return BatchedMPC.differentiating(self, rec)

    @property
    def record_size(self) -> int:
        return sum(p.record_size for p in self.parts)

    def trim_records(self):
        for p in self.parts:
            p.trim_records()

    def record_stats(self):
        s = [p.record_stats() for p in self.parts]
        return sum(a for a, _ in s), sum(b for _, b in s)

    def sensitivities(self, trajectory: bool = False):
        """BatchedMPC.sensitivities of every part, stitched in the caller's order."""
        return _stitch([p.sensitivities(trajectory) for p in self.parts])

    def sensitivities_dev(self, du0_dp_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.sensitivities_dev of every part into its rows of (B,2,10) doubles / (B,) int32, each on its part's stream."""
        self._forward_dev("sensitivities_dev", _Rows(du0_dp_ptr, "du0_dp"), _Rows(ok_ptr, "flag"))

    def param_sensitivities(self, trajectory: bool = False):
        """BatchedMPC.param_sensitivities of every part, stitched in the caller's order."""
        return _stitch([p.param_sensitivities(trajectory) for p in self.parts], first=("names",))

    def param_sensitivities_dev(self, du0_dth_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.param_sensitivities_dev of every part into its rows of (B,2,16) doubles / (B,) int32, each on its part's
        stream."""
        self._forward_dev("param_sensitivities_dev", _Rows(du0_dth_ptr, "du0_dtheta"), _Rows(ok_ptr, "flag"))

    def adjoint(self, gX=None, gU=None, theta: bool = True):
        """BatchedMPC.adjoint of every part with its rows of the cotangents, stitched in the caller's order."""
        r = [p.adjoint(gXp, gUp, theta) for p, gXp, gUp in self._rows_of(_f64(gX), _f64(gU))]
        return _stitch(r, first=("names",))

    def adjoint_dev(self, gX_ptr: int, gU_ptr: int, grad_p_ptr: int = 0, grad_theta_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.adjoint_dev of every part on its rows of (B,N+1,8) / (B,N,2) cotangents into its rows of (B,10) / (B,16)
        doubles / (B,) int32, each on its part's stream."""
        self._forward_dev("adjoint_dev", _Rows(gX_ptr, "X"), _Rows(gU_ptr, "U"), _Rows(grad_p_ptr, "p"), _Rows(grad_theta_ptr, "theta"),
                          _Rows(ok_ptr, "flag"))

    def adjoint_tables(self, gX=None, gU=None, slots: bool = False):
        """BatchedMPC.adjoint_tables of every part with its rows of the cotangents: grad_tables summed over the parts in part
        order (on the host), slot_grad and ok stitched in the caller's order."""
        r = [p.adjoint_tables(gXp, gUp, slots) for p, gXp, gUp in self._rows_of(_f64(gX), _f64(gU))]
        return _stitch(r, first=("names", "slot_names"), summed=("grad_tables",))

    def adjoint_tables_dev(self, gX_ptr: int, gU_ptr: int, grad_tables_ptr: int = 0, slot_grad_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.adjoint_tables_dev with the same arrays: slot_grad (B,N,10) and ok (B,) by rows, each part on its own
        stream, and grad_tables (4,n_table) summed over the parts in part order: the first part overwrites the array, every
        later one adds to it after the part before it has finished (the handle is synchronised in between, so the sum is the
        same from call to call up to each part's own atomic order).  Returns with the parts' work enqueued or done."""
        self._forward_dev("adjoint_tables_dev", _Rows(gX_ptr, "X"), _Rows(gU_ptr, "U"), grad_tables_ptr, _Rows(slot_grad_ptr, "slot"),
                          _Rows(ok_ptr, "flag"), sum_into=grad_tables_ptr)

    def jvp(self, dp=None, dtheta=None):
        """BatchedMPC.jvp of every part with its rows of the directions, stitched in the caller's order."""
        return _stitch([p.jvp(dpp, dthp) for p, dpp, dthp in self._rows_of(_f64(dp), _f64(dtheta))])

    def jvp_dev(self, dp_ptr: int, dtheta_ptr: int, tX_ptr: int = 0, tU_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.jvp_dev of every part on its rows of (B,10) / (B,16) directions into its rows of (B,N+1,8) / (B,N,2)
        doubles / (B,) int32, each on its part's stream."""
        self._forward_dev("jvp_dev", _Rows(dp_ptr, "p"), _Rows(dtheta_ptr, "theta"), _Rows(tX_ptr, "X"), _Rows(tU_ptr, "U"), _Rows(ok_ptr, "flag"))

    def _jvp_tables_parts(self, name, dp, dtables, dslot):
        return _stitch([getattr(p, name)(dpp, dtables, dslotp) for p, dpp, dslotp in self._rows_of(_f64(dp), _f64(dslot))])

    def _jvp_tables_parts_dev(self, name, dp_ptr, dtables_ptr, dslot_ptr, tX_ptr, tU_ptr, ok_ptr):
        self._forward_dev(name, _Rows(dp_ptr, "p"), dtables_ptr, _Rows(dslot_ptr, "slot"), _Rows(tX_ptr, "X"), _Rows(tU_ptr, "U"),
                          _Rows(ok_ptr, "flag"))

    def jvp_tables(self, dp=None, dtables=None, dslot=None):
        """BatchedMPC.jvp_tables of every part: dtables to every part, dp and dslot by the part's rows, the results stitched in
        the caller's order (they are per instance: nothing is summed over the parts)."""
        return self._jvp_tables_parts("jvp_tables", dp, dtables, dslot)

    def jvp_tables_dev(self, dp_ptr: int = 0, dtables_ptr: int = 0, dslot_ptr: int = 0, tX_ptr: int = 0, tU_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.jvp_tables_dev of every part on the same (4,n_table) direction and its rows of (B,10) / (B,N,10) into its
        rows of (B,N+1,8) / (B,N,2) doubles / (B,) int32, each on its part's stream."""
        self._jvp_tables_parts_dev("jvp_tables_dev", dp_ptr, dtables_ptr, dslot_ptr, tX_ptr, tU_ptr, ok_ptr)

    def jvp_table_sets(self, dp=None, dtables=None, dslot=None):
        """BatchedMPC.jvp_table_sets of every part, as jvp_tables: the (n_sets,4,n_table) direction to every part."""
        return self._jvp_tables_parts("jvp_table_sets", dp, dtables, dslot)

    def jvp_table_sets_dev(self, dp_ptr: int = 0, dtables_ptr: int = 0, dslot_ptr: int = 0, tX_ptr: int = 0, tU_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.jvp_table_sets_dev of every part, as jvp_tables_dev."""
        self._jvp_tables_parts_dev("jvp_table_sets_dev", dp_ptr, dtables_ptr, dslot_ptr, tX_ptr, tU_ptr, ok_ptr)

    def set_u_prev(self, u_prev):
        """BatchedMPC.set_u_prev with the rows split across the parts."""
        u = np.asarray(u_prev, dtype=np.float64).reshape(-1, NU)
        if u.shape[0] != self.B:
            raise ValueError(f"set_u_prev: expected {self.B} inputs of dimension {NU}, got array of shape {u.shape}")
        if not np.isfinite(u).all():  # (the whole batch checked first: a bad row changes no part)
            raise ValueError(f"set_u_prev: non-finite u_prev of instance {int(np.argwhere(~np.isfinite(u))[0][0])}")
        for p, mine in self._rows_of(u):
            p.set_u_prev(mine)

    def set_u_prev_dev(self, u_prev_ptr: int):
        """BatchedMPC.set_u_prev_dev of every part on its rows of (B,2) doubles, each on its part's stream."""
        self._forward_dev("set_u_prev_dev", _Rows(u_prev_ptr, "u"))

    def plant_sensitivities(self, x, u, n_sub: int = 400, theta: bool = True):
        """BatchedMPC.plant_sensitivities of every part on its rows, stitched in the caller's order."""
        x, u = np.asarray(x, dtype=np.float64).reshape(self._shape("x")), np.asarray(u, dtype=np.float64).reshape(self._shape("u"))
        return _stitch([p.plant_sensitivities(xp, up, n_sub, theta) for p, xp, up in self._rows_of(x, u)], first=("names",))

    def plant_sensitivities_dev(self, x_ptr: int, u_ptr: int, xn_ptr: int = 0, dx_ptr: int = 0, du_ptr: int = 0, dtheta_ptr: int = 0,
                                n_sub: int = 400):
        """BatchedMPC.plant_sensitivities_dev of every part on its rows, each on its part's stream."""
        self._forward_dev("plant_sensitivities_dev", _Rows(x_ptr, "x"), _Rows(u_ptr, "u"), _Rows(xn_ptr, "x"), _Rows(dx_ptr, "plant_dx"),
                          _Rows(du_ptr, "plant_du"), _Rows(dtheta_ptr, "plant_dtheta"), n_sub)

    def loop_begin(self, mode: int = 3):
        for p in self.parts:
            p.loop_begin(mode)

    def loop_tick_dev(self, x_ptr: int, u_ptr: int, xn_ptr: int, n_sub: int = 400):
        """BatchedMPC.loop_tick_dev of every part on its rows of x (B,8), u (B,2), xn (B,8), each on its part's stream."""
        self._forward_dev("loop_tick_dev", _Rows(x_ptr, "x"), _Rows(u_ptr, "u"), _Rows(xn_ptr, "x"), n_sub)

    def loop_tick(self, x, u0, n_sub: int = 400):
        x, u0 = np.asarray(x, dtype=np.float64).reshape(self._shape("x")), np.asarray(u0, dtype=np.float64).reshape(self._shape("u"))
        return np.concatenate([p.loop_tick(xp, up, n_sub) for p, xp, up in self._rows_of(x, u0)])

    def loop_sensitivities(self):
        """BatchedMPC.loop_sensitivities of every part, stitched in the caller's order."""
        return _stitch([p.loop_sensitivities() for p in self.parts], first=("names",))

    def loop_sensitivities_dev(self, dx_ptr: int = 0, du_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.loop_sensitivities_dev of every part into its rows of (B,8,24) / (B,2,24) doubles / (B,) int32."""
        self._forward_dev("loop_sensitivities_dev", _Rows(dx_ptr, "loop_dx"), _Rows(du_ptr, "loop_du"), _Rows(ok_ptr, "flag"))

    def loop_end(self):
        for p in self.parts:
            p.loop_end()

    def prediction_dev(self, X_ptr: int = 0, U_ptr: int = 0):
        """BatchedMPC.prediction_dev of every part into its rows of (B,N+1,8) / (B,N,2) doubles, each on its part's stream."""
        self._forward_dev("prediction_dev", _Rows(X_ptr, "X"), _Rows(U_ptr, "U"))

    # ---- the feedback policy (BatchedMPC.policy): by global index, each part fills its rows
    def policy(self):
        """BatchedMPC.policy of every part, stitched in the caller's order."""
        return _stitch([p.policy() for p in self.parts])

    def policy_dev(self, K_ptr: int = 0, Kv_ptr: int = 0, ok_ptr: int = 0):
        """BatchedMPC.policy_dev of every part into its rows of (B,N,2,8) / (B,N,2,2) doubles / (B,) int32, each on its part's stream."""
        self._forward_dev("policy_dev", _Rows(K_ptr, "K"), _Rows(Kv_ptr, "Kv"), _Rows(ok_ptr, "flag"))

    def policy_step(self, k: int, x, v=None, clip: bool = False):
        """BatchedMPC.policy_step with the rows split across the parts (shapes and finiteness checked first: a bad row reaches no part)."""
        x = _shaped("policy_step", "x", x, self._shape("x"))
        v = _shaped_or_none("policy_step", "v", v, self._shape("u"))
        if not (np.isfinite(x).all() and (v is None or np.isfinite(v).all())):
            raise ValueError("policy_step: non-finite x or v")
        return np.concatenate([p.policy_step(k, xp, vp, clip) for p, xp, vp in self._rows_of(x, v)])

    def policy_step_dev(self, k: int, x_ptr: int, v_ptr: int, u_ptr: int, clip: bool = False):
        """BatchedMPC.policy_step_dev of every part on its rows of x (B,8), v (B,2; 0: V_k), u (B,2), each on its part's stream."""
        self._forward_dev("policy_step_dev", k, _Rows(x_ptr, "x"), _Rows(v_ptr, "u"), _Rows(u_ptr, "u"), clip)

    def policy_run_dev(self, k0: int, n: int, x_ptr: int, v_ptr: int = 0, n_sub: int = 400, clip: bool = False, u_log_ptr: int = 0,
                       x_log_ptr: int = 0):
        """BatchedMPC.policy_run_dev of every part on its rows of x (B,8), v (B,2), u_log (B,n,2), x_log (B,n,8), each on its
        part's stream."""
        n = int(n)
        self._forward_dev("policy_run_dev", k0, n, _Rows(x_ptr, "x"), _Rows(v_ptr, "u"), n_sub, clip, _Rows(u_log_ptr, "u_log", n),
                          _Rows(x_log_ptr, "x_log", n))

    def policy_last_dev(self, n: int, u_log_ptr: int, u_ptr: int):
        """BatchedMPC.policy_last_dev of every part on its rows of u_log (B,n,2) and u (B,2), each on its part's stream."""
        n = int(n)
        self._forward_dev("policy_last_dev", n, _Rows(u_log_ptr, "u_log", n), _Rows(u_ptr, "u"))

    def policy_run(self, k0: int, n: int, x, v=None, n_sub: int = 400, clip: bool = False):
        """BatchedMPC.policy_run with the rows split across the parts, stitched in the caller's order."""
        x = _shaped("policy_run", "x", x, self._shape("x"))
        v = _shaped_or_none("policy_run", "v", v, self._shape("u"))
        return _stitch([p.policy_run(k0, n, xp, vp, n_sub, clip) for p, xp, vp in self._rows_of(x, v)])
