"""torch.autograd layer over a BatchedMPC handle: the solve and the plant step as differentiable functions of device tensors.

    u0, X, U, ok = mpc_solve(mpc, x0, u_prev, theta, tables)   # make_step_dev + prediction_dev; backward: adjoint_dev (and
                                                               # adjoint_tables_dev for tables), forward mode: jvp_dev,
                                                               # jvp_tables_dev for a tangent in tables (forward_tables=True)
    x_next       = plant_step(mpc, x, u0, theta, n_sub)   # plant_sensitivities_dev; backward: its Jacobians through torch.einsum

so that one tick `u0 = solve(x, u_prev, th); x = plant(x, u0, th)` is differentiable end to end and a T-tick loop backpropagates
in plain torch.  Torch plumbing only: every number comes from the handle's kernels.

All tensors are float64, contiguous and on the handle's device (`mpc.device`, the one device check; a stand-in handle with
device "cpu" runs the layer on CPU tensors).  Streams, simple and safe: torch's current stream is synchronised before the handle
is called and the handle after, so the layer neither overlaps with torch's work nor needs the handle on torch's stream.

The handle is stateful: derivatives refer to ITS last solve.  mpc_solve records the handle's `solve_count`; backward / jvp raise
a RuntimeError when another solve or initial guess has run on the handle since (solve, differentiate, then solve again), unless
the solve was made with keep=True: it then carries a solve record (BatchedMPC.record) and is differentiated from that, at any
later time, on the same handle.  Instances with ok = 0 give zero gradients, as the C interface does.
"""
from __future__ import annotations

import contextlib

import torch
from torch.autograd.function import once_differentiable

NX, NU, NTHETA, NROWS = 8, 2, 16, 4


def _check(mpc, name, t, shape):
    if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != torch.device(mpc.device):
        raise ValueError(f"{name}: expected a contiguous float64 tensor of shape {shape} on {mpc.device}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}")


def _sync_torch(mpc):
    dev = torch.device(mpc.device)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()


def _new(mpc, *shape, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device=torch.device(mpc.device))


def _dense(mpc, t, shape):
    """a tangent or cotangent as the handle reads it (None: zeros)"""
    if t is None:
        return torch.zeros(shape, dtype=torch.float64, device=torch.device(mpc.device))
    return t.to(torch.float64).expand(shape).contiguous()


def _fresh(mpc, count, what):
    if mpc.solve_count != count:
        raise RuntimeError(f"mpc_solve {what}: another solve or initial guess has run on this handle since the solve being "
                           f"differentiated (solve_count {mpc.solve_count}, recorded {count}); its derivatives are gone")


def _on(mpc, rec):
    """the passes of the body on `rec` (selected on enter, deselected on exit whatever happens); None: on the live solve"""
    return mpc.differentiating(rec) if rec is not None else contextlib.nullcontext()


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mpc, x0, u_prev, theta, tables, keep=False, forward_tables=False):
        B, N = mpc.B, mpc.N
        _check(mpc, "mpc_solve: x0", x0, (B, NX))
        if tables is not None:
            _check(mpc, "mpc_solve: tables", tables, (NROWS, mpc.n_table))  # (the handle copies n_table doubles per row)
            if getattr(mpc, "n_table_sets", 0):
                raise RuntimeError("mpc_solve: `tables` is the handle-wide table input and this handle has per-instance table sets "
                                   "(set_table_sets): no instance reads the handle's rows; adjoint_table_sets_dev gives one gradient per set")
        if u_prev is not None:
            _check(mpc, "mpc_solve: u_prev", u_prev, (B, NU))
        if theta is not None:
            _check(mpc, "mpc_solve: theta", theta, (B, NTHETA))
        u0, X, U, ok = _new(mpc, B, NU), _new(mpc, B, N + 1, NX), _new(mpc, B, N, NU), _new(mpc, B, dtype=torch.int32)
        _sync_torch(mpc)
        if tables is not None:
            for r in range(NROWS):
                mpc.set_table_values_dev(r, tables[r].data_ptr())
        if theta is not None:
            mpc.set_theta_dev(theta.data_ptr())
        if u_prev is not None:
            mpc.set_u_prev_dev(u_prev.data_ptr())
        mpc.make_step_dev(x0.data_ptr(), u0.data_ptr())
        mpc.prediction_dev(X.data_ptr(), U.data_ptr())
        mpc.sensitivities_dev(0, ok.data_ptr())  # (ok, and the factorisation that backward / jvp share)
        ctx.rec = mpc.record() if keep else None  # (keep: this solve's own record; released when the graph that holds ctx is freed)
        mpc.synchronize()
        ctx.mpc, ctx.count, ctx.has = mpc, mpc.solve_count, (u_prev is not None, theta is not None, tables is not None)
        ctx.forward_tables = bool(forward_tables)
        ctx.mark_non_differentiable(ok)
        return u0, X, U, ok

    @staticmethod
    @once_differentiable
    def backward(ctx, g_u0, g_X, g_U, _g_ok):
        mpc = ctx.mpc
        if ctx.rec is None:
            _fresh(mpc, ctx.count, "backward")
        B, N = mpc.B, mpc.N
        gX = _dense(mpc, g_X, (B, N + 1, NX))
        gU = _dense(mpc, g_U, (B, N, NU)).clone()
        if g_u0 is not None:
            gU[:, 0] += g_u0
        want_theta = ctx.has[1] and ctx.needs_input_grad[3]
        gp = _new(mpc, B, NX + NU)
        gth = _new(mpc, B, NTHETA) if want_theta else None
        want_tables = ctx.has[2] and ctx.needs_input_grad[4]
        gtab = _new(mpc, NROWS, mpc.n_table) if want_tables else None
        _sync_torch(mpc)
        with _on(mpc, ctx.rec):
            mpc.adjoint_dev(gX.data_ptr(), gU.data_ptr(), gp.data_ptr(), gth.data_ptr() if want_theta else 0, 0)
            if want_tables:
                mpc.adjoint_tables_dev(gX.data_ptr(), gU.data_ptr(), gtab.data_ptr(), 0, 0)
            mpc.synchronize()
        return None, gp[:, :NX], gp[:, NX:] if ctx.has[0] else None, gth, gtab, None, None

    @staticmethod
    def jvp(ctx, _mpc, t_x0, t_uprev, t_theta, t_tables, _keep=None, _forward_tables=None):
        mpc = ctx.mpc
        if not ctx.forward_tables and t_tables is not None and ctx.has[2] and bool((t_tables != 0).any()):  # (torch hands zeros for an input without a tangent)
            raise RuntimeError("mpc_solve jvp: forward mode is not available for `tables` unless the solve was made with "
                               "forward_tables=True (the directional pass in the tables, jvp_tables_dev); reverse mode returns grad_tables")
        if ctx.rec is None:
            _fresh(mpc, ctx.count, "jvp")
        B, N = mpc.B, mpc.N
        if not ctx.has[0]:
            t_uprev = None
        if not ctx.has[1]:
            t_theta = None
        if not ctx.has[2] or (t_tables is not None and not bool((t_tables != 0).any())):  # (torch hands zeros for an input without a tangent)
            t_tables = None
        dp = None
        if t_x0 is not None or t_uprev is not None:
            dp = torch.cat([_dense(mpc, t_x0, (B, NX)), _dense(mpc, t_uprev, (B, NU))], dim=1).contiguous()
        dth = None if t_theta is None else _dense(mpc, t_theta, (B, NTHETA))
        dtab = None if t_tables is None else _dense(mpc, t_tables, (NROWS, mpc.n_table))
        tX, tU = _new(mpc, B, N + 1, NX), _new(mpc, B, N, NU)
        if dp is None and dth is None and dtab is None:
            return _dense(mpc, None, (B, NU)), tX.zero_(), tU.zero_(), None
        _sync_torch(mpc)
        with _on(mpc, ctx.rec):
            if dtab is None:
                mpc.jvp_dev(dp.data_ptr() if dp is not None else 0, dth.data_ptr() if dth is not None else 0, tX.data_ptr(), tU.data_ptr(), 0)
            else:  # (J_p dp + J_y dy in one sweep; the map is linear, so theta's part is jvp_dev's, added)
                mpc.jvp_tables_dev(dp.data_ptr() if dp is not None else 0, dtab.data_ptr(), 0, tX.data_ptr(), tU.data_ptr(), 0)
                if dth is not None:
                    tXt, tUt = _new(mpc, B, N + 1, NX), _new(mpc, B, N, NU)
                    mpc.jvp_dev(0, dth.data_ptr(), tXt.data_ptr(), tUt.data_ptr(), 0)
            mpc.synchronize()
        if dtab is not None and dth is not None:
            tX, tU = tX + tXt, tU + tUt
        return tU[:, 0].clone(), tX, tU, None


class _Plant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mpc, x, u, theta, n_sub):
        B = mpc.B
        _check(mpc, "plant_step: x", x, (B, NX))
        _check(mpc, "plant_step: u", u, (B, NU))
        if theta is not None:
            _check(mpc, "plant_step: theta", theta, (B, NTHETA))
        want_theta = theta is not None and ctx.needs_input_grad[3]
        xn, dx, du = _new(mpc, B, NX), _new(mpc, B, NX, NX), _new(mpc, B, NX, NU)
        dth = _new(mpc, B, NX, NTHETA) if want_theta else None
        _sync_torch(mpc)
        if theta is not None:
            mpc.set_theta_dev(theta.data_ptr())
        mpc.plant_sensitivities_dev(x.data_ptr(), u.data_ptr(), xn.data_ptr(), dx.data_ptr(), du.data_ptr(),
                                    dth.data_ptr() if want_theta else 0, int(n_sub))
        mpc.synchronize()
        ctx.mpc, ctx.n_sub, ctx.dx, ctx.du, ctx.dth = mpc, int(n_sub), dx, du, dth
        ctx.xu = (x.detach(), u.detach(), theta.detach()) if theta is not None else None  # (forward mode: dtheta on request, see jvp)
        return xn

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gx = torch.einsum("bi,bij->bj", g, ctx.dx)
        gu = torch.einsum("bi,bij->bj", g, ctx.du)
        gth = torch.einsum("bi,bij->bj", g, ctx.dth) if ctx.dth is not None and ctx.needs_input_grad[3] else None
        return None, gx, gu, gth, None

    @staticmethod
    def jvp(ctx, _mpc, t_x, t_u, t_theta, _n_sub):
        mpc = ctx.mpc
        out = torch.zeros_like(ctx.dx[:, :, 0])
        if t_x is not None:
            out = out + torch.einsum("bij,bj->bi", ctx.dx, t_x)
        if t_u is not None:
            out = out + torch.einsum("bij,bj->bi", ctx.du, t_u)
        if t_theta is not None and ctx.xu is not None:
            dth = ctx.dth
            if dth is None:  # (theta needed no gradient in reverse mode: its columns now, at the forward's rows, set again)
                dth = _new(mpc, mpc.B, NX, NTHETA)
                _sync_torch(mpc)
                mpc.set_theta_dev(ctx.xu[2].data_ptr())
                mpc.plant_sensitivities_dev(ctx.xu[0].data_ptr(), ctx.xu[1].data_ptr(), 0, 0, 0, dth.data_ptr(), ctx.n_sub)
                mpc.synchronize()
            out = out + torch.einsum("bij,bj->bi", dth, t_theta)
        return out


def mpc_solve(mpc, x0, u_prev=None, theta=None, tables=None, keep=False, forward_tables=False):
    """One solve of the handle as a differentiable function: (u0 (B,2), X (B,N+1,8), U (B,N,2), ok (B,) int32) of x0 (B,8),
    u_prev (B,2; None: the one the handle makes itself, no gradient), theta (B,16 per-instance rows in THETA_NAMES order;
    None: the rows or params in effect, no gradient) and tables ((4, n_table): the value rows kappa, n_left, n_right, v_ref
    of the handle's look-up tables, TABLE_ROW_NAMES order; None: the rows in effect, no gradient).

    Forward: set_table_values_dev (the four rows) / set_theta_dev / set_u_prev_dev for the arguments given, make_step_dev,
    prediction_dev (and ok of the sensitivity pass).  Backward: adjoint_dev with the cotangent of u0 added to gU[:, 0];
    grad_theta is requested only when theta needs a gradient, and adjoint_tables_dev only when tables does (its result is the
    sum over the instances, which share the tables).  Forward mode (torch.autograd.forward_ad): jvp_dev; a tangent in `tables`
    raises a RuntimeError unless forward_tables=True, and then goes to jvp_tables_dev (the tangents of x0, u_prev and the tables in
    one sweep) plus jvp_dev's theta part (the switch keeps a caller that relied on the error as it was).  ok is not differentiable; where it is 0 all
    derivatives are 0.  Torch's current stream is synchronised before the calls and the handle after them.

    keep=True: the forward saves a solve record (BatchedMPC.record) and keeps it with the graph.  backward and
    forward mode then run on that record (select, the passes, deselect) whatever the handle has done since - later solves,
    other theta rows, other tables (the record has its own copies of the four rows) - so a T-tick closed loop backpropagates
    on ONE handle; solve_count is not checked.  The record goes back to the handle's free list when the graph is freed, so
    a training loop allocates T records once.  keep=False (the default) is the code path described above.

    The tables set here stay on the handle: they are the CONTROLLER's belief of the track from then on, and the handle's plant
    step reads the kappa row too (plant_step below takes no tables and has no gradient w.r.t. them)."""
    if forward_tables:
        return _Solve.apply(mpc, x0, u_prev, theta, tables, bool(keep), True)
    if not keep:
        return _Solve.apply(mpc, x0, u_prev, theta, tables)
    return _Solve.apply(mpc, x0, u_prev, theta, tables, True)


def plant_step(mpc, x, u, theta=None, n_sub=400):
    """The plant step as a differentiable function: x_next (B,8; the bits of plant_step_dev) of x (B,8), u (B,2) and theta
    (B,16 rows, set on the handle as set_theta_dev does; None: the rows or params in effect, no gradient).  Forward:
    plant_sensitivities_dev (dxn_dtheta only when theta needs a gradient); backward contracts the stored Jacobians with
    torch.einsum.  Same stream rule as mpc_solve.

    There is no tables input: the tables that mpc_solve differentiates are the controller's belief, the plant's track is the
    physical one.  A closed loop of mpc_solve and plant_step therefore backpropagates to n_left, n_right, v_ref and the
    controller's kappa through the solves only; the plant's own dependence on kappa is not differentiated."""
    return _Plant.apply(mpc, x, u, theta, n_sub)
