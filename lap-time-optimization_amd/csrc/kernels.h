// kernels.h — HIP kernels of the batched interior-point NLP solver (gfx950).
//
// One make_step (reference src/mpc.py:142, do_mpc MPC.make_step -> IPOPT) = up to max_iter interior-point
// iterations, each a fixed sequence of kernels over the instances that have not finished:
//
//   layout.h      buffers, field indices, Work / Launch / Consts, wave-level helpers
//   linearise.h   (kernels instantiated for the reference's bound pattern, BoundsRef, and for a run-time pattern)
//                 k_eval    thread = (interval k, instance b): derivatives of dynamics / cost / constraints at the
//                           Radau point and the next node, KKT-residual partials, block-structured elimination of the
//                           collocation variables -> stage QP blocks (A, B, b, Q, S, R, q, r)
//                 k_expand  thread = (k, b): collocation steps and multipliers, slack / inequality-multiplier steps,
//                           fraction-to-the-boundary partials
//   eval8.h       k_eval8 / k_expand8: the same with 8 lanes per (k, b) (latency mode)
//   riccati.h     k_riccati8 (8 instances per wavefront) / k_riccati1 (one instance per wavefront) / k_riccati1q (one instance
//                 on four wavefronts, launches of at most 16 instances) / k_riccati (one thread per instance, reference implementation): KKT error, termination, barrier update, Riccati
//                 backward sweep with inertia-correcting regularisation, forward rollout
//   linesearch.h  k_linesearch (filter measures of the step candidates), k_pick (filter test, step length, stall
//                 bookkeeping), k_update (z += alpha dz), k_step1 (the three fused, one workgroup per instance)
//   aux_kernels.h k_init, k_shift, re-packing of the unfinished instances (k_pack_perm / k_pack move their data to the
//                 front of the batch, k_compact re-packs the index list only), I/O, k_plant (RK4 plant step), test hooks
//   rollout.h     k_roll_*: closed-loop rollout with free-running instances (ltompc_rollout_dev)
//   velocity.h    k_velocity_profile: the forward / backward speed-profile passes of src/velocity.py
//   sensitivity.h k_sens_*: parametric sensitivities of the solution w.r.t. (x0, u_prev) at the final iterate
//                 (ltompc_get_sensitivities): re-linearisation, head-less Riccati sweep at delta_w = 0, forward propagation
//   param_sensitivity.h k_psens_*: the same w.r.t. the vehicle and cost parameters (ltompc_get_param_sensitivities): condensed
//                 right-hand sides of the 16 columns, their backward recursion on the stored factorisation, forward pass
//   adjoint.h     k_adj_sweep: the gradient of a loss of the predicted trajectory w.r.t. (x0, u_prev, theta) from its cotangents
//                 (ltompc_get_adjoint): one backward / forward recursion of vectors on the same factorisation, contracted with
//                 k_psens_cond's planes; k_prediction_dev: the prediction as device arrays in the caller's order
//   jvp.h         k_jvp_sweep: the product of those Jacobians with one direction (dp, dtheta) (ltompc_get_jvp): the backward recursion
//                 of the one dtheta-weighted vector and one forward pass on the same factorisation; k_set_uprev (ltompc_set_u_prev)
//   plant_sensitivity.h k_plant_sens: the derivative of k_plant's discrete RK4 map w.r.t. (x, u, theta) (ltompc_plant_sensitivities);
//                 k_loop_accum: the closed-loop recursion that chains it with the du0 outputs of the two forward passes over many
//                 ticks (ltompc_loop_*)
//   table_sensitivity.h k_adj_sweep_tab, k_tab_cond, k_tab_scatter: the gradient of a loss of the predicted trajectory w.r.t. the knot
//                 values of the track tables (ltompc_get_adjoint_tables): adjoint.h's recursion keeping its trajectory,
//                 the per-slot contraction with the condensed columns of the ten look-up results, the scatter to the knots (lut_basis)
//   table_jvp.h   k_tabjvp_cond, k_jvp_sweep_tab: the product of those Jacobians w.r.t. the knot values with one direction
//                 (ltompc_get_jvp_tables): the ten look-up tangents of every slot (given, or gathered with lut_basis),
//                 their columns condensed into one stage vector, jvp.h's recursion on it
//   deriv_passes.h (host, part of ltompc.hip only) the drivers and C entry points of the passes of the seven headers above
//   warm_state.h  per-instance control of the warm start: k_load_x0_m / k_init_m / k_roll_mark_m / k_roll_init_m (the
//                 start of a solve with a per-instance cold flag), k_ws_reset_* (ltompc_reset_instances), k_ws_guess (ltompc_set_guess),
//                 k_ws_export / k_ws_import (the carried state of chosen instances <-> instance-major blobs, an LDS tile transpose)
//   warm_state_host.h (host, part of ltompc.hip only) their C entry points
//   record.h      k_rec_save: everything the derivative passes read of a solve, gathered into a record in the caller's order
//                 (ltompc_record_save); the passes then run on a Work that points into the record
//   policy.h      k_policy_gather, k_policy_step, k_policy_run: the feedback policy of a solve (ltompc_get_policy, ltompc_policy_step,
//                 ltompc_policy_run_dev): the stage gains K_k, Kv_k of the sensitivity pass's factorisation in the
//                 caller's order (an LDS tile transpose), u = U_k + K_k (x - X_k) + Kv_k (v - V_k) on the iterate and the gains where
//                 they are, and n ticks of that law and d_plant in one launch
//   *_pi          the kernels above that read a vehicle or cost parameter, once more with per-instance values of the 16 of
//                 param_sensitivity.h (ltompc_set_instance_params): the same device functions instantiated with
//                 PI = true, reading the rows through WorkPI (layout.h); the uniform kernels are unchanged
//   *_ts          the kernels above that read a value row of the track tables, a third time with per-instance table sets
//                 (ltompc_set_table_sets): the same device functions instantiated with PI = true and TS = true,
//                 K.T replaced by inst_tables<TS>(K.T, W, b) - the handle's tables with the four value pointers moved to the
//                 rows of the instance's set, read through WorkTS (layout.h).  Thread-per-slot evaluation only; the Riccati
//                 heads and d_pick are among them (lterm(x_0) reads v_ref when the smoothing changes); the sweeps of the
//                 derivative passes read no table and stay the _pi ones; the uniform and _pi kernels are unchanged
#pragma once
#include "layout.h"
#include "linearise.h"
#include "riccati.h"
#include "linesearch.h"
#include "aux_kernels.h"
#include "eval8.h"
#include "velocity.h"
#include "rollout.h"
#include "sensitivity.h"
#include "param_sensitivity.h"
#include "adjoint.h"
#include "jvp.h"
#include "plant_sensitivity.h"
#include "table_sensitivity.h"
#include "table_jvp.h"
#include "warm_state.h"
#include "record.h"
#include "policy.h"
