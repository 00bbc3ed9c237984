"""ctypes binding of libltompc.so (include/ltompc.h).  No CPU fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._build import LIB

NX, NU = 8, 2
# columns of ltompc_get_param_sensitivities (LTOMPC_NTHETA, include/ltompc.h): the ltompc_params fields, in this order
THETA_NAMES = ("mass", "inertia_z", "B_f", "C_f", "D_f", "B_r", "C_r", "D_r", "C_m", "Cr_0", "Cr_2", "q_n", "q_mu", "q_B",
               "r_du[0]", "r_du[1]")
NTHETA = len(THETA_NAMES)
# columns of ltompc_get_loop_sensitivities (LTOMPC_NLOOP): the initial state, then theta
LOOP_NAMES = tuple(f"x_init[{i}]" for i in range(8)) + THETA_NAMES
NLOOP = len(LOOP_NAMES)
# rows of ltompc_set_table_values and of grad_tables (LTOMPC_TABLE_VALUE_ROWS): the value rows of the look-up tables, in this order
TABLE_ROW_NAMES = ("kappa", "n_left", "n_right", "v_ref")
# the ten scalars of slot_grad (ltompc_get_adjoint_tables): value and slope (') of kappa at c_k and at x_{k+1}, of the others at x_{k+1}
TABLE_SLOT_NAMES = ("kappa_c", "kappa_c'", "kappa_x", "kappa_x'", "n_left", "n_left'", "n_right", "n_right'", "v_ref", "v_ref'")
NO_BOUND = 1.0e30
STATUS_NAMES = {0: "solved", 1: "acceptable", 2: "max_iter", 3: "numerical", 4: "stalled", 5: "infeasible"}


class Params(C.Structure):
    """ltompc_params (include/ltompc.h)."""
    _fields_ = [(n, C.c_double) for n in (
        "mass", "inertia_z", "length_f", "length_r", "width", "B_f", "C_f", "D_f", "B_r", "C_r", "D_r",
        "C_m", "Cr_0", "Cr_2", "gravity", "ptv", "q_n", "q_mu", "q_vy", "q_v", "vref_scale", "q_B")] + [
        ("r_du", C.c_double * 2), ("x_lb", C.c_double * 8), ("x_ub", C.c_double * 8),
        ("u_lb", C.c_double * 2), ("u_ub", C.c_double * 2)] + [
        (n, C.c_double) for n in ("ell_penalty", "ell_rho", "ell_D_f", "ell_D_r")]


class Options(C.Structure):
    """ltompc_options (include/ltompc.h)."""
    _fields_ = [(n, C.c_double) for n in (
        "t_step", "tol", "acceptable_tol", "mu_init", "mu_min", "kappa_eps", "kappa_mu", "theta_mu", "tau_min",
        "bound_push", "s_max", "delta_w_first", "smooth_eps_min", "smooth_scale", "mu_init_warm", "soft_rho", "resto_rho",
        "resto_rho_max", "resto_rho_factor", "dual_inf_max")] + [
        ("max_iter", C.c_int), ("acceptable_iter", C.c_int), ("n_linesearch", C.c_int), ("stall_iter", C.c_int),
        ("max_ls_fail", C.c_int), ("warm_shift", C.c_int), ("warm_reset_on_fail", C.c_int), ("periodic_tables", C.c_int), ("max_soc", C.c_int), ("resto_sticky", C.c_int),
        ("node0_check", C.c_int), ("warm_fallback_iter", C.c_int), ("resto_shift_retry", C.c_int), ("max_mu_stay", C.c_int), ("infeasible_sticky", C.c_int), ("latency_mode", C.c_int)]


class LtompcError(RuntimeError):
    pass


_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def lib() -> C.CDLL:
    """Load libltompc.so; raise if it has not been built (there is deliberately no other compute path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise LtompcError(
                f"{LIB} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own HIP runtime; libltompc.so links the system one.  In one process the first one loaded
        # serves both, and it has to be torch's: with the system runtime initialised first (a handle created before `import torch`)
        # torch finds no devices ("No HIP GPUs are available", measured on the MI355X box).  So torch is imported here when it is
        # installed; without torch the library runs on the system runtime alone.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB)
        L.ltompc_last_error.restype = C.c_char_p
        L.ltompc_version.restype = C.c_char_p
        L.ltompc_get_param_sensitivities.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
        L.ltompc_param_sensitivities_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_get_adjoint.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _ip]
        L.ltompc_adjoint_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_get_adjoint_tables.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _ip]
        L.ltompc_adjoint_tables_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_adjoint_tables_add_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_get_prediction_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_get_jvp.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _ip]
        L.ltompc_jvp_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("ltompc_get_jvp_tables", "ltompc_get_jvp_table_sets"):
            getattr(L, name).argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _ip]
        for name in ("ltompc_jvp_tables_dev", "ltompc_jvp_table_sets_dev"):
            getattr(L, name).argtypes = [C.c_void_p] * 7
        L.ltompc_set_u_prev.argtypes = [C.c_void_p, _dp]
        L.ltompc_set_u_prev_dev.argtypes = [C.c_void_p, C.c_void_p]
        L.ltompc_set_table_values.argtypes = [C.c_void_p, C.c_int, _dp]
        L.ltompc_set_table_values_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ltompc_get_table_values.argtypes = [C.c_void_p, C.c_int, _dp]
        L.ltompc_set_table_sets.argtypes = [C.c_void_p, C.c_int, _dp, _ip]
        L.ltompc_set_table_sets_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ltompc_get_table_sets.argtypes = [C.c_void_p, _ip, _dp, _ip]
        L.ltompc_get_adjoint_table_sets.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _ip]
        L.ltompc_adjoint_table_sets_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_adjoint_table_sets_add_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_set_instance_params.argtypes = [C.c_void_p, _dp]
        L.ltompc_set_instance_params_dev.argtypes = [C.c_void_p, C.c_void_p]
        L.ltompc_get_instance_params.argtypes = [C.c_void_p, _dp]
        L.ltompc_plant_sensitivities.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]
        L.ltompc_plant_sensitivities_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_loop_begin.argtypes = [C.c_void_p, C.c_int]
        L.ltompc_loop_tick_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ltompc_loop_tick.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _dp]
        L.ltompc_get_loop_sensitivities.argtypes = [C.c_void_p, _dp, _dp, _ip, _ip]
        L.ltompc_loop_sensitivities_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_loop_end.argtypes = [C.c_void_p]
        L.ltompc_reset_instances.argtypes = [C.c_void_p, _ip, _dp]
        L.ltompc_reset_instances_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_set_guess.argtypes = [C.c_void_p, _ip, _dp, _dp, _dp, _dp]
        L.ltompc_set_guess_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_warm_state_size.argtypes = [C.c_void_p]
        L.ltompc_export_state.argtypes = [C.c_void_p, _ip, C.c_int, _dp]
        L.ltompc_export_state_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ltompc_import_state.argtypes = [C.c_void_p, _ip, C.c_int, _dp]
        L.ltompc_import_state_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ltompc_record_size.argtypes = [C.c_void_p]
        L.ltompc_record_size.restype = C.c_longlong
        L.ltompc_record_save.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.ltompc_record_select.argtypes = [C.c_void_p, C.c_void_p]
        L.ltompc_record_release.argtypes = [C.c_void_p, C.c_void_p]
        L.ltompc_record_trim.argtypes = [C.c_void_p]
        L.ltompc_record_stats.argtypes = [C.c_void_p, _ip, _ip]
        L.ltompc_get_policy.argtypes = [C.c_void_p, _dp, _dp, _ip]
        L.ltompc_policy_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ltompc_policy_step.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp]
        L.ltompc_policy_step_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ltompc_policy_run_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.ltompc_policy_last_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        raise LtompcError(lib().ltompc_last_error().decode())


def dptr(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def iptr(a: np.ndarray):
    return a.ctypes.data_as(_ip)


def default_params() -> Params:
    p = Params()
    lib().ltompc_default_params(C.byref(p))
    return p


def default_options() -> Options:
    o = Options()
    lib().ltompc_default_options(C.byref(o))
    return o
