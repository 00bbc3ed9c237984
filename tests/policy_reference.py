"""Reference for the stage gains of the feedback policy (ltompc_get_policy) without truncation error.  K_k and Kv_k
are the derivatives of the first control of the barrier problem of the tail (nodes k .. N) w.r.t. its initial state x_k and its
previous input u_{k-1}: sens_reference's implicit-function system on the stage slices [k:], where stage k plays stage 0 and
its du0 (2,10) is [K_k | Kv_k].  The stage blocks (the torch restatement of the NLP, differentiated) are taken ONCE per batch;
every (instance, k) is then one sparse LU with refinement."""
from __future__ import annotations

import numpy as np

import sens_reference as SR


def gains_batch(it, x0, uprev, tab, eps, params, ks, refine=3, h=0.1):
    """For each of M instances (arrays as sens_reference.sensitivities_batch takes them) a dict k -> sens_reference._solve's
    result on the slice [k:] (du0 = [K_k | Kv_k], backward, gap, lam_min, ...)."""
    SR.check_params(params)
    blk = SR.stage_blocks(it, x0, uprev, tab, eps, params, h)
    out = []
    for m in range(blk["H"].shape[0]):
        T, NU = np.asarray(it["T"][m], float), np.asarray(it["NU"][m], float)
        out.append({k: SR._solve(blk["H"][m][k:], blk["JG"][m][k:], blk["Jnl"][m][k:], T[k:], NU[k:], params, refine) for k in ks})
    return out
