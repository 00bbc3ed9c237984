"""Independent float64 reference of the plant step's sensitivities: the discrete RK4 map of the plant
(n_sub classical RK4 sub-steps under zero-order-hold u, the curvature table exact, eps = 0) restated in torch with the 16
parameters theta as a tensor, and differentiated by reverse-mode autograd through all 4 n_sub stage evaluations.  The
expressions are those of nlp_reference.rhs; neither the kernels' hand-derived Jacobian nor theta_jet is used.
tests/test_plant_sens_reference.py pins it against the CPU oracle."""
from __future__ import annotations

import numpy as np
import torch

import nlp_reference as R
import param_sens_reference as PR

NT = PR.NT


def rhs(x, u, th, tab):
    """nlp_reference.rhs at eps = 0 with theta (.., 16) in PR.NAMES order in place of the constants."""
    s, n, mu, vx, vy, r, de, thr = x.unbind(-1)
    m, Iz, Bf, Cf, Df, Br, Cr, Dr, Cm, Cr0, Cr2 = (th[..., j] for j in range(11))
    lf, lr, g = R.P["lf"], R.P["lr"], R.P["g"]
    kap = R.lut(tab.s_kappa, tab.kappa, s, 0.0)
    sdot = (vx * torch.cos(mu) - vy * torch.sin(mu)) / (1 - n * kap)
    af = torch.atan2(vy + lf * r, vx) - de
    ar = torch.atan2(vy - lr * r, vx)
    L = lf + lr
    Fnf, Fnr = lr * m * g / L, lf * m * g / L
    Fyf = -Fnf * Df * torch.sin(Cf * torch.atan(Bf * af))
    Fyr = -Fnr * Dr * torch.sin(Cr * torch.atan(Br * ar))
    Fx = Cm * thr - Cr0 - Cr2 * vx * vx
    return torch.stack([
        sdot, vx * torch.sin(mu) + vy * torch.cos(mu), r - kap * sdot,
        (Fx - Fyf * torch.sin(de) + m * vy * r) / m,
        (Fyr + Fyf * torch.cos(de) - m * vx * r) / m,
        (Fyf * lf * torch.cos(de) - Fyr * lr) / Iz,
        u[..., 0] + 0 * s, u[..., 1] + 0 * s], dim=-1)


def rk4(x, u, th, tab, dt, n_sub):
    """The plant's map (aux_kernels.h d_plant / the oracle's plant_step), same order of the sums."""
    y, hs = x, dt / n_sub
    for _ in range(n_sub):
        k1 = rhs(y, u, th, tab)
        k2 = rhs(y + 0.5 * hs * k1, u, th, tab)
        k3 = rhs(y + 0.5 * hs * k2, u, th, tab)
        k4 = rhs(y + hs * k3, u, th, tab)
        y = y + hs / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return y


def plant_sensitivities(x, u, tab, theta=None, dt=0.1, n_sub=400):
    """x (B,8), u (B,2), theta None (nlp_reference's P), (16,) or (B,16)  ->  dict x_next (B,8), dx (B,8,8), du (B,8,2),
    dtheta (B,8,16): the Jacobian of rk4.  The instances are independent, so row i of every instance's Jacobian comes from one
    cotangent e_i on all of them."""
    x = torch.tensor(np.asarray(x, float).reshape(-1, 8), requires_grad=True)
    B = x.shape[0]
    u = torch.tensor(np.asarray(u, float).reshape(B, 2), requires_grad=True)
    th = PR.theta_values() if theta is None else np.asarray(theta, float)
    th = torch.tensor(np.broadcast_to(th, (B, NT)).copy(), requires_grad=True)
    xn = rk4(x, u, th, tab, dt, n_sub)
    # one batched backward pass for the 8 rows: cotangent i is e_i for every instance
    G = torch.zeros(8, B, 8)
    for i in range(8):
        G[i, :, i] = 1.0
    gx, gu, gt = torch.autograd.grad(xn, (x, u, th), grad_outputs=G, is_grads_batched=True)
    return dict(x_next=xn.detach().numpy(), dx=gx.permute(1, 0, 2).numpy().copy(), du=gu.permute(1, 0, 2).numpy().copy(),
                dtheta=gt.permute(1, 0, 2).numpy().copy())
