"""Forward mode in the `tables` input of the autograd layer (lap-time-optimization_amd/autograd.py) without a GPU.
A stand-in handle of this file's own implements the `_dev` methods the layer calls on CPU tensors, through ctypes views of the
pointers it is given.  Its "solve" is a fixed smooth map of (x0, u_prev, theta, tables) with a known Jacobian, so
torch.autograd.gradcheck - reverse and forward mode, `tables` among the inputs - checks the plumbing alone: a tangent in `tables`
goes, in a solve made with forward_tables=True, to jvp_tables_dev together with the tangents of x0 and u_prev (one sweep; without
the switch it raises, as before), theta's tangent goes to jvp_dev and is added,
without a table tangent the call is jvp_dev's as before, and an instance with ok = 0 gets zeros."""
import ctypes as C
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

B, N, NT = 3, 2, 5
NP, NTH, NXO, NUO = 10, 16, (N + 1) * 8, N * 2
NIN = NP + NTH + 4 * NT


def _view(ptr, *shape, dtype=C.c_double):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array((dtype * n).from_address(ptr)).reshape(shape)


class StandIn:
    """(X, U) = tanh(M [x0, u_prev, theta, tables] / 4) per instance (the tables shared), u0 = U[:, 0].  bad_last: ok = 0 for the
    last instance, whose derivatives are then 0 (the C contract)."""
    device = "cpu"
    n_table = NT

    def __init__(self, bad_last=False):
        rng = np.random.default_rng(11)
        self.B, self.N = B, N
        self.M = rng.standard_normal((NXO + NUO, NIN))
        self.theta = np.tile(rng.uniform(0.5, 1.5, NTH), (B, 1))
        self.uprev, self.tab = np.zeros((B, 2)), np.zeros((4, NT))
        self.ok = np.ones(B, dtype=np.int32)
        if bad_last:
            self.ok[-1] = 0
        self.solve_count, self.calls = 0, []

    def set_table_values_dev(self, row, ptr):
        self.tab[row] = _view(ptr, NT)
        self.solve_count += 1

    def set_theta_dev(self, ptr):
        self.theta = _view(ptr, B, NTH).copy()

    def set_u_prev_dev(self, ptr):
        self.uprev = _view(ptr, B, 2).copy()

    def make_step_dev(self, x0_ptr, u0_ptr):
        self.solve_count += 1
        z = np.concatenate([_view(x0_ptr, B, 8), self.uprev, self.theta, np.tile(self.tab.ravel(), (B, 1))], axis=1)
        y = np.tanh(z @ self.M.T / 4)
        self.J = (1 - y ** 2)[:, :, None] * self.M[None] / 4 * self.ok[:, None, None]  # (B, outputs, NIN)
        self.X, self.U = y[:, :NXO].reshape(B, N + 1, 8), y[:, NXO:].reshape(B, N, 2)
        _view(u0_ptr, B, 2)[:] = self.U[:, 0]
        self.uprev = self.U[:, 0].copy()

    def prediction_dev(self, X_ptr=0, U_ptr=0):
        _view(X_ptr, B, N + 1, 8)[:] = self.X
        _view(U_ptr, B, N, 2)[:] = self.U

    def sensitivities_dev(self, du0_ptr=0, ok_ptr=0):
        _view(ok_ptr, B, dtype=C.c_int32)[:] = self.ok

    def _put(self, v, tX_ptr, tU_ptr):
        t = np.einsum("bej,bj->be", self.J, v)
        _view(tX_ptr, B, N + 1, 8)[:] = t[:, :NXO].reshape(B, N + 1, 8)
        _view(tU_ptr, B, N, 2)[:] = t[:, NXO:].reshape(B, N, 2)

    def adjoint_dev(self, gX_ptr, gU_ptr, gp_ptr=0, gth_ptr=0, ok_ptr=0):
        g = np.concatenate([_view(gX_ptr, B, N + 1, 8).reshape(B, -1), _view(gU_ptr, B, N, 2).reshape(B, -1)], axis=1)
        grad = np.einsum("be,bej->bj", g, self.J)
        _view(gp_ptr, B, NP)[:] = grad[:, :NP]
        if gth_ptr:
            _view(gth_ptr, B, NTH)[:] = grad[:, NP:NP + NTH]

    def adjoint_tables_dev(self, gX_ptr, gU_ptr, gt_ptr=0, sg_ptr=0, ok_ptr=0):
        g = np.concatenate([_view(gX_ptr, B, N + 1, 8).reshape(B, -1), _view(gU_ptr, B, N, 2).reshape(B, -1)], axis=1)
        _view(gt_ptr, 4, NT)[:] = np.einsum("be,bej->j", g, self.J[:, :, NP + NTH:]).reshape(4, NT)

    def jvp_dev(self, dp_ptr, dth_ptr, tX_ptr=0, tU_ptr=0, ok_ptr=0):
        self.calls.append(("jvp_dev", bool(dp_ptr), bool(dth_ptr)))
        v = np.zeros((B, NIN))
        if dp_ptr:
            v[:, :NP] = _view(dp_ptr, B, NP)
        if dth_ptr:
            v[:, NP:NP + NTH] = _view(dth_ptr, B, NTH)
        self._put(v, tX_ptr, tU_ptr)

    def jvp_tables_dev(self, dp_ptr=0, dtables_ptr=0, dslot_ptr=0, tX_ptr=0, tU_ptr=0, ok_ptr=0):
        self.calls.append(("jvp_tables_dev", bool(dp_ptr), bool(dtables_ptr), bool(dslot_ptr)))
        v = np.zeros((B, NIN))
        if dp_ptr:
            v[:, :NP] = _view(dp_ptr, B, NP)
        v[:, NP + NTH:] = _view(dtables_ptr, 4 * NT)[None]
        self._put(v, tX_ptr, tU_ptr)

    def synchronize(self):
        pass


@pytest.fixture(scope="module")
def layer():
    return importlib.import_module("lap-time-optimization_amd.autograd")


def _inputs(seed=0, grad=True):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 8, dtype=torch.float64, generator=g)
    up = torch.randn(B, 2, dtype=torch.float64, generator=g)
    th = torch.rand(B, NTH, dtype=torch.float64, generator=g) + 0.5
    tab = torch.randn(4, NT, dtype=torch.float64, generator=g)
    return tuple(t.requires_grad_(grad) for t in (x0, up, th, tab))


def test_gradcheck_of_the_tables_in_reverse_and_forward_mode(layer):
    # (a fresh handle per evaluation: gradcheck differentiates its first evaluation after many others)
    fn = lambda x0, up, th, tab: layer.mpc_solve(StandIn(), x0, up, th, tab, forward_tables=True)[:3]
    assert torch.autograd.gradcheck(fn, _inputs(), check_forward_ad=True)
    fn = lambda x0, tab: layer.mpc_solve(StandIn(), x0, tables=tab, forward_tables=True)[:3]
    x0, _, _, tab = _inputs(1)
    assert torch.autograd.gradcheck(fn, (x0, tab), check_forward_ad=True)


def test_which_pass_gets_which_tangent(layer):
    import torch.autograd.forward_ad as fwAD
    x0, up, th, tab = _inputs(2, grad=False)
    one = torch.ones_like
    with fwAD.dual_level():
        # tables alone (torch hands a zero tangent for x0, which travels as dp): jvp_tables_dev; the tangent is J_y dy and that of u0 is tU[:, 0]; ok = 0 gives zeros
        m = StandIn(bad_last=True)
        u0, X, U, _ = layer.mpc_solve(m, x0, tables=fwAD.make_dual(tab, one(tab)), forward_tables=True)
        assert [(c[0], c[2], c[3]) for c in m.calls] == [("jvp_tables_dev", True, False)]
        want = np.einsum("bej,j->be", m.J[:, :, NP + NTH:], np.ones(4 * NT))
        tX, tU, tu0 = (fwAD.unpack_dual(t).tangent.numpy() for t in (X, U, u0))
        assert np.allclose(tX.reshape(B, -1), want[:, :NXO], rtol=0, atol=1e-14) and np.allclose(tU.reshape(B, -1), want[:, NXO:], rtol=0, atol=1e-14)
        assert np.array_equal(tu0, tU[:, 0]) and (tX[-1] == 0).all() and (tU[-1] == 0).all() and np.abs(tU[:-1]).min() > 0
        # x0 and tables: ONE call with dp; theta too: its part from jvp_dev without dp, added
        m = StandIn()
        layer.mpc_solve(m, fwAD.make_dual(x0, one(x0)), tables=fwAD.make_dual(tab, one(tab)), forward_tables=True)
        assert m.calls == [("jvp_tables_dev", True, True, False)]
        m = StandIn()
        X = layer.mpc_solve(m, fwAD.make_dual(x0, one(x0)), up, fwAD.make_dual(th, one(th)), fwAD.make_dual(tab, one(tab)), forward_tables=True)[1]
        assert m.calls == [("jvp_tables_dev", True, True, False), ("jvp_dev", False, True)]
        v = np.ones((B, NIN))
        v[:, 8:10] = 0.0
        assert np.allclose(fwAD.unpack_dual(X).tangent.numpy().reshape(B, -1), np.einsum("bej,bj->be", m.J, v)[:, :NXO], rtol=0, atol=1e-14)
        # no tangent in the tables (none, or tables not given): jvp_dev as before
        m = StandIn()
        layer.mpc_solve(m, fwAD.make_dual(x0, one(x0)), tables=tab)
        assert m.calls == [("jvp_dev", True, False)]
        m = StandIn()
        layer.mpc_solve(m, fwAD.make_dual(x0, one(x0)))
        assert m.calls == [("jvp_dev", True, False)]
        # the pass is an opt-in of the solve: without forward_tables=True a tangent in the tables raises as it always did
        with pytest.raises(RuntimeError, match="forward mode is not available for `tables`"):
            layer.mpc_solve(StandIn(), x0, tables=fwAD.make_dual(tab, one(tab)))
