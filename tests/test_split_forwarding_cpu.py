"""What SplitMPC hands to its parts, without a GPU, on the smallest ragged split (N = 4, B = 8, parts [0,3) [3,6) [6,8)).
(a) The device-pointer forwards on a recording stand-in for the library (the one of test_policy_abi.py, which pins the four policy
forwards): every part's pointer is base + bytes per row * its first row, with the row bytes written out here from the shapes of
include/ltompc.h; int32 arrays advance 4 bytes a row; an array that all parts share keeps its pointer; 0 stays 0; the two summed
table gradients are overwritten by the first part and added to by the later ones, each after the part before it has finished.
(b) The host forwards on stub parts: every part receives its rows (None stays None, shared arguments whole), per-instance results
come back in the caller's order, names are the first part's, and the table gradients are summed in part order, bit for bit."""
import numpy as np
import pytest

from test_policy_abi import fake  # noqa: F401  (the fixture that puts the recording stand-in in the library's place)

N, B = 4, 8
BOUNDS = [(0, 3), (3, 6), (6, 8)]
PARTS = ((1, 0), (2, 3), (3, 6))  # (handle, first row)
P = [100000 * (i + 1) for i in range(7)]  # base pointers: further apart than any array is long

# bytes per instance of the device arrays (include/ltompc.h: NX = 8, NU = 2, NTHETA = 16, NLOOP = 24, 10 look-up slots an interval)
X_ROW, U_ROW = 8 * 8, 8 * 2  # x (B,8), u (B,2)
XS_ROW, US_ROW, CS_ROW = 8 * (N + 1) * 8, 8 * N * 2, 8 * N * 8  # X (B,N+1,8), U (B,N,2), C (B,N,8)
P_ROW, TH_ROW = 8 * (8 + 2), 8 * 16  # (B,10): x0 and u_prev; (B,16): theta
DU0_DP_ROW, DU0_DTH_ROW = 8 * 2 * (8 + 2), 8 * 2 * 16  # (B,2,10), (B,2,16)
SLOT_ROW = 8 * N * 10  # (B,N,10)
PLANT_ROWS = (8 * 8 * 8, 8 * 8 * 2, 8 * 8 * 16)  # (B,8,8), (B,8,2), (B,8,16)
LOOP_ROWS = (8 * 8 * 24, 8 * 2 * 24)  # (B,8,24), (B,2,24)
INT_ROW = 4  # ok, a mask, the set index: (B,) int32

# (method, arguments, entry point, the arguments it receives for a part whose first row is lo)
FORWARDS = [
    ("reset_dev", (P[0], P[1]), "ltompc_reset_instances_dev", lambda lo: (P[0] + INT_ROW * lo, P[1] + X_ROW * lo)),
    ("set_guess_dev", (P[0], P[1], P[2], P[3], P[4]), "ltompc_set_guess_dev",
     lambda lo: (P[0] + INT_ROW * lo, P[1] + XS_ROW * lo, P[2] + CS_ROW * lo, P[3] + US_ROW * lo, P[4] + U_ROW * lo)),
    ("set_guess_dev", (P[0], P[1], P[2], P[3]), "ltompc_set_guess_dev",
     lambda lo: (P[0] + INT_ROW * lo, P[1] + XS_ROW * lo, P[2] + CS_ROW * lo, P[3] + US_ROW * lo, 0)),
    ("set_table_values_dev", ("n_right", P[0]), "ltompc_set_table_values_dev", lambda lo: (2, P[0])),
    ("set_table_sets_dev", (2, P[0], P[1]), "ltompc_set_table_sets_dev", lambda lo: (2, P[0], P[1] + INT_ROW * lo)),
    ("set_table_sets_dev", (2, 0, 0), "ltompc_set_table_sets_dev", lambda lo: (2, 0, 0)),
    ("sensitivities_dev", (P[0], P[1]), "ltompc_sensitivities_dev", lambda lo: (P[0] + DU0_DP_ROW * lo, P[1] + INT_ROW * lo)),
    ("sensitivities_dev", (), "ltompc_sensitivities_dev", lambda lo: (0, 0)),
    ("param_sensitivities_dev", (P[0], P[1]), "ltompc_param_sensitivities_dev", lambda lo: (P[0] + DU0_DTH_ROW * lo, P[1] + INT_ROW * lo)),
    ("param_sensitivities_dev", (), "ltompc_param_sensitivities_dev", lambda lo: (0, 0)),
    ("adjoint_dev", (P[0], P[1], P[2], P[3], P[4]), "ltompc_adjoint_dev",
     lambda lo: (P[0] + XS_ROW * lo, P[1] + US_ROW * lo, P[2] + P_ROW * lo, P[3] + TH_ROW * lo, P[4] + INT_ROW * lo)),
    ("adjoint_dev", (0, 0), "ltompc_adjoint_dev", lambda lo: (0, 0, 0, 0, 0)),
    ("jvp_dev", (P[0], P[1], P[2], P[3], P[4]), "ltompc_jvp_dev",
     lambda lo: (P[0] + P_ROW * lo, P[1] + TH_ROW * lo, P[2] + XS_ROW * lo, P[3] + US_ROW * lo, P[4] + INT_ROW * lo)),
    ("jvp_dev", (0, 0), "ltompc_jvp_dev", lambda lo: (0, 0, 0, 0, 0)),
    ("jvp_tables_dev", (P[0], P[1], P[2], P[3], P[4], P[5]), "ltompc_jvp_tables_dev",
     lambda lo: (P[0] + P_ROW * lo, P[1], P[2] + SLOT_ROW * lo, P[3] + XS_ROW * lo, P[4] + US_ROW * lo, P[5] + INT_ROW * lo)),
    ("jvp_tables_dev", (), "ltompc_jvp_tables_dev", lambda lo: (0, 0, 0, 0, 0, 0)),
    ("jvp_table_sets_dev", (P[0], P[1], P[2], P[3], P[4], P[5]), "ltompc_jvp_table_sets_dev",
     lambda lo: (P[0] + P_ROW * lo, P[1], P[2] + SLOT_ROW * lo, P[3] + XS_ROW * lo, P[4] + US_ROW * lo, P[5] + INT_ROW * lo)),
    ("jvp_table_sets_dev", (), "ltompc_jvp_table_sets_dev", lambda lo: (0, 0, 0, 0, 0, 0)),
    ("set_u_prev_dev", (P[0],), "ltompc_set_u_prev_dev", lambda lo: (P[0] + U_ROW * lo,)),
    ("plant_sensitivities_dev", (P[0], P[1], P[2], P[3], P[4], P[5], 7), "ltompc_plant_sensitivities_dev",
     lambda lo: (P[0] + X_ROW * lo, P[1] + U_ROW * lo, 7, P[2] + X_ROW * lo, P[3] + PLANT_ROWS[0] * lo, P[4] + PLANT_ROWS[1] * lo,
                 P[5] + PLANT_ROWS[2] * lo)),
    ("plant_sensitivities_dev", (P[0], P[1]), "ltompc_plant_sensitivities_dev", lambda lo: (P[0] + X_ROW * lo, P[1] + U_ROW * lo, 400, 0, 0, 0, 0)),
    ("loop_tick_dev", (P[0], P[1], P[2], 9), "ltompc_loop_tick_dev", lambda lo: (P[0] + X_ROW * lo, P[1] + U_ROW * lo, 9, P[2] + X_ROW * lo)),
    ("loop_sensitivities_dev", (P[0], P[1], P[2]), "ltompc_loop_sensitivities_dev",
     lambda lo: (P[0] + LOOP_ROWS[0] * lo, P[1] + LOOP_ROWS[1] * lo, P[2] + INT_ROW * lo)),
    ("loop_sensitivities_dev", (), "ltompc_loop_sensitivities_dev", lambda lo: (0, 0, 0)),
    ("prediction_dev", (P[0], P[1]), "ltompc_get_prediction_dev", lambda lo: (P[0] + XS_ROW * lo, P[1] + US_ROW * lo)),
    ("prediction_dev", (), "ltompc_get_prediction_dev", lambda lo: (0, 0)),
]


@pytest.fixture()
def split(pkg, tables, fake):  # noqa: F811
    s = pkg.SplitMPC(tables, N, B, n_parts=3)
    fake.made.append(s)
    assert s.bounds == BOUNDS
    fake.calls.clear()
    return s


def test_device_forwards_offset_each_array_by_its_row(split, fake):  # noqa: F811
    for method, args, entry, expect in FORWARDS:
        fake.calls.clear()
        getattr(split, method)(*args)
        assert fake.calls == [(entry, h, expect(lo)) for h, lo in PARTS], (method, args)


def test_threaded_device_forwards_offset_each_array_by_its_row(split, fake):  # noqa: F811
    """The forwards that run in the parts' threads: the same rows, in any order across the handles."""
    n = 3  # ticks of the rollout logs: (B,n,2) doubles, (B,n) int32
    for method, args, entry, expect in (
            ("set_initial_guess_dev", (P[0],), "ltompc_set_initial_guess_dev", lambda lo: (P[0] + X_ROW * lo,)),
            ("make_step_dev", (P[0], P[1]), "ltompc_make_step_dev", lambda lo: (P[0] + X_ROW * lo, P[1] + U_ROW * lo)),
            ("rollout_dev", (P[0], n, 5, P[1], P[2], P[3]), "ltompc_rollout_dev",
             lambda lo: (P[0] + X_ROW * lo, n, 5, P[1] + U_ROW * n * lo, P[2] + INT_ROW * n * lo, P[3] + INT_ROW * n * lo)),
            ("rollout_dev", (P[0], n), "ltompc_rollout_dev", lambda lo: (P[0] + X_ROW * lo, n, 400, 0, 0, 0))):
        fake.calls.clear()
        getattr(split, method)(*args)
        assert sorted(c for c in fake.calls if c[0] == entry) == [(entry, h, expect(lo)) for h, lo in PARTS], (method, args)


@pytest.mark.parametrize("method, entry", [("adjoint_tables_dev", "ltompc_adjoint_tables"), ("adjoint_table_sets_dev", "ltompc_adjoint_table_sets")])
def test_summed_device_forwards_add_in_part_order(split, fake, method, entry):  # noqa: F811
    """The gradient's pointer is the same for every part: part 1 overwrites, parts 2 and 3 add, each after the part before it has
    finished; without a gradient nobody waits."""
    def rows(lo):
        return (P[0] + XS_ROW * lo, P[1] + US_ROW * lo, P[2], P[3] + SLOT_ROW * lo, P[4] + INT_ROW * lo)
    getattr(split, method)(P[0], P[1], P[2], P[3], P[4])
    assert fake.calls == [(entry + "_dev", 1, rows(0)), ("ltompc_synchronize", 1, ()), (entry + "_add_dev", 2, rows(3)),
                          ("ltompc_synchronize", 2, ()), (entry + "_add_dev", 3, rows(6))]
    fake.calls.clear()
    getattr(split, method)(0, P[1])
    assert fake.calls == [(entry + ("_add_dev" if h > 1 else "_dev"), h, (0, P[1] + US_ROW * lo, 0, 0, 0)) for h, lo in PARTS]


# ---- (b) host forwards on stub parts
NAMES, SLOT_NAMES = ("the", "first", "part's"), ("slots",)
# what a stub part returns: method -> (keys with one row per instance, keys that are the same for all parts, keys that are summed)
RETURNS = {
    "sensitivities": (("du0_dx0", "du0_duprev", "ok", "margin", "dX", "dU"), {}, ()),
    "param_sensitivities": (("du0_dtheta", "ok", "dX", "dU"), dict(names=NAMES), ()),
    "adjoint": (("grad_x0", "grad_uprev", "ok", "grad_theta"), dict(names=NAMES), ()),
    "adjoint_tables": (("ok", "slot_grad"), dict(names=NAMES, slot_names=SLOT_NAMES), ("grad_tables",)),
    "adjoint_table_sets": (("ok", "slot_grad"), dict(names=NAMES, slot_names=SLOT_NAMES), ("grad_sets",)),
    "jvp": (("tX", "tU", "ok"), {}, ()),
    "jvp_tables": (("tX", "tU", "ok"), {}, ()),
    "jvp_table_sets": (("tX", "tU", "ok"), {}, ()),
    "plant_sensitivities": (("x_next", "dx", "du", "dtheta"), dict(names=NAMES), ()),
    "loop_sensitivities": (("dx", "du", "ok", "ticks"), dict(names=NAMES), ()),
    "loop_tick": None,  # (an array, one row per instance)
    "policy": (("K", "Kv", "ok"), {}, ()),
    "policy_step": None,
    "policy_run": (("u", "x"), {}, ()),
    "stats": (("status", "iters", "kkt"), {}, ()),
    "iterate": (("X", "C", "U", "L1", "L2", "T", "NU"), {}, ()),
}
SUMMANDS = (0.1, 0.2, 0.3)  # ((0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3): the order of the sum shows in the last bit)


def _per_instance(k, lo, hi, j):
    """Rows of part k: 1000 k + the instance's index in the whole batch, + 0.25 j for the j-th key."""
    return (1000.0 * k + np.arange(lo, hi) + 0.25 * j)[:, None] * np.ones((1, 3))


class _Part:
    def __init__(self, k, lo, hi):
        self.k, self.lo, self.hi, self.calls, self.summed = k, lo, hi, [], {}

    def __getattr__(self, method):
        if method not in RETURNS:
            raise AttributeError(method)

        def call(*args):
            self.calls.append((method, args))
            if RETURNS[method] is None:
                return _per_instance(self.k, self.lo, self.hi, 0)
            per, first, summed = RETURNS[method]
            # (parts other than the first return names of their own: the stitched ones must be the first part's)
            out = {key: (v if self.k == 0 else ("part", self.k)) for key, v in first.items()}
            out.update({key: _per_instance(self.k, self.lo, self.hi, j) for j, key in enumerate(per)})
            for key in summed:
                self.summed[key] = out[key] = SUMMANDS[self.k] * (1.0 + np.arange(20.0).reshape(4, 5))
            return out
        return call


@pytest.fixture()
def stubs(pkg):
    s = pkg.SplitMPC.__new__(pkg.SplitMPC)
    s.parts, s.bounds, s.n_table, s.B, s.N = [_Part(k, lo, hi) for k, (lo, hi) in enumerate(BOUNDS)], BOUNDS, 5, B, N
    return s


def _arr(*shape):
    return np.arange(float(np.prod(shape))).reshape(shape) + 0.5


x, u = _arr(B, 8), _arr(B, 2)
gX, gU = _arr(B, N + 1, 8), _arr(B, N, 2)
dp, dth, dslot = _arr(B, 10), _arr(B, 16), _arr(B, N, 10)
dtab, dsets = _arr(4, 5), _arr(2, 4, 5)
# (method, arguments, which of them are split by rows; the others reach every part as they are)
HOST = [
    ("sensitivities", (True,), ()), ("param_sensitivities", (True,), ()),
    ("adjoint", (gX, None, False), (0, 1)), ("adjoint", (None, gU, True), (0, 1)), ("adjoint", (gX.tolist(), gU, True), (0, 1)),
    ("adjoint_tables", (gX, gU, True), (0, 1)), ("adjoint_tables", (None, gU, False), (0, 1)),
    ("adjoint_table_sets", (gX, gU, True), (0, 1)), ("adjoint_table_sets", (gX, None, False), (0, 1)),
    ("jvp", (dp, None), (0, 1)), ("jvp", (None, dth), (0, 1)),
    ("jvp_tables", (dp, dtab, None), (0, 2)), ("jvp_tables", (None, None, dslot), (0, 2)),
    ("jvp_table_sets", (None, dsets, dslot), (0, 2)), ("jvp_table_sets", (dp, dsets, None), (0, 2)),
    ("plant_sensitivities", (x, u, 7, False), (0, 1)), ("loop_sensitivities", (), ()), ("loop_tick", (x, u, 9), (0, 1)),
    ("policy", (), ()), ("policy_step", (2, x, None, True), (1, 2)), ("policy_step", (1, x, u, False), (1, 2)),
    ("policy_run", (1, 2, x, u, 5, True), (2, 3)), ("policy_run", (0, 1, x, None, 5, False), (2, 3)),
    ("stats", (), ()), ("iterate", (), ()),
]


@pytest.mark.parametrize("method, args, by_rows", HOST, ids=[f"{m}-{i}" for i, (m, _, _) in enumerate(HOST)])
def test_host_forwards_slice_the_inputs_and_stitch_the_results(stubs, method, args, by_rows):
    out = getattr(stubs, method)(*args)
    for p in stubs.parts:
        (name, got), = p.calls
        assert name == method and len(got) == len(args)
        for i, (g, a) in enumerate(zip(got, args)):
            if a is None:
                assert g is None
            elif i in by_rows:
                assert np.array_equal(g, np.asarray(a)[p.lo:p.hi]) and g.dtype == np.float64
            else:
                assert g is a  # (shared: whole, and not copied)
    if RETURNS[method] is None:
        assert np.array_equal(out, np.concatenate([_per_instance(k, lo, hi, 0) for k, (lo, hi) in enumerate(BOUNDS)]))
        return
    per, first, summed = RETURNS[method]
    assert set(out) == set(per) | set(first) | set(summed)
    for j, key in enumerate(per):
        assert np.array_equal(out[key], np.concatenate([_per_instance(k, lo, hi, j) for k, (lo, hi) in enumerate(BOUNDS)])), key
    for key, v in first.items():
        assert out[key] is v
    for key in summed:
        g0, g1, g2 = (p.summed[key] for p in stubs.parts)
        assert np.array_equal(out[key], (g0 + g1) + g2) and not np.array_equal(out[key], g0 + (g1 + g2))
        assert out[key] is not g0 and np.array_equal(g0, SUMMANDS[0] * (1.0 + np.arange(20.0).reshape(4, 5)))  # (part 0's is untouched)
