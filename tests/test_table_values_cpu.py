"""Settable table values without a GPU: the entry points exist and refuse a null handle with an error code; the binding checks
the row, the shape and the values before any call; SplitMPC checks once and hands the same set to every part."""
import importlib

import numpy as np
import pytest


def test_entry_points_refuse_a_null_handle(gpu_lib):
    for f in (gpu_lib.ltompc_set_table_values, gpu_lib.ltompc_set_table_values_dev, gpu_lib.ltompc_get_table_values):
        assert f(None, 0, None) == -1
        assert b"null" in gpu_lib.ltompc_last_error()


def test_row_and_values_are_checked_before_any_call(pkg):
    S = importlib.import_module("lap-time-optimization_amd.solver")
    assert pkg.TABLE_ROW_NAMES == ("kappa", "n_left", "n_right", "v_ref")
    assert [S._table_row(n) for n in pkg.TABLE_ROW_NAMES] == [0, 1, 2, 3] and S._table_row(2) == 2
    for bad, what in (("s_arc", "unknown row"), (4, "row must be"), (-1, "row must be")):
        with pytest.raises(ValueError, match=what):
            S._table_row(bad)
    v = np.arange(6.0)
    out = S._table_values(v, 6)
    assert out.dtype == np.float64 and out.flags.c_contiguous and np.array_equal(out, v) and out is not v
    assert np.array_equal(S._table_values(list(range(6)), 6), v)
    with pytest.raises(ValueError, match=r"shape \(7,\)"):
        S._table_values(v, 7)
    v[4] = np.nan
    with pytest.raises(ValueError, match="knot 4"):
        S._table_values(v, 6)


class _Part:
    def __init__(self, n):
        self._tab = np.zeros((6, n))
        self.sets = []

    def set_table_values(self, row, values):
        self.sets.append((row, np.array(values)))

    def set_table_values_dev(self, row, ptr):
        self.sets.append((row, ptr))

    def table_values(self):
        return "rows of part 0"


def test_split_mpc_checks_once_and_sets_every_part(pkg):
    split = pkg.SplitMPC.__new__(pkg.SplitMPC)
    split.parts, split.n_table = [_Part(5), _Part(5), _Part(5)], 5
    with pytest.raises(ValueError, match="shape"):
        split.set_table_values("v_ref", np.ones(4))
    with pytest.raises(ValueError, match="unknown row"):
        split.set_table_values_dev("width", 1024)
    assert all(p.sets == [] for p in split.parts)
    split.set_table_values("n_right", np.arange(5.0))
    split.set_table_values_dev("v_ref", 1024)
    for p in split.parts:
        assert p.sets[0][0] == 2 and np.array_equal(p.sets[0][1], np.arange(5.0)) and p.sets[1] == (3, 1024)
    assert split.table_values() == "rows of part 0"


def test_adjoint_tables_entry_points_refuse_a_null_handle(gpu_lib):
    for f in (gpu_lib.ltompc_get_adjoint_tables, gpu_lib.ltompc_adjoint_tables_dev):
        assert f(None, None, None, None, None, None) == -1
        assert b"null" in gpu_lib.ltompc_last_error()


def test_adjoint_tables_checks_shapes_before_any_call(pkg):
    """BatchedMPC.adjoint_tables refuses cotangents of the wrong shape in the binding; SplitMPC sums grad_tables over its
    parts in part order and stitches slot_grad and ok."""
    mpc = pkg.BatchedMPC.__new__(pkg.BatchedMPC)
    mpc.B, mpc.N, mpc._tab, mpc._h = 3, 4, np.zeros((6, 5)), None
    with pytest.raises(ValueError, match=r"gX must have shape \(3, 5, 8\)"):
        mpc.adjoint_tables(np.zeros((3, 4, 8)))
    with pytest.raises(ValueError, match=r"gU must have shape \(3, 4, 2\)"):
        mpc.adjoint_tables(None, np.zeros((3, 4, 3)))

    class Part:
        def __init__(self, k, n):
            self.k, self.n, self._tab = k, n, np.zeros((6, 5))

        def adjoint_tables(self, gX, gU, slots):
            assert gX.shape[0] == self.n and gU is None
            out = dict(grad_tables=np.full((4, 5), 10.0 ** self.k), names=pkg.TABLE_ROW_NAMES, ok=np.full(self.n, self.k % 2 == 0))
            if slots:
                out.update(slot_grad=np.full((self.n, 4, 10), float(self.k)), slot_names=pkg.TABLE_SLOT_NAMES)
            return out

    split = pkg.SplitMPC.__new__(pkg.SplitMPC)
    split.parts, split.bounds = [Part(0, 2), Part(1, 2), Part(2, 1)], [(0, 2), (2, 4), (4, 5)]
    r = split.adjoint_tables(np.zeros((5, 5, 8)), slots=True)
    assert (r["grad_tables"] == 111.0).all() and r["ok"].tolist() == [True, True, False, False, True]
    assert r["slot_grad"][:, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0, 2.0] and r["names"] == pkg.TABLE_ROW_NAMES
    assert "slot_grad" not in split.adjoint_tables(np.zeros((5, 5, 8)))
