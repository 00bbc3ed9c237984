"""C ABI and Python surface of the per-instance vehicle and cost parameters without a GPU (ltompc_set_instance_params,
include/ltompc.h): the entry points are declared and exported and reject a null handle; the Python layer
rejects bad shapes, names and values before any call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ENTRY = ("ltompc_set_instance_params", "ltompc_set_instance_params_dev", "ltompc_get_instance_params")


def test_entry_points_are_declared():
    src = open(os.path.join(ROOT, "include", "ltompc.h")).read()
    for name in ENTRY:
        assert re.search(r"\bint " + name + r"\(ltompc_handle h, (const )?double\* theta(_dev)?\);", src), name


def test_entry_points_are_exported_and_reject_a_null_handle(gpu_lib):
    for name in ENTRY:
        assert hasattr(gpu_lib, name), name
    t = (C.c_double * 16)()
    assert gpu_lib.ltompc_set_instance_params(None, t) < 0
    assert b"null handle" in gpu_lib.ltompc_last_error()
    assert gpu_lib.ltompc_set_instance_params_dev(None, None) < 0
    assert gpu_lib.ltompc_get_instance_params(None, t) < 0


@pytest.fixture(scope="module")
def rows_of():
    S = importlib.import_module("lap-time-optimization_amd.solver")
    L = importlib.import_module("lap-time-optimization_amd._lib")
    p = L.default_params()
    base = np.array([getattr(p, n) for n in L.THETA_NAMES[:-2]] + [p.r_du[0], p.r_du[1]])
    return lambda theta, B=4: S._theta_rows(theta, B, base), base, L.THETA_NAMES


def test_python_builds_and_checks_the_rows(rows_of):
    f, base, names = rows_of
    r = f({"D_f": np.array([0.9, 1.0, 1.1, 1.2]), "mass": 1200.0})
    assert r.shape == (4, 16) and r.flags.c_contiguous
    assert np.array_equal(r[:, names.index("D_f")], [0.9, 1.0, 1.1, 1.2]) and (r[:, 0] == 1200.0).all()
    keep = [j for j in range(16) if names[j] not in ("D_f", "mass")]
    assert np.array_equal(r[:, keep], np.tile(base[keep], (4, 1)))
    assert np.array_equal(f(np.tile(base, (4, 1))), np.tile(base, (4, 1)))
    bad = [np.zeros((4, 15)), np.zeros((3, 16)), {"grip": 1.0}, {"D_f": np.ones(5)}, {"mass": 0.0}, {"inertia_z": -1.0},
           {"q_n": -1e-3}, {"r_du[1]": -1.0}, {"C_f": np.nan}, {"B_r": np.inf}]
    for theta in bad:
        with pytest.raises(ValueError):
            f(theta)
    t = np.tile(base, (4, 1))
    t[2, 5] = np.nan
    with pytest.raises(ValueError, match=r"row 2, B_r"):
        f(t)
    assert (f({"q_n": 0.0})[:, names.index("q_n")] == 0.0).all()  # (a zero weight is allowed)


def test_python_rows_are_a_copy(rows_of):
    """The rows kept for feedback(theta=...) do not alias the caller's array: refilling it for the next tick changes nothing."""
    f, base, names = rows_of
    t = np.ascontiguousarray(np.tile(base, (4, 1)))
    r = f(t)
    assert not np.shares_memory(r, t)
    t[:, 0] = 1.0
    assert (r[:, 0] == base[0]).all()
    v = np.full(4, 0.9)
    r = f({"D_f": v})
    v[:] = 2.0
    assert (r[:, names.index("D_f")] == 0.9).all()
