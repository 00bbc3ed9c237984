"""C ABI of the solve records without a GPU (ltompc_record_*, include/ltompc.h): the entry points are declared,
bound with their ctypes signatures, exported, and reject a null handle."""
import ctypes as C
import importlib
import os
import re

from conftest import ROOT

DECLS = {
    "ltompc_record_size": ("long long", r"ltompc_handle h"),
    "ltompc_record_save": ("int", r"ltompc_handle h, ltompc_record\* rec"),
    "ltompc_record_select": ("int", r"ltompc_handle h, ltompc_record rec"),
    "ltompc_record_release": ("int", r"ltompc_handle h, ltompc_record rec"),
    "ltompc_record_trim": ("int", r"ltompc_handle h"),
    "ltompc_record_stats": ("int", r"ltompc_handle h, int\* in_use, int\* free_"),
}


def test_entry_points_are_declared():
    src = open(os.path.join(ROOT, "include", "ltompc.h")).read()
    assert re.search(r"typedef struct ltompc_record_s\* ltompc_record;", src)
    for name, (ret, args) in DECLS.items():
        assert re.search(r"\b" + ret + " " + name + r"\(" + args + r"\);", src), name


def test_entry_points_are_exported_with_signatures_and_reject_a_null_handle(gpu_lib):
    L = importlib.import_module("lap-time-optimization_amd._lib")
    ip, vp = L._ip, C.c_void_p
    sig = {"ltompc_record_size": [vp], "ltompc_record_save": [vp, C.POINTER(vp)], "ltompc_record_select": [vp, vp],
           "ltompc_record_release": [vp, vp], "ltompc_record_trim": [vp], "ltompc_record_stats": [vp, ip, ip]}
    for name, argtypes in sig.items():
        assert hasattr(gpu_lib, name), name
        assert list(getattr(gpu_lib, name).argtypes) == argtypes, name
    assert gpu_lib.ltompc_record_size.restype is C.c_longlong
    rec, a, b = vp(), C.c_int(), C.c_int()
    for call in (lambda: gpu_lib.ltompc_record_size(None), lambda: gpu_lib.ltompc_record_save(None, C.byref(rec)),
                 lambda: gpu_lib.ltompc_record_select(None, None), lambda: gpu_lib.ltompc_record_release(None, None),
                 lambda: gpu_lib.ltompc_record_trim(None), lambda: gpu_lib.ltompc_record_stats(None, C.byref(a), C.byref(b))):
        assert call() == -1
        assert b"null handle" in gpu_lib.ltompc_last_error()
    assert not rec.value
