"""k_step1 with the instance's operands staged in LDS (csrc/linesearch.h: d_step1_stage, StepStage; profiles/r09), from the
device-only compilation to assembly of test_kernel_resources_lut.py: the three forms of the reference's bound pattern - k_step1
(with and without the friction ellipse), k_step1_pi, k_step1_ts - hold the staging array as static LDS of at most 48 KiB (the host
harness starts them with no dynamic LDS, and three workgroups fit a CU), and their text has fewer `global_load` instructions than
before the staging: the loads of state, step and slacks in the line search and 14 of the update's 24 words per row are LDS reads
now.  There is no fallback kernel: a horizon or a bound pattern that one window does not hold takes several windows in the same
kernel.  (Registers, spills, occupancy and waits of the same kernels: tests/test_kernel_resources_step1_update.py, unchanged.)

The compilation takes minutes, and the modules that use the `isa` fixture before this one in a session have each made it and
left the assembly in the session's temporary directory: that file is read where it exists, and the fixture is asked for only
when this module runs on its own.  Needs hipcc, not a GPU."""
import re

import pytest

from test_kernel_resources_lut import isa  # noqa: F401  (the module-scoped fixture: one device-only compilation to assembly)
from test_kernel_resources_step1_update import K_STEP1, K_STEP1_ELL, K_STEP1_PI, K_STEP1_TS

LDS_CEILING = 48 * 1024
# `global_load` instructions in the kernel's text, measured from the final build   (the parent commit, counted the same way)
GLOBAL_LOAD_CEILING = {K_STEP1: 426,      # (516)
                       K_STEP1_ELL: 426,  # (524)
                       K_STEP1_PI: 447,   # (537)
                       K_STEP1_TS: 450}   # (540)


def _assembly(tmp_path_factory):
    return sorted(tmp_path_factory.getbasetemp().glob("isa*/ltompc_dev.s"))


@pytest.fixture(scope="module")
def text(request, tmp_path_factory):
    """Per kernel: global_load instructions, LDS reads and writes, static LDS bytes from the kernel descriptor."""
    if not _assembly(tmp_path_factory):
        request.getfixturevalue("isa")
    out, cur = {}, None
    for line in open(_assembly(tmp_path_factory)[0]):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), dict(gl=0, ds=0, lds=None))
            continue
        m = re.match(r"\s*\.amdhsa_group_segment_fixed_size (\d+)", line)
        if m and cur is not None:
            cur["lds"] = int(m.group(1))
        w = line.split()
        if cur is None or not w:
            continue
        if w[0].startswith("global_load"):
            cur["gl"] += 1
        elif w[0].startswith("ds_read") or w[0].startswith("ds_write"):
            cur["ds"] += 1
    return out


@pytest.mark.parametrize("kernel", sorted(GLOBAL_LOAD_CEILING))
def test_static_lds_and_fewer_global_loads(text, kernel):
    assert kernel in text, f"{kernel} not in the assembly"
    t = text[kernel]
    print(kernel, t)
    assert t["lds"] is not None and 0 < t["lds"] <= LDS_CEILING, t
    assert t["ds"] > 0, t
    assert t["gl"] <= GLOBAL_LOAD_CEILING[kernel], t
