"""Register budget of k_rec_save (csrc/record.h), compiled device-only for gfx950 with the flags of _build.py:
no VGPR spilled, no scratch memory (its descriptor table is a by-value argument: an index into it that the compiler cannot
resolve would put the table into scratch), no LDS.  The kernel depends on nothing but layout.h, so it is compiled from a
translation unit of its own: the same code as in the library, in seconds.  Needs hipcc, not a GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC

CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")
KERNEL = "_ZN6ltompc10k_rec_saveENS_9RecPlanesEPKiii"  # ltompc::k_rec_save


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("rec")
    src = d / "rec_save.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "record.h"\n')
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "--cuda-device-only", "-c", str(src), "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), "-o", str(d / "rec_save.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    rows, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def test_rec_save_has_no_spill_no_scratch_no_lds(report):
    assert KERNEL in report, sorted(report)
    r = report[KERNEL]
    print(r)
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["LDS Size"] == 0, r


def test_the_library_includes_the_kernel():
    assert '#include "record.h"' in open(os.path.join(CSRC, "kernels.h")).read()
