"""Register budget of the wave-cooperative Riccati sweep: compiled device-only for gfx950 with the flags of _build.py,
k_riccati8 and its sensitivity instantiation run with no VGPR spilled and no scratch memory (a spill reload in
the stage loop waited for the stage block in flight).  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc", "ltompc.hip")
KERNELS = ["_ZN6ltompc10k_riccati8ENS_6ConstsENS_4WorkENS_6LaunchEii",  # ltompc::k_riccati8
           "_ZN6ltompc15k_sens_riccati8ENS_6ConstsENS_4WorkEPKiPi"]    # ltompc::k_sens_riccati8


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("res") / "ltompc_dev.o"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "--cuda-device-only", "-c", SRC,
           "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(SRC))
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


@pytest.mark.parametrize("kernel", KERNELS)
def test_riccati8_does_not_spill(resources, kernel):
    assert kernel in resources, f"{kernel} not in the compiler's resource report"
    r = resources[kernel]
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 1, r  # one wavefront per SIMD, as designed
