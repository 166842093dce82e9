"""Register budget of the class-scatter kernel (csrc/nplda_scatter.hip): its grid is sized for two blocks per CU, and its MFMA
loop has no room for spills.  hipcc cross-compiles for gfx950 without a GPU, so this runs in the CPU suite."""
import os
import re
import shutil
import subprocess

import pytest

from neuralplda_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuralplda_amd", "csrc")


def _resources(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    err = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, "-c", os.path.join(CSRC, src), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): +(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_register_budget_of_the_class_scatter_kernels():
    assert callable(ops.class_scatter)
    res = _resources("nplda_scatter.hip")
    mfma = {k: v for k, v in res.items() if "scatter_kernelILb" in k}
    assert len(mfma) == 2, sorted(res)   # rows by index or in order
    for k, v in mfma.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
    rest = {k: v for k, v in res.items() if k not in mfma}
    assert len(rest) == 5, sorted(res)   # reduce, class sums (two forms), fix-up, total
    for k, v in rest.items():
        assert v["ScratchSize"] == 0, (k, v)
