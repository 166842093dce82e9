"""The batch sizes of the fp32-unit GPU tests against the forward dispatch itself (csrc/nplda_fwd_dispatch.h), no GPU: each
pair-scoring case takes the kernel family and the split its table names, and each embedding case the kernel its table names.
The GPU tests assert the kernel NAME, which labels a FWD_SPLIT batch by its streaming kernel and has no form for embed(); this
pins what the name cannot show (compiled host-only from tests/c/fp32_units_dispatch.hip, as tests/test_dispatch_cpu.py does)."""
import os
import shutil
import subprocess

import pytest

from tests.test_fp32_units_fwd_gpu import CUS, EMBED_CASES, MID, PAIR_CASES, SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_SMALL, FWD_MID, FWD_STREAM, FWD_SPLIT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def dispatch_bin(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("fp32_units_dispatch") / "fp32_units_dispatch")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "neuralplda_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "fp32_units_dispatch.hip"), "-o", out], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _query(binary, D0, D, sizes):
    out = subprocess.run([binary, str(D0), str(D), str(CUS)] + [str(n) for n in sizes], capture_output=True, text=True,
                         timeout=60, check=True).stdout
    rows = {}
    for ln in out.splitlines():
        n, k, sp, kr, emb = ln.split()
        rows[int(n)] = (int(k), int(sp), int(kr), emb)
    return rows


@pytest.mark.parametrize("D0,D,B,kernel,split", PAIR_CASES)
def test_pair_cases_take_their_kernel_and_split(dispatch_bin, D0, D, B, kernel, split):
    k, sp, kr, _ = _query(dispatch_bin, D0, D, [B])[B]
    if kernel == MID:
        assert k == FWD_MID, k
    elif kernel == SMALL:
        assert k == FWD_SMALL, k
    elif split:  # full rounds streamed, the remainder (less than one round) on the balanced-tile kernel
        assert k == FWD_SPLIT and kr == FWD_MID and 0 < B - sp < 128 * CUS, (k, sp, kr)
    else:
        assert k == FWD_STREAM, k


@pytest.mark.parametrize("D", [150, 170])
@pytest.mark.parametrize("N,tile,kernel", EMBED_CASES)
def test_embed_cases_take_their_kernel(dispatch_bin, D, N, tile, kernel):
    assert _query(dispatch_bin, 512, D, [N])[N][3] == kernel
