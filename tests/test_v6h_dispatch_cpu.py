"""Which layer-1 form the headline kernel's dispatch launches, and the label it reports, on the dispatch's own host code
(csrc/nplda_fwd_dispatch.h, compiled host-only from tests/c/v6h_dispatch.hip), no GPU: the hybrid form
(nplda_fwd_v6h_kernel) for D = 150 layouts with an even count of k16-steps, nplda_fwd_v6_kernel otherwise and under
NPLDA_FWD_V6_L1=f32 / NPLDA_FWD_V6_L2=f32; NPLDA_FWD_V6_L1S picks another instantiated S1.  Also pins that the ragged
batches of tests/test_v6_hybrid_l1_gpu.py are streamed whole, which the label cannot show."""
import os
import shutil
import subprocess

import pytest

from tests.test_v6_hybrid_l1_gpu import EVEN_KS1_CASES, N_SPLIT, ODD_KS1_CASES, ONE_ROUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_MID, FWD_STREAM, FWD_SPLIT = 1, 2, 3
PREFIX = "nplda_fwd_v6_kernel (persistent, "
SWITCHES = ("NPLDA_FWD_V6_L1", "NPLDA_FWD_V6_L1S", "NPLDA_FWD_V6_L2", "NPLDA_FWD_NO_V6", "NPLDA_FWD_NO_MID", "NPLDA_FWD_NO_SPLIT",
            "NPLDA_FWD_SMALL_MAX")


@pytest.fixture(scope="module")
def dispatch_bin(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("v6h_dispatch") / "v6h_dispatch")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "neuralplda_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "v6h_dispatch.hip"), "-o", out], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _query(binary, D0, n, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    out = subprocess.run([binary, str(D0), "150", "256", str(n)], capture_output=True, text=True, timeout=60, check=True,
                         env=e).stdout
    head, label = out.strip().split(" | ", 1)
    _, choice, s1, default = (int(v) for v in head.split())
    return choice, s1, default, label


def _hybrid_label(label, s1):
    return (label.startswith(PREFIX) and "split bf16x3" in label and "nplda_fwd_v6h_kernel" in label
            and f"S1 = {s1}: {10 - s1} feature blocks" in label)


def _v6_label(label, l2_split=True):
    return label.startswith(PREFIX) and "v6h" not in label and ("split bf16x3" in label) == l2_split and (l2_split or "split" not in label)


@pytest.mark.parametrize("D0,n,choice", [(512, 1 << 20, FWD_STREAM), (512, ONE_ROUND, FWD_STREAM), (512, N_SPLIT, FWD_SPLIT),
                                         (512, 2 * ONE_ROUND + 77, FWD_SPLIT)] + [(d0, n, FWD_STREAM) for d0, n in EVEN_KS1_CASES])
def test_even_k16_step_counts_take_the_hybrid_kernel(dispatch_bin, D0, n, choice):
    k, s1, default, label = _query(dispatch_bin, D0, n)
    assert k == choice and s1 == default and default in (2, 3, 4) and _hybrid_label(label, default), (k, s1, default, label)


def test_one_round_and_77_pairs_go_to_the_balanced_tile_kernel(dispatch_bin):
    k, _, _, label = _query(dispatch_bin, 512, ONE_ROUND + 77)
    assert k == FWD_MID and label.startswith("nplda_fwd_mid_kernel"), (k, label)


@pytest.mark.parametrize("D0,n", ODD_KS1_CASES + [(144, 20037)])
def test_odd_k16_step_counts_keep_v6(dispatch_bin, D0, n):
    for env in ({}, {"NPLDA_FWD_V6_L1S": "4"}):
        k, s1, _, label = _query(dispatch_bin, D0, n, **env)
        assert k == FWD_STREAM and s1 == 0 and _v6_label(label), (env, k, s1, label)


@pytest.mark.parametrize("D0,n", [(512, 1 << 20), (96, 20037)])
def test_environment_switches(dispatch_bin, D0, n):
    _, s1, _, label = _query(dispatch_bin, D0, n, NPLDA_FWD_V6_L1="f32")
    assert s1 == 0 and _v6_label(label), (s1, label)  # today's default: fp32 layer 1, split layer 2
    _, s1, _, label = _query(dispatch_bin, D0, n, NPLDA_FWD_V6_L1="f32", NPLDA_FWD_V6_L1S="3")
    assert s1 == 0 and _v6_label(label), (s1, label)
    _, s1, _, label = _query(dispatch_bin, D0, n, NPLDA_FWD_V6_L2="f32")
    assert s1 == 0 and _v6_label(label, l2_split=False), (s1, label)  # the all-fp32 form
    _, s1, _, label = _query(dispatch_bin, D0, n, NPLDA_FWD_V6_L2="f32", NPLDA_FWD_V6_L1S="3")
    assert s1 == 0 and _v6_label(label, l2_split=False), (s1, label)
    for want in (2, 3, 4):
        _, s1, _, label = _query(dispatch_bin, D0, n, NPLDA_FWD_V6_L1S=str(want))
        assert s1 == want and _hybrid_label(label, want), (want, s1, label)
    for other in ("0", "1", "5", "10", "x"):  # not instantiated: the default
        _, s1, default, label = _query(dispatch_bin, D0, n, NPLDA_FWD_V6_L1S=other)
        assert s1 == default and _hybrid_label(label, default), (other, s1, label)
    _, _, _, label = _query(dispatch_bin, D0, n, NPLDA_FWD_NO_V6="1")
    assert label.startswith("nplda_fwd_v3_kernel"), label
