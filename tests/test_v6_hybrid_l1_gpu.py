"""The headline kernel with a hybrid layer 1 (csrc/nplda_fwd_v6h.h: the last S1 feature blocks as three bf16 pieces and six
16x16x32 passes, the others on fp32-input MFMAs) in units of an fp32 computation (tests/fp32_units.py, default thresholds:
rms <= 3, max <= 5 over the whole output and every region) — units that tell a dropped bf16 piece from a correct product.
The dispatch takes the kernel for D = 150 layouts with an even count of k16-steps; NPLDA_FWD_V6_L1=f32 (read once per
process: a child process) runs nplda_fwd_v6.h on the same inputs.  Ratios measured on MI355X are noted next to each case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc
from tests import fp32_units as fu
from tests.test_forward_gpu import to_dev
from tests.test_fp32_units_fwd_gpu import CUS, _check_pairs, _inputs, _kernel_name, _pair_refs, _split_point

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL, RTOL = 2e-5, 1e-5
D = 150
ONE_ROUND = 128 * CUS           # 32 768 pairs: one full round of the persistent grid
N_SPLIT = 4 * ONE_ROUND + 77    # FWD_SPLIT: four full rounds on the streaming kernel, 77 pairs on the balanced-tile kernel
# fp32 rows, an even count of k16-steps, a ragged batch the dispatch streams whole (tests/test_v6h_dispatch_cpu.py pins the
# choice): D0 = 96 is three layer-1 chunks (the odd-count path), D0 = 64 two
EVEN_KS1_CASES = [(96, 20037), (64, 20037)]
ODD_KS1_CASES = [(72, 20037), (16, 20037)]  # five k16-steps, one k16-step: nplda_fwd_v6.h


def _is_hybrid(name):
    return (name.startswith("nplda_fwd_v6_kernel (persistent, ") and "split bf16x3" in name and "nplda_fwd_v6h_kernel" in name
            and "S1 = " in name)


def _score(p, x1, x2):
    from neuralplda_amd import ops
    return ops.score_pairs(x1, x2, ops.pack_params(*to_dev(p)))


def test_one_full_round(hip_lib):  # measured (worst rms / max ratio over the regions, S1 = 3): 1.60 / 1.89
    name = _kernel_name(ONE_ROUND, 512, D, D)
    assert _is_hybrid(name), name
    p, x1, x2 = _inputs(ONE_ROUND + 1, 512, D, ONE_ROUND)
    r = _check_pairs(_score(p, x1, x2), p, x1, x2, fu.Regions(ONE_ROUND, 128, seed=1), f"hybrid layer 1 B={ONE_ROUND}")
    print("ratios", r)


@pytest.mark.parametrize("B", [ONE_ROUND + 77, 2 * ONE_ROUND + 77])
def test_bf16_rows_with_a_partial_last_tile(hip_lib, B):
    """nplda_score_pairs_bf16rows_f32 streams a ragged batch whole (XM = 2 and a partial last tile) wherever the fp32 call
    would stream or split it.  That holds from two rounds + 77 pairs on; at one round + 77 the cost model prefers the
    balanced-tile kernel to a second, nearly empty round, and ops.score_pairs widens the rows for it — that size is kept as
    the case the change was specified with, and it pins the boundary."""
    # measured: 1.26 / 1.65 (widened rows, balanced-tile kernel) and 1.67 / 1.73 (XM = 2)
    name = _kernel_name(B, 512, D, D)
    assert _is_hybrid(name) if B > 2 * ONE_ROUND else name.startswith("nplda_fwd_mid_kernel"), name
    p, x1, x2 = _inputs(B + 2, 512, D, B, torch.bfloat16)
    r = _check_pairs(_score(p, x1, x2), p, x1, x2, fu.Regions(B, 128, seed=2), f"hybrid layer 1, bf16 rows B={B}")
    print("ratios", r)


@pytest.mark.parametrize("D0,B", EVEN_KS1_CASES)
def test_even_k16_step_counts_stream_a_ragged_batch_whole(hip_lib, D0, B):  # measured: D0 = 96 1.58 / 1.97, D0 = 64 1.57 / 1.57
    name = _kernel_name(B, D0, D, D)
    assert _is_hybrid(name), name
    p, x1, x2 = _inputs(B + D0, D0, D, B)
    r = _check_pairs(_score(p, x1, x2), p, x1, x2, fu.Regions(B, 128, seed=D0), f"hybrid layer 1 D0={D0} B={B}")
    print("ratios", r)


@pytest.mark.parametrize("D0,B", ODD_KS1_CASES)
def test_odd_k16_step_counts_keep_todays_kernel(hip_lib, D0, B):
    name = _kernel_name(B, D0, D, D)
    assert name.startswith("nplda_fwd_v6_kernel (persistent, ") and "split bf16x3" in name and "v6h" not in name, name
    p, x1, x2 = _inputs(B + D0, D0, D, B)
    _check_pairs(_score(p, x1, x2), p, x1, x2, fu.Regions(B, 128, seed=D0), f"v6 D0={D0} B={B}")


def test_full_rounds_and_remainder(hip_lib):  # measured: 1.56 / 1.72
    assert _is_hybrid(_kernel_name(N_SPLIT, 512, D, D))
    p, x1, x2 = _inputs(N_SPLIT + 3, 512, D, N_SPLIT)
    r = _check_pairs(_score(p, x1, x2), p, x1, x2, fu.Regions(N_SPLIT, 128, _split_point(N_SPLIT), seed=3),
                     f"hybrid layer 1 B={N_SPLIT}")
    print("ratios", r)


_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from tests.test_v6_hybrid_l1_gpu import _inputs, _score, _kernel_name, N_SPLIT, D
p, x1, x2 = _inputs(N_SPLIT + 3, 512, D, N_SPLIT)
np.save({out!r}, _score(p, x1, x2).cpu().numpy())
print(json.dumps({{"kernel": _kernel_name(N_SPLIT, 512, D, D)}}))
"""


def test_hybrid_against_the_fp32_layer_1(hip_lib, tmp_path):
    """The inputs of test_full_rounds_and_remainder under NPLDA_FWD_V6_L1=f32: the two score vectors agree to the oracle gate
    of the older tests, and the hybrid form's worst error against fp64 is at most twice the fp32 form's.  Measured: 3.4e-7
    against 4.0e-7, largest difference between the two 4.8e-7."""
    out = str(tmp_path / "s_f32.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, out=out)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT, env=dict(os.environ, NPLDA_FWD_V6_L1="f32"))
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert child["kernel"].startswith("nplda_fwd_v6_kernel (persistent, ") and "split bf16x3" in child["kernel"], child
    assert "v6h" not in child["kernel"], child
    assert _is_hybrid(_kernel_name(N_SPLIT, 512, D, D))  # this process runs the hybrid form
    p, x1, x2 = _inputs(N_SPLIT + 3, 512, D, N_SPLIT)
    s_new, s_old = _score(p, x1, x2).cpu().numpy(), np.load(out)
    d = np.abs(s_new - s_old)
    assert np.all(d <= ATOL + RTOL * np.abs(s_old)), float(d.max())
    reg = fu.Regions(N_SPLIT, 128, _split_point(N_SPLIT), sample=4096, seed=4)
    r64, _ = _pair_refs(p, x1, x2, reg)
    e_new, e_old = float(np.abs(s_new[reg.idx] - r64).max()), float(np.abs(s_old[reg.idx] - r64).max())
    print("max |error| against fp64: hybrid", e_new, "fp32 layer 1", e_old, "max |difference|", float(d.max()))
    assert e_new <= 2 * max(e_old, 1e-7), (e_new, e_old)


def test_wide_dynamic_range_of_x(hip_lib):
    """Rows of x scaled over 1e-4 .. 1e4: the bf16 pieces of x carry exponents eight decades apart from row to row.
    Measured: 1.80 / 2.36."""
    B = ONE_ROUND
    p, x1, x2 = _inputs(B + 5, 512, D, B)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x1 = x1 * 10.0 ** (8.0 * torch.rand(B, 1, device="cuda", generator=gen) - 4.0)
    x2 = x2 * 10.0 ** (8.0 * torch.rand(B, 1, device="cuda", generator=gen) - 4.0)
    r = _check_pairs(_score(p, x1, x2), p, x1, x2, fu.Regions(B, 128, seed=5), "hybrid layer 1, scaled rows")
    print("ratios", r)


def test_rows_with_zero_first_layer_output(hip_lib):
    """b1 = 0 and all-zero rows: W1 x + b1 = 0 in the fp32 and in the split blocks alike, F.normalize's eps branch gives
    y = 0 and the score is the bias term alone."""
    B = ONE_ROUND
    p, x1, x2 = _inputs(B + 6, 512, D, B)
    p = orc.Params(p.W1, np.zeros_like(p.b1), p.W2, p.b2, p.P_sqrt, p.Q)
    zr = torch.tensor([0, 5, 17, 127, 128, 4095, 16384 + 3, B - 1], device="cuda")
    x1[zr[::2]] = 0.0
    x2[zr[1::2]] = 0.0
    x1[zr[-1]] = 0.0
    s = _score(p, x1, x2)
    reg = fu.Regions(B, 128, seed=6)
    _check_pairs(s, p, x1, x2, reg, "hybrid layer 1, zero rows")
    zi = zr.cpu().numpy()
    ref = orc.forward(x1[zr].cpu().numpy(), x2[zr].cpu().numpy(), p, np.float64)
    got = s[zr].cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= ATOL + RTOL * np.abs(ref)), (zi, got, ref)
