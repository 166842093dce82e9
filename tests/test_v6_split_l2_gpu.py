"""The headline kernel's layer 2 in split form (csrc/nplda_fwd_v6.h, L2S = 1: normalised y and W2 as three bf16 pieces, six
16x16x32 passes, fp32 accumulation) against the fp64 oracle at the SURVEY 8(c) tolerance, and against the fp32 layer 2
(NPLDA_FWD_V6_L2=f32, a child process: the dispatch reads the switch once) on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL, RTOL = 2e-5, 1e-5
D0, D = 512, 150
N_ROUNDS = 131072 + 77  # four full rounds of the persistent grid on 256 CUs + a remainder for the balanced-tile kernel


def _params(seed, w1_row_scale=None, zero_b1=False):
    rng = np.random.default_rng(seed)
    k1, k2 = 1 / np.sqrt(D0), 1 / np.sqrt(D)
    W1 = rng.uniform(-k1, k1, (D, D0)).astype(np.float32)
    if w1_row_scale is not None:
        W1 *= w1_row_scale[:, None].astype(np.float32)
    b1 = np.zeros(D, np.float32) if zero_b1 else rng.uniform(-k1, k1, D).astype(np.float32)
    return orc.Params(W1, b1, rng.uniform(-k2, k2, (D, D)).astype(np.float32), rng.uniform(-k2, k2, D).astype(np.float32),
                      rng.uniform(0, 1, D).astype(np.float32), rng.uniform(0, 1, D).astype(np.float32))


def _score(p, x1, x2):
    from neuralplda_amd import ops
    packed = ops.pack_params(*[torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in p.tensors()])
    return ops.score_pairs(torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda(), packed).cpu().numpy()


def _check(s, x1, x2, p, idx):
    ref = orc.forward(x1[idx], x2[idx], p, np.float64)
    err = np.abs(s[idx] - ref)
    assert np.all(np.isfinite(s[idx])) and np.all(err <= ATOL + RTOL * np.abs(ref)), float(err.max())
    return float(err.max())


def _kernel_name(n):
    from neuralplda_amd import _lib
    return _lib.load().nplda_score_pairs_kernel_name(n, D0, D, D).decode()


def test_default_is_the_split_form(hip_lib):
    name = _kernel_name(1 << 20)
    assert name.startswith("nplda_fwd_v6_kernel (persistent, ") and "split bf16x3" in name, name


def test_full_size_sample_matches_oracle(hip_lib):
    from neuralplda_amd import ops
    B = 1 << 20
    rng = np.random.default_rng(31)
    p = _params(31)
    packed = ops.pack_params(*[torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in p.tensors()])
    gen = torch.Generator(device="cuda").manual_seed(31)
    x1 = torch.randn(B, D0, device="cuda", generator=gen)
    x2 = torch.randn(B, D0, device="cuda", generator=gen)
    s = ops.score_pairs(x1, x2, packed)
    assert s.shape == (B,) and bool(torch.isfinite(s).all())
    idx = torch.from_numpy(np.sort(rng.choice(B, 4096, replace=False))).cuda()
    ref = orc.forward(x1[idx].cpu().numpy(), x2[idx].cpu().numpy(), p, np.float64)
    err = np.abs(s[idx].cpu().numpy() - ref)
    assert np.all(err <= ATOL + RTOL * np.abs(ref)), float(err.max())


def test_full_rounds_and_remainder_match_oracle(hip_lib):
    rng = np.random.default_rng(32)
    p = _params(32)
    x1 = rng.standard_normal((N_ROUNDS, D0), dtype=np.float32)
    x2 = rng.standard_normal((N_ROUNDS, D0), dtype=np.float32)
    s = _score(p, x1, x2)
    # pairs of every wave position of the first and last full tiles, a sample of the rest, and the whole remainder
    idx = np.unique(np.concatenate([np.arange(256), np.arange(131072 - 256, N_ROUNDS),
                                    rng.choice(N_ROUNDS, 2048, replace=False)]))
    _check(s, x1, x2, p, idx)


def test_wide_dynamic_range_of_y(hip_lib):
    """W1's rows scaled over 1e-6 .. 1e3 (the normalised y then spans ~9 decades within a row, so its bf16 pieces carry
    low pieces of very different exponents) and rows of x scaled over 1e-4 .. 1e4."""
    rng = np.random.default_rng(33)
    p = _params(33, w1_row_scale=10.0 ** rng.uniform(-6, 3, D))
    B = N_ROUNDS
    x1 = rng.standard_normal((B, D0), dtype=np.float32) * (10.0 ** rng.uniform(-4, 4, (B, 1))).astype(np.float32)
    x2 = rng.standard_normal((B, D0), dtype=np.float32) * (10.0 ** rng.uniform(-4, 4, (B, 1))).astype(np.float32)
    s = _score(p, x1, x2)
    _check(s, x1, x2, p, np.unique(np.concatenate([np.arange(512), rng.choice(B, 2048, replace=False)])))


def test_row_with_zero_first_layer_output(hip_lib):
    """b1 = 0 and all-zero rows: W1 x + b1 = 0, F.normalize's eps branch gives y = 0 and the score is the bias term alone."""
    rng = np.random.default_rng(34)
    p = _params(34, zero_b1=True)
    B = N_ROUNDS
    x1 = rng.standard_normal((B, D0), dtype=np.float32)
    x2 = rng.standard_normal((B, D0), dtype=np.float32)
    zr = np.array([0, 5, 17, 4095, 65536 + 3, 131071, 131072 + 10])  # full rounds and remainder, either side or both
    x1[zr[::2]] = 0.0
    x2[zr[1::2]] = 0.0
    x1[zr[-1]] = x2[zr[-1]] = 0.0
    s = _score(p, x1, x2)
    _check(s, x1, x2, p, np.unique(np.concatenate([zr, rng.choice(B, 1024, replace=False)])))


_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from tests.test_v6_split_l2_gpu import _inputs_ab, _score, _kernel_name, N_ROUNDS
p, x1, x2 = _inputs_ab()
np.save({out!r}, _score(p, x1, x2))
print(json.dumps({{"kernel": _kernel_name(1 << 20)}}))
"""


def _inputs_ab():
    rng = np.random.default_rng(35)
    p = _params(35)
    x1 = rng.standard_normal((N_ROUNDS, D0), dtype=np.float32)
    x2 = rng.standard_normal((N_ROUNDS, D0), dtype=np.float32)
    return p, x1, x2


def test_split_form_against_the_fp32_layer_2(hip_lib, tmp_path):
    out = str(tmp_path / "s_f32.npy")
    env = dict(os.environ, NPLDA_FWD_V6_L2="f32")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, out=out)], capture_output=True, text=True,
                       timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert child["kernel"].startswith("nplda_fwd_v6_kernel (persistent, ") and "split" not in child["kernel"], child
    assert "split bf16x3" in _kernel_name(1 << 20)  # this process runs the split form
    p, x1, x2 = _inputs_ab()
    s_new, s_old = _score(p, x1, x2), np.load(out)
    d = np.abs(s_new - s_old)
    assert np.all(d <= ATOL + RTOL * np.abs(s_old)), float(d.max())
    rng = np.random.default_rng(36)
    idx = np.unique(np.concatenate([np.arange(256), rng.choice(N_ROUNDS, 4096, replace=False)]))
    e_new, e_old = _check(s_new, x1, x2, p, idx), _check(s_old, x1, x2, p, idx)
    assert e_new <= 2 * max(e_old, 1e-7), (e_new, e_old)
