"""Forward kernels in units of an fp32 computation (tests/fp32_units.py): every arithmetic path the pair-scoring, embedding,
gathered-row, score-epilogue and cohort-statistics dispatch can pick, against the fp64 oracle with the float32 oracle as the
unit.  Thresholds: rms_ratio <= 3, max_ratio <= 5 (fp32_units.RMS_MAX / MAX_MAX) unless a case says otherwise; the ratios
measured on MI355X are noted next to each case table.  Batch sizes follow csrc/nplda_fwd_dispatch.h on a 256-CU device and
every pair-scoring case asserts the kernel it reaches (nplda_score_pairs_kernel_name).  Large batches are generated on the
device; the oracle runs on the region rows only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc
from tests import fp32_units as fu
from tests.test_forward_gpu import rand_params, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256  # the sizes below assume the MI355X's 256 CUs (the kernel-name assertions check that they land where intended)

MID, SMALL = "nplda_fwd_mid_kernel", "nplda_fwd_small_kernel"
V3, V5, V6 = "nplda_fwd_v3_kernel", "nplda_fwd_v5_kernel", "nplda_fwd_v6_kernel"


def _kernel_name(B, D0, D1, D2):
    from neuralplda_amd import _lib
    return _lib.load().nplda_score_pairs_kernel_name(B, D0, D1, D2).decode()


def _split_point(B):
    return (B // 128 // CUS) * 128 * CUS  # csrc/nplda_fwd_dispatch.h: pair_split_point


def _inputs(seed, D0, D, B, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    p = rand_params(rng, D0, D, D)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x1 = torch.randn(B, D0, device="cuda", generator=gen).to(dtype)
    x2 = torch.randn(B, D0, device="cuda", generator=gen).to(dtype)
    return p, x1, x2


def _rows(x, reg):
    return x[torch.from_numpy(reg.idx).cuda()].float().cpu().numpy()


def _pair_refs(p, x1, x2, reg):
    a, b = _rows(x1, reg), _rows(x2, reg)
    return orc.forward(a, b, p, np.float64), orc.forward(a, b, p, np.float32)


def _check_pairs(s, p, x1, x2, reg, what, **thr):
    r64, r32 = _pair_refs(p, x1, x2, reg)
    return fu.assert_fp32_level(s[torch.from_numpy(reg.idx).cuda()].cpu().numpy(), r64, r32, what, reg, **thr)


# (D0, D, B, kernel, split): mid, small, mid where it beats the stream, the stream alone, FWD_SPLIT (full rounds streamed, the
# remainder on the balanced-tile kernel).  nplda_score_pairs_kernel_name labels a FWD_SPLIT batch by its streaming kernel, so
# the name cannot tell a split from a whole-batch stream: tests/test_fp32_units_dispatch_cpu.py pins the choice itself (split
# or not, and the remainder's kernel) for every case of this table on the dispatch's own code at 256 CUs.  Measured on MI355X, worst rms / max ratio over the regions of each kernel's cases:
# mid 1.34 / 1.49, small 1.47 / 1.53, v3 1.63 / 1.95, v5 1.78 / 2.39, v6 (split layer 2) 1.77 / 2.03.
PAIR_CASES = [
    (512, 150, 1000, MID, False), (512, 150, 2048, MID, False), (512, 150, 3000, SMALL, False),
    (512, 150, 10240, MID, False), (512, 150, 20037, MID, False), (512, 150, 32768, V6, False),
    (512, 150, 131072, V6, False), (512, 150, 131072 + 77, V6, True), (512, 150, 100000, V6, True),
    (512, 170, 1000, MID, False), (512, 170, 2048, MID, False), (512, 170, 3000, SMALL, False),
    (512, 170, 10240, MID, False), (512, 170, 20037, MID, False), (512, 170, 32768, V5, False),
    (512, 170, 131072, V5, False), (512, 170, 131072 + 77, V5, True), (512, 170, 100000, V5, True),
    (512, 128, 1000, SMALL, False), (512, 128, 16384, SMALL, False), (512, 128, 20037, V3, False),
    (512, 128, 131072 + 77, V3, False),
    (72, 150, 20037, V6, False), (72, 150, 131072 + 77, V6, False),  # v6 with an odd count of layer-1 chunks
]


@pytest.mark.parametrize("D0,D,B,kernel,split", PAIR_CASES)
def test_score_pairs_fp32_rows(hip_lib, D0, D, B, kernel, split):
    from neuralplda_amd import ops
    name = _kernel_name(B, D0, D, D)
    assert name.startswith(kernel), (B, name)
    if kernel == V6:
        assert "split bf16x3" in name, name  # layer 2 in split form (the default)
    p, x1, x2 = _inputs(B + D + D0, D0, D, B)
    s = ops.score_pairs(x1, x2, ops.pack_params(*to_dev(p)))
    tile = 128 if kernel in (V3, V5, V6) else 16
    reg = fu.Regions(B, tile, _split_point(B) if split else None, seed=B)
    _check_pairs(s, p, x1, x2, reg, f"score_pairs {name} D0={D0} D={D} B={B}")


_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from neuralplda_amd import ops
from tests.test_fp32_units_fwd_gpu import _inputs, _kernel_name
from tests.test_forward_gpu import to_dev
p, x1, x2 = _inputs({seed}, 512, 150, {B})
s = ops.score_pairs(x1, x2, ops.pack_params(*to_dev(p)))
np.save({out!r}, s.cpu().numpy())
print(json.dumps({{"kernel": _kernel_name({B}, 512, 150, 150)}}))
"""


@pytest.mark.parametrize("B", [32768, 131072 + 77])
def test_score_pairs_v6_fp32_layer_2(hip_lib, tmp_path, B):
    """NPLDA_FWD_V6_L2=f32 (read once per process: a child process) must meet the same yardstick (measured 1.78 / 2.05)."""
    out = str(tmp_path / "s.npy")
    seed = B + 150 + 512
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, out=out, seed=seed, B=B)], capture_output=True,
                       text=True, timeout=600, cwd=ROOT, env=dict(os.environ, NPLDA_FWD_V6_L2="f32"))
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert child["kernel"].startswith(V6) and "split" not in child["kernel"], child
    p, x1, x2 = _inputs(seed, 512, 150, B)
    reg = fu.Regions(B, 128, _split_point(B) if B % (128 * CUS) else None, seed=B)
    _check_pairs(torch.from_numpy(np.load(out)).cuda(), p, x1, x2, reg, f"v6 fp32 layer 2 B={B}")


@pytest.mark.parametrize("D,B,kernel", [(150, 32768, V6), (150, 131072 + 77, V6), (170, 32768, V5), (170, 131072 + 77, V5)])
def test_score_pairs_bf16_rows(hip_lib, D, B, kernel):
    """nplda_score_pairs_bf16rows_f32 (the streaming kernels read bf16 rows): the yardstick's input is the bf16-rounded rows
    (measured 1.83 / 2.18)."""
    from neuralplda_amd import ops
    assert _kernel_name(B, 512, D, D).startswith(kernel)
    p, x1, x2 = _inputs(B + D + 7, 512, D, B, torch.bfloat16)
    s = ops.score_pairs(x1, x2, ops.pack_params(*to_dev(p)))
    _check_pairs(s, p, x1, x2, fu.Regions(B, 128, seed=B), f"bf16 rows D={D} B={B}")


@pytest.mark.parametrize("D", [150, 170])
@pytest.mark.parametrize("B", [1, 1000, 20037])
def test_score_pairs_bf16x3(hip_lib, D, B):
    """The opt-in precision='bf16x3' image (nplda_score_pairs_bf16x3: six bf16 passes per fp32 product).  (No kernel-name
    query exists for this entry point: it has one kernel.)  Measured 1.77 / 2.05."""
    from neuralplda_amd import ops
    p, x1, x2 = _inputs(B + D + 11, 512, D, B)
    s = ops.score_pairs(x1, x2, ops.pack_params(*to_dev(p), precision="bf16x3"))
    _check_pairs(s, p, x1, x2, fu.Regions(B, 16, seed=B), f"bf16x3 D={D} B={B}")


def _check_embed(z, q, x, p, reg, what, D):
    xr = _rows(x, reg)
    z64 = orc.extract_plda_embeddings(xr, p, np.float64)
    z32 = orc.extract_plda_embeddings(xr, p, np.float32)
    sel = torch.from_numpy(reg.idx).cuda()
    zg = z[sel].cpu().numpy()
    assert np.all(zg[:, D:] == 0)
    fu.assert_fp32_level(zg[:, :D], z64, z32, what + " z", reg)
    if q is not None:
        fu.assert_fp32_level(q[sel].cpu().numpy(), orc.self_term(z64, p, np.float64), orc.self_term(z32, p, np.float32),
                             what + " q", reg)


# embed() (launch_fwd<MODE_EMBED>): U = (N + 1) / 2 units; the balanced-tile kernel where the pair cost model, without a split,
# picks it for U, else the small kernel up to 16 384 units, else v2.  The balanced-tile kernel wins up to just below a whole
# number of streaming rounds: N = 262 144 + 77 (131 111 units) still takes it, N = 262 144 - 153 (130 996 units, four full
# rounds at 256 CUs) goes to v2 — tests/test_fp32_units_dispatch_cpu.py checks these cases against the dispatch's own code.
# Measured (z and q): 1.56 / 1.96; embed_rows 1.29 / 1.60, embed_pair 1.35 / 1.70.
EMBED_CASES = [(1000, 16, "mid"), (5000, 32, "small"), (262144 - 153, 256, "v2")]


@pytest.mark.parametrize("D", [150, 170])
@pytest.mark.parametrize("N,tile,kernel", EMBED_CASES)
def test_embed(hip_lib, D, N, tile, kernel):
    from neuralplda_amd import ops
    p, x, _ = _inputs(N + D + 3, 512, D, N)
    z, q = ops.embed(x, ops.pack_params(*to_dev(p)))
    _check_embed(z, q, x, p, fu.Regions(N, tile, seed=N), f"embed D={D} N={N}", D)


@pytest.mark.parametrize("D", [150, 170])
def test_embed_rows_and_embed_pair(hip_lib, D):
    from neuralplda_amd import ops
    p, table, xb = _inputs(D + 5, 512, D, 5000)
    packed = ops.pack_params(*to_dev(p))
    rows = torch.from_numpy(np.random.default_rng(D).integers(0, 5000, 3001)).cuda()
    z, q = ops.embed_rows(table, rows, packed)
    xg = table[rows]
    _check_embed(z, q, xg, p, fu.Regions(3001, 16, full=True), f"embed_rows D={D}", D)
    (za, qa), (zb, qb) = ops.embed_pair(table[:1500], xb[:1701], packed)
    _check_embed(za, qa, table[:1500], p, fu.Regions(1500, 16, full=True), f"embed_pair a D={D}", D)
    _check_embed(zb, qb, xb[:1701], p, fu.Regions(1701, 16, full=True), f"embed_pair b D={D}", D)


@pytest.mark.parametrize("D", [150, 170])
@pytest.mark.parametrize("B", [1000, 20037])
def test_score_pairs_rows(hip_lib, D, B):
    """Pairs gathered from a resident table inside the kernel (nplda_score_pairs_rows_f32).  Measured 1.31 / 1.47."""
    from neuralplda_amd import ops
    p, table, _ = _inputs(B + D + 13, 512, D, 5000)
    rng = np.random.default_rng(B)
    r1, r2 = (torch.from_numpy(rng.integers(0, 5000, B)).cuda() for _ in range(2))
    s = ops.score_pairs_rows(table, r1, r2, ops.pack_params(*to_dev(p)))
    _check_pairs(s, p, table[r1], table[r2], fu.Regions(B, 16, seed=B), f"score_pairs_rows D={D} B={B}")


@pytest.mark.parametrize("D", [150, 170])
@pytest.mark.parametrize("with_q", [True, False])
def test_score_indexed_epilogue(hip_lib, D, with_q):
    """The gathered score epilogue on the device's own z (embedding error kept out of the measurement).  Measured 1.29 / 1.71."""
    from neuralplda_amd import ops
    p, x, _ = _inputs(D + 17, 512, D, 3000)
    packed = ops.pack_params(*to_dev(p))
    z, q = ops.embed(x, packed)
    rng = np.random.default_rng(D)
    B = 20037
    i1, i2 = rng.integers(0, 3000, B), rng.integers(0, 3000, B)
    s = ops.score_indexed(z, q if with_q else None, torch.from_numpy(i1).cuda(), torch.from_numpy(i2).cuda(), packed)
    zd = z.cpu().numpy()[:, :D]
    r64, r32 = orc.score_indexed(zd, i1, i2, p, np.float64), orc.score_indexed(zd, i1, i2, p, np.float32)
    if with_q:  # the kernel adds the device's own fp32 q: the yardstick starts from the same self terms
        qd = q.cpu().numpy().astype(np.float64)
        r64 = r64 - orc.self_term(zd[i1], p, np.float64) - orc.self_term(zd[i2], p, np.float64) + qd[i1] + qd[i2]
    fu.assert_fp32_level(s.cpu().numpy(), r64, r32, f"score_indexed D={D} q={with_q}", fu.Regions(B, 16, seed=B))


@pytest.mark.parametrize("D", [150, 170])
def test_score_embeddings_epilogue(hip_lib, D):  # measured 0.77 / 0.99
    from neuralplda_amd import ops
    rng = np.random.default_rng(D + 19)
    p = rand_params(rng, 512, D, D)
    B = 20037
    z1 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    z2 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    s = ops.score_embeddings(torch.from_numpy(z1).cuda(), torch.from_numpy(z2).cuda(), torch.from_numpy(p.P_sqrt).cuda(),
                             torch.from_numpy(p.Q).cuda())
    fu.assert_fp32_level(s.cpu().numpy(), orc.forward_from_plda_embeddings(z1, z2, p, np.float64),
                         orc.forward_from_plda_embeddings(z1, z2, p, np.float32), f"score_embeddings D={D}",
                         fu.Regions(B, 16, seed=B))


# ---- cohort statistics: the GEMM measured on the device's own z rows (cohort_scores fp64 vs fp32, statistics in fp64) ----

def _cohort_setup(D, R, M, seed):
    from neuralplda_amd import ops
    p, xr, _ = _inputs(seed, 512, D, R)
    _, xc, _ = _inputs(seed + 1, 512, D, M)
    packed = ops.pack_params(*to_dev(p))
    zr, qr = ops.embed(xr, packed)
    zc, qc = ops.embed(xc, packed)
    return p, packed, zr, qr, zc, qc


def cohort_refs(p, zr, qr, zc, qc, D, topn, select="lowest"):
    """fp64 / fp32 oracle statistics of the cohort score matrix of the device's z rows.  The kernels add the device's own fp32
    self terms q, so the fp64 matrix starts from those too (its cross term is orc.cohort_scores' without the self terms)."""
    a, b = zr.cpu().numpy()[:, :D], zc.cpu().numpy()[:, :D]
    cross = orc.cohort_scores(a, b, p, np.float64) - orc.self_term(a, p, np.float64)[:, None] - orc.self_term(b, p, np.float64)[None, :]
    c64 = qr.cpu().numpy().astype(np.float64)[:, None] + qc.cpu().numpy().astype(np.float64)[None, :] + cross
    return (orc.cohort_stats(c64, topn, select), orc.cohort_stats(orc.cohort_scores(a, b, p, np.float32), topn, select))


def check_cohort(got, r64, r32, what, **thr):
    """Each column on its own, over all rows and over the edge tiles of the fused kernel's 128-row items."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    reg = fu.Regions(got.shape[0], 128, full=True)
    assert np.array_equal(reg.idx, np.arange(got.shape[0]))
    for c, col in enumerate(("mean", "std", "mean_top", "std_top")):
        fu.assert_fp32_level(got[:, c], r64[:, c], r32[:, c], f"{what} {col}", reg, **thr)


# (D, R, M, topn): the full 256-row tiles and the 128-row tiles of small R (129, 300 rows: one / two items per resident block).
# Measured over all four columns, both forms, spill and prepared: 0.86 / 1.09.
COHORT_CASES = [(150, 300, 10000, 500), (170, 300, 10000, 500), (150, 129, 4096, 100), (170, 129, 4096, 100),
                (150, 517, 9999, 37)]


@pytest.mark.parametrize("form", ["split", "fp32"])
@pytest.mark.parametrize("D,R,M,topn", COHORT_CASES)
def test_cohort_stats_fused(hip_lib, monkeypatch, form, D, R, M, topn):
    """The fused path in its split form (default) and its fp32-input form (NPLDA_COHORT_SPLIT=0, read at every call), both
    selections."""
    from neuralplda_amd import ops
    p, packed, zr, qr, zc, qc = _cohort_setup(D, R, M, D + R + M)
    if form == "fp32":
        monkeypatch.setenv("NPLDA_COHORT_SPLIT", "0")
    for select in ("lowest", "highest"):
        got, nfb = ops.cohort_stats(zr, qr, zc, qc, packed, topn=topn, select=select, return_fallback_rows=True)
        assert nfb is not None and nfb <= R // 20, nfb
        check_cohort(got, *cohort_refs(p, zr, qr, zc, qc, D, topn, select), f"cohort {form} D={D} R={R} {select}")


@pytest.mark.parametrize("D", [150, 170])
def test_cohort_stats_spill_and_prepared(hip_lib, D):
    from neuralplda_amd import ops
    R, M, topn = 300, 10000, 500
    p, packed, zr, qr, zc, qc = _cohort_setup(D, R, M, D + 23)
    r64, r32 = cohort_refs(p, zr, qr, zc, qc, D, topn)
    check_cohort(ops.cohort_stats(zr, qr, zc, qc, packed, topn=topn, force_spill=True), r64, r32, f"cohort spill D={D}")
    prep = ops.cohort_prepare(zc, qc, packed, topn=topn)
    check_cohort(ops.cohort_stats(zr, qr, zc, qc, packed, topn=topn, prepared=prep), r64, r32, f"cohort prepared D={D}")
