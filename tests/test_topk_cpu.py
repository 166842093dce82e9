"""The top-k search without a GPU: the numpy oracle of tests/topk_ref.py on the inputs tests/test_topk_gpu.py uses (exact
cases are exact and tie across rank k; the float32 unit satisfies the GPU test's selection condition), the argument checks
and the sizing function of the C entry point, the chunk-cap variable, the canonicalise-and-deduplicate step of
mine_hard_trials and the resource budget of csrc/nplda_topk.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from neuralplda_amd import sv_trials_loaders
from tests import topk_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuralplda_amd", "csrc")


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D2", [32, 150, 170])
def test_exact_inputs_are_exact_in_any_order(D2):
    """float32 in two feature orders equals float64 bit for bit, |s| < 1000."""
    rng = np.random.default_rng(D2)
    P_sqrt, Q = tr.exact_params(D2, rng)
    zr, zt = tr.exact_rows(40, D2, rng), tr.exact_rows(300, D2, rng)
    rev, perm = list(range(D2))[::-1], list(rng.permutation(D2))
    q32 = tr.qvec(zt, Q, np.float32)
    assert np.array_equal(q32, tr.qvec(zt, Q, np.float32, rev)) and np.array_equal(q32.astype(np.float64), tr.qvec(zt, Q, np.float64))
    qr = tr.qvec(zr, Q, np.float32)
    S64 = tr.scores(zr, qr, zt, q32, P_sqrt, np.float64)
    for order in (None, rev, perm):
        S32 = tr.scores(zr, qr, zt, q32, P_sqrt, np.float32, order)
        assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), S64)
    assert np.abs(S64).max() < 1000.0


@pytest.mark.parametrize("cs", tr.EXACT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_exact_cases_tie_across_rank_k(cs):
    """The generator asserts the tie (where a row has more than k eligible columns); here also: every score of a full-mask
    row occurs at least three times, and the oracle's output is sorted with ties in ascending column order."""
    c = tr.exact_case(*cs)
    if c["M"] >= 3 and c["M"] % 3 == 0:
        _, n = np.unique(c["S"][0], return_counts=True)
        assert n.min() >= 3
    for lg in (True, False):
        vals, idx = c["ref"][lg]
        assert vals.shape == idx.shape == (c["R"], c["k"]) and vals.dtype == np.float32
        have = idx >= 0
        assert (have.sum(1) == np.minimum(c["elig"].sum(1), c["k"])).all()
        both = have[:, 1:]
        a, b = vals[:, :-1], vals[:, 1:]
        assert ((a >= b) if lg else (a <= b))[both].all() and (idx[:, :-1] < idx[:, 1:])[both & (a == b)].all()
        assert np.isinf(vals[~have]).all()


def test_topk_oracle_on_a_hand_made_row():
    S = np.array([[1.0, 3.0, -0.0, 3.0, 0.0, 2.0]], np.float32)
    e = np.array([[True, True, True, True, True, False]])
    v, i = tr.topk(S, e, 4, True)
    assert i.tolist() == [[1, 3, 0, 2]] and v.tolist() == [[3.0, 3.0, 1.0, 0.0]]
    v, i = tr.topk(S, e, 6, False)
    assert i.tolist() == [[2, 4, 0, 1, 3, -1]] and v[0, 5] == np.inf    # -0.0 == +0.0: column order decides


@pytest.mark.parametrize("cs", tr.FLOAT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_float32_reference_meets_the_selection_condition(cs):
    """The float32 unit, selected exactly, satisfies the GPU test's checks with zero violations: the tolerance
    (D2 + 8) 2^-24 A is an a-priori bound, it leaves room for any evaluation order (worst ratio here: about 0.02)."""
    c = tr.float_case(*cs)
    for lg in (True, False):
        vals, idx = tr.topk(c["S32"], c["elig"], c["k"], lg)
        worst = tr.check_float_result(vals, idx, c, lg, f"float32 reference {cs} largest={lg}")
        assert worst < 0.1
    assert (np.abs(c["S32"] - c["S64"]) <= c["tol"]).all()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_abi_argument_checks(hip_lib):
    EINVAL, EUNSUP, ENOSPC = -22, -95, -28
    L = hip_lib
    dummy = ctypes.create_string_buffer(4096)
    p16 = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40

    def call(zr=p16, qr=p16, R=8, zt=p16, qt=p16, M=100, ldz=160, packed=p16, D0=512, D1=150, D2=150, k=10, largest=1,
             mode=0, lr=None, lt=None, gr=None, gt=None, sr=None, vals=p16, idx=p16, ws=p16, wsb=big):
        return L.nplda_topk_scores_f32(zr, qr, R, zt, qt, M, ldz, packed, D0, D1, D2, k, largest, mode, lr, lt, gr, gt, sr,
                                       vals, idx, ws, wsb, None)

    size = L.nplda_topk_workspace_bytes
    need = size(8, 100, 150, 10)
    assert need >= 8 * 10 * 8 and need % 256 == 0
    # never decreases with R, M or k
    for R in (1, 63, 64, 65, 128, 129, 192, 193, 1000, 40000):
        assert size(R + 1, 5000, 150, 10) >= size(R, 5000, 150, 10) > 0
    last = 0
    for R in range(1, 700, 7):
        assert size(R, 1 << 20, 150, 64) >= last
        last = size(R, 1 << 20, 150, 64)
    for M in (0, 1, 63, 64, 65, 3000, 1 << 20):
        assert size(17, M + 1, 150, 10) >= size(17, M, 150, 10) > 0
    for k in range(1, 128):
        assert size(17, 3000, 150, k + 1) >= size(17, 3000, 150, k)
    # zero on unsupported
    assert size(-1, 100, 150, 10) == 0 and size(8, -1, 150, 10) == 0 and size(8, 100, 193, 10) == 0 and size(8, 100, 0, 10) == 0
    assert size(8, 100, 150, 0) == 0 and size(8, 100, 150, 129) == 0 and size(8, 1 << 31, 150, 10) == 0 and size(1 << 24, 100, 150, 10) == 0
    assert size(8, (1 << 31) - 1, 192, 128) > 0 and size((1 << 24) - 1, 100, 150, 10) > 0

    assert call(R=0) == 0 and call(R=0, zr=None, vals=None, ws=None) == 0          # a no-op: nothing is launched
    for kw in (dict(zr=None), dict(qr=None), dict(zt=None), dict(qt=None), dict(packed=None), dict(vals=None), dict(idx=None),
               dict(ws=None)):
        assert call(**kw) == EINVAL, kw
    assert call(R=-1) == EINVAL and call(M=-1) == EINVAL and call(D2=0) == EINVAL
    assert call(k=0) == EINVAL and call(k=129) == EINVAL and call(largest=2) == EINVAL
    assert call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(mode=1) == EINVAL and call(mode=2, lr=p16) == EINVAL and call(mode=1, lt=p16) == EINVAL   # labels missing
    assert call(gr=p16) == EINVAL and call(gt=p16) == EINVAL                                               # both or neither
    assert call(zr=p16 + 4) == EINVAL and call(zt=p16 + 8) == EINVAL and call(ws=p16 + 4) == EINVAL
    assert call(ldz=150) == EINVAL and call(ldz=162) == EINVAL and call(ldz=156) == EINVAL               # short / misaligned rows
    assert call(D0=510) == EINVAL
    assert call(D2=193, ldz=208) == EUNSUP and call(D1=200, ldz=208) == EUNSUP
    assert call(M=1 << 31) == EUNSUP and call(R=1 << 31) == EUNSUP and call(R=1 << 24) == EUNSUP
    assert call(wsb=need - 1) == ENOSPC and call(wsb=0) == ENOSPC


def test_chunk_cap_variable_only_lowers_the_workspace(hip_lib, monkeypatch):
    size = hip_lib.nplda_topk_workspace_bytes
    shapes = [(1, 3000, 150, 10), (1, 1 << 20, 150, 128), (65, 3000, 170, 128), (1000, 100000, 150, 64), (40000, 5000, 32, 1)]
    monkeypatch.delenv("NPLDA_TOPK_MAX_CHUNKS", raising=False)
    default = [size(*s) for s in shapes]
    prev = [0] * len(shapes)
    for cap in ("1", "2", "3", "7", "64"):             # a cap lowers the size or leaves it; a higher cap never gives less
        monkeypatch.setenv("NPLDA_TOPK_MAX_CHUNKS", cap)
        got = [size(*s) for s in shapes]
        assert all(0 < p <= g <= d for p, g, d in zip(prev, got, default)) or prev[0] == 0 and all(0 < g <= d for g, d in zip(got, default)), cap
        prev = got
    for cap in ("100000", "0", "-5", "junk"):          # above the built-in cap, or no number at all: unchanged
        monkeypatch.setenv("NPLDA_TOPK_MAX_CHUNKS", cap)
        assert [size(*s) for s in shapes] == default, cap
    monkeypatch.setenv("NPLDA_TOPK_MAX_CHUNKS", "1")
    assert size(1, 1 << 20, 150, 128) < default[1]     # one chunk: one list per row
    assert size(1, 1 << 20, 150, 128) == 64 * 128 * 8


# ---- mine_hard_trials: canonicalise and deduplicate ----------------------------------------------------------------------------------

def test_canonical_trials_on_hand_made_indices():
    rows = torch.tensor([10, 11, 20, 21, 30], dtype=torch.int64)       # positions 0..4 -> table rows
    neg = torch.tensor([[2, 3], [2, -1], [0, 1], [-1, -1], [0, 0]])     # (10,20) found from both sides; a repeated slot
    pos = torch.tensor([[1], [0], [3], [2], [-1]])                      # (10,11) and (20,21), each from both sides
    r1, r2, t = sv_trials_loaders.canonical_trials(rows, neg, pos)
    assert r1.dtype == torch.int64 and r2.dtype == torch.int64 and t.dtype == torch.float32
    got = list(zip(r1.tolist(), r2.tolist(), t.tolist()))
    assert got == [(10, 11, 1.0), (10, 20, 0.0), (10, 21, 0.0), (10, 30, 0.0), (11, 20, 0.0), (20, 21, 1.0)]
    assert (10, 11, 0.0) not in got                                     # a mined positive is no negative
    # positives only, negatives only, nothing at all, a self pair is dropped
    r1, r2, t = sv_trials_loaders.canonical_trials(rows, None, pos)
    assert list(zip(r1.tolist(), r2.tolist())) == [(10, 11), (20, 21)] and t.tolist() == [1.0, 1.0]
    r1, r2, t = sv_trials_loaders.canonical_trials(rows, torch.tensor([[0], [0], [-1], [-1], [-1]]))
    assert list(zip(r1.tolist(), r2.tolist())) == [(10, 11)] and t.tolist() == [0.0]
    r1, r2, t = sv_trials_loaders.canonical_trials(rows, torch.full((5, 3), -1))
    assert r1.numel() == r2.numel() == t.numel() == 0
    r1, r2, t = sv_trials_loaders.canonical_trials(torch.zeros(0, dtype=torch.int64))
    assert r1.numel() == 0 and t.dtype == torch.float32


def test_mined_pairs_oracle_matches_canonical_trials():
    """The oracle's list (a python set of pairs) equals canonical_trials on the oracle's own top-k indices."""
    rng = np.random.default_rng(5)
    n = 60
    S = rng.integers(-8, 9, (n, n)).astype(np.float32)
    S = S + S.T
    spk, grp = rng.integers(0, 7, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)
    rows = np.sort(rng.choice(200, n, replace=False)).astype(np.int64)
    full_spk, full_grp = np.zeros(200, np.int32), np.zeros(200, np.int32)
    full_spk[rows], full_grp[rows] = spk, grp
    want = tr.mined_pairs(S, full_spk, full_grp, rows, 3, 2)
    me = np.arange(n)
    neg = tr.topk(S, tr.eligible(n, n, "different", spk, spk, grp, grp, me), 3, True)[1]
    pos = tr.topk(S, tr.eligible(n, n, "same", spk, spk, grp, grp, me), 2, False)[1]
    got = sv_trials_loaders.canonical_trials(torch.from_numpy(rows), torch.from_numpy(neg), torch.from_numpy(pos))
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)
    assert want[2].sum() > 0 and (want[2] == 0).sum() > 0 and (want[0] < want[1]).all()


def test_gallery_stamp_covers_the_extractor():
    """A Gallery is stale once ANY tensor extract_plda_embeddings reads has changed: the head's and, for
    Etdnn_Xvec_NeuralPlda, the extractor's weights and batch-norm statistics."""
    from neuralplda_amd import models, search, xvector

    class NC:
        xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
        beta, alpha, device, loss, pooling_function = [99.0], 15.0, "cpu", "SoftCdet", "std"

    for m in (models.NeuralPlda(NC), xvector.Etdnn_Xvec_NeuralPlda(NC)):
        gal = search.Gallery(m, None, torch.zeros(3, 160), torch.zeros(3), ids=["a", "b", "c"], stamp=search.model_stamp(m))
        gal.check()
        assert gal.ids_of(torch.tensor([[2, -1]])) == [["c", None]]
        touched = [m.Q] + ([m.xvector_extractor.tdnn1.kernel.weight, m.xvector_extractor.tdnn1.bn.running_mean]
                           if hasattr(m, "xvector_extractor") else [])
        for t in touched:
            stamp = search.model_stamp(m)
            with torch.no_grad():
                t.add_(1.0)
            assert search.model_stamp(m) != stamp
            with pytest.raises(ValueError):
                gal.check()
            gal.stamp = search.model_stamp(m)


# ---- kernel resources --------------------------------------------------------------------------------------------------------------

def _resources(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    err = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, "-c", os.path.join(CSRC, src), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): +(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_register_and_lds_budget_of_the_topk_kernels():
    """design/k19_topk_search.md plans three blocks of four waves per CU for k <= 16 (at most 168 registers, three waves per
    SIMD), two for k <= 64 (at most 256) and one for k <= 128, whose candidate lists take 128 KB: static LDS (the 16-row stage and its labels) plus the
    dynamic candidate lists, 64 rows x 2 KC x 8 bytes, within 160 KB per CU.  No kernel uses scratch."""
    res = _resources("nplda_topk.hip")
    main = {k: v for k, v in res.items() if "topk_mainILi" in k}
    assert len(main) == 6 * 3, sorted(res)   # NB in {2, 4, 8, 10, 11, 12} x KC in {16, 64, 128}
    for name, v in main.items():
        nb, kc = map(int, re.search(r"topk_mainILi(\d+)ELi(\d+)E", name).groups())
        blocks = {16: 3, 64: 2, 128: 1}[kc]   # (k <= 16: the 768-block plan needs three waves per SIMD, 168 registers)
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= blocks and v["VGPRs"] + v["AGPRs"] <= 512 // blocks // 8 * 8, (name, v)
        assert v["VGPRs"] + v["AGPRs"] <= 256, (name, v)
        assert v["LDS"] <= 16 * (16 * nb + 4) * 4 + 3 * 64 + 64, (name, v)
        assert blocks * (v["LDS"] + 64 * 2 * kc * 8) <= 160 * 1024, (name, v)
    rest = {k: v for k, v in res.items() if k not in main}
    assert len(rest) == 1, sorted(res)       # the merge
    for name, v in rest.items():
        assert v["ScratchSize"] == 0 and v["LDS"] <= 4 * 256 * 8 and v["VGPRs"] + v["AGPRs"] <= 128, (name, v)
