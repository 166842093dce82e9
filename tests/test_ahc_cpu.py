"""The agglomerative clustering without a GPU: the numpy twin of tests/ahc_ref.py against scipy and on hand-made cases with
ties, the host re-cut, the exactness of the exact inputs, the argument checks of the C entry points (status codes come before
any launch), the declared names and the resource budget of csrc/nplda_ahc.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import ahc_ref as ar
from tests.test_topk_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINKS = ["average", "complete", "single"]


# ---- the twin ---------------------------------------------------------------------------------------------------------------------

def _partition(labels):
    return {frozenset(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)}


@pytest.mark.parametrize("linkage", LINKS)
def test_twin_against_scipy_on_tie_free_data(linkage):
    """scipy clusters by smallest distance: linkage on -S.  Heights agree (average: to the rounding of scipy's own
    recurrence, a weighted mean per step; complete and single exactly) and so do the partitions at several cuts."""
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(3)
    n = 60
    pts = rng.standard_normal((n, 5))
    S = (-np.linalg.norm(pts[:, None] - pts[None, :], axis=2)).astype(np.float32)
    rec, done, ncl, labels = ar.ahc(S, linkage)
    assert done == n - 1 and ncl == 1 and (labels == 0).all()
    Z = hier.linkage(-S[np.triu_indices(n, 1)].astype(np.float64), method=linkage)
    h = -Z[:, 2]
    assert (np.diff(rec["value"]) <= 0).all()
    if linkage == "average":
        assert np.abs(rec["value"] - h).max() <= 64 * np.finfo(np.float64).eps * np.abs(h).max()
    else:
        assert np.array_equal(rec["value"], h)
    assert np.array_equal(rec["size_after"], Z[:, 3].astype(np.int32))
    for k in (2, 3, 7, 20, 59):
        t = rec["value"][n - 1 - k]          # the last merge executed when k clusters remain
        mine = ar.cut(rec, n, threshold=t)
        assert np.unique(mine).size == k
        assert _partition(mine) == _partition(hier.fcluster(Z, k, criterion="maxclust"))
        assert np.array_equal(mine, ar.cut(rec, n, n_clusters=k))


def test_twin_on_hand_made_cases_with_ties():
    ones = ar.equal_matrix(5)
    for linkage in LINKS:
        rec, done, ncl, labels = ar.ahc(ones, linkage)
        assert [(r["a"], r["b"]) for r in rec] == [(0, 1), (0, 2), (0, 3), (0, 4)]
        assert rec["value"].tolist() == [1.0] * 4 and rec["size_after"].tolist() == [2, 3, 4, 5]
    # two tight pairs that tie: the lower pair first; then {0, 1} and {2, 3}: average (1 + 1 + 3 + 1) / 4, complete 1, single 3
    S = np.array([[0, 9, 1, 1, -5], [9, 0, 3, 1, -5], [1, 3, 0, 9, -5], [1, 1, 9, 0, -5], [-5, -5, -5, -5, 0]], np.float32)
    for linkage, third in (("average", 1.5), ("complete", 1.0), ("single", 3.0)):
        rec, done, ncl, labels = ar.ahc(S, linkage)
        assert [(r["a"], r["b"]) for r in rec] == [(0, 1), (2, 3), (0, 2), (0, 4)]
        assert rec["value"].tolist() == [9.0, 9.0, third, -5.0] and rec["size_after"].tolist() == [2, 2, 4, 5]
    # the lower triangle is never read
    T = S.copy()
    T[np.tril_indices(5, -1)] = 1e30
    T[np.diag_indices(5)] = -1e30
    assert np.array_equal(ar.ahc(T, "average")[0], ar.ahc(S, "average")[0])
    # stops: a threshold ON a height executes that merge; min_clusters; labels rank clusters by smallest member
    rec, done, ncl, labels = ar.ahc(S, "average", threshold=1.5)
    assert done == 3 and ncl == 2 and labels.tolist() == [0, 0, 0, 0, 1] and rec[3]["a"] == -1 and np.isnan(rec[3]["value"])
    rec, done, ncl, labels = ar.ahc(S, "average", threshold=np.nextafter(1.5, 2.0))
    assert done == 2 and labels.tolist() == [0, 0, 1, 1, 2]
    rec, done, ncl, labels = ar.ahc(S, "average", min_clusters=4)
    assert done == 1 and labels.tolist() == [0, 0, 1, 2, 3]
    assert ar.ahc(S, "average", min_clusters=8)[1] == 0
    # a tie between (0, 3) and (1, 2): row-major order decides; then (0, 1) against (0, 2), equal again
    S = np.array([[0, 1, 1, 5], [1, 0, 5, 1], [1, 5, 0, 1], [1, 1, 1, 0]], np.float32)
    rec = ar.ahc(S, "single")[0]
    assert [(r["a"], r["b"]) for r in rec] == [(0, 3), (1, 2), (0, 1)]
    for n in (0, 1):
        rec, done, ncl, labels = ar.ahc(np.zeros((n, n), np.float32))
        assert rec.size == 0 and done == 0 and ncl == n and labels.tolist() == [0] * n


@pytest.mark.parametrize("linkage", LINKS)
def test_cut_of_the_full_dendrogram_equals_a_run_with_that_threshold(linkage):
    rng = np.random.default_rng(8)
    for S in (ar.int_matrix(37, 1), rng.standard_normal((41, 41)).astype(np.float32)):
        n = S.shape[0]
        full = ar.ahc(S, linkage)[0]
        assert (np.diff(full["value"]) <= 0).all()          # reducible: the heights never increase
        for t in [full["value"][k] for k in (0, 5, 20, n - 2)] + [-3.5, 0.25, 1e9, -1e9]:
            rec, done, ncl, labels = ar.ahc(S, linkage, threshold=t)
            assert np.array_equal(ar.cut(full, n, threshold=t), labels)
            assert np.array_equal(full[:done], rec[:done]) and done == (full["value"] >= t).sum()


def test_clustering_cut_is_the_twins():
    """cluster.Clustering.cut on the twin's records of a ragged batch, rows in a scrambled caller order."""
    from neuralplda_amd import cluster
    rng = np.random.default_rng(2)
    mats = [ar.int_matrix(n, 4) for n in (0, 7, 1, 12)]
    rec, done, ncl, labels = ar.batch(mats, "average")
    offsets = np.array([0, 0, 7, 8, 20], np.int64)
    order = rng.permutation(20).astype(np.int64)
    full = cluster.Clustering(np.zeros(20, np.int64), ncl, rec, offsets, order, done)
    for kw in (dict(threshold=2.0), dict(n_clusters=3), dict(threshold=-1.0, n_clusters=2), dict()):
        got = full.cut(**kw)
        want, base = np.empty(20, np.int64), 0
        for p, m in enumerate(mats):
            lab = ar.cut(ar.ahc(m, "average")[0], m.shape[0], kw.get("threshold"), kw.get("n_clusters"))
            want[order[offsets[p]:offsets[p + 1]]] = base + lab
            assert got.n_clusters[p] == (lab.max() + 1 if lab.size else 0)
            base += int(got.n_clusters[p])
        assert np.array_equal(got.labels, want)
    names = full.cut(n_clusters=3).spk2utt([f"u{i}" for i in range(20)])
    assert [n for n, _ in names] == [f"c{c:04d}" for c in range(3 + 1 + 3)] and sorted(u for _, us in names for u in us) == sorted(f"u{i}" for i in range(20))
    with pytest.raises(ValueError):
        full.cut(threshold=float("nan"))
    with pytest.raises(ValueError):
        full.cut(n_clusters=0)


def test_exact_inputs_are_exact():
    """Integer matrices: every numerator the clustering can form is an integer below 2^53, so fp64 sums are exact in any
    order — the same heights come out when the members' scores are summed afresh in another order."""
    for S in (ar.int_matrix(70, 2), ar.equal_matrix(33), ar.ordered_matrix(1025), ar.ordered_matrix(40, False)):
        n = S.shape[0]
        assert np.array_equal(S, S.T) and np.array_equal(S, np.round(S)) and ar.exactness_bound(S, n) < 2.0 ** 53
        assert np.abs(S).max() < 2.0 ** 24
    S = ar.int_matrix(70, 2)
    rec = ar.ahc(S, "average")[0]
    members = {i: [i] for i in range(70)}
    for r in rec:
        A, B = members[r["a"]], members.pop(r["b"])
        total = sum(float(S[i, j]) for i in reversed(A) for j in reversed(B))
        assert r["value"] == total / float(len(A) * len(B))
        members[r["a"]] = A + B
    _, counts = np.unique(rec["value"], return_counts=True)
    assert counts.max() >= 2                                 # executed heights tie


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_declared_names_are_present(hip_lib):
    from neuralplda_amd import _lib
    names = ["nplda_score_matrix_bytes", "nplda_score_matrix_f32", "nplda_ahc_workspace_bytes", "nplda_ahc_small_n", "nplda_ahc_max_n", "nplda_ahc_block", "nplda_ahc_f32"]
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(hip_lib, n) and re.search(r"\b%s\(" % n, hdr), n
    assert hip_lib.nplda_abi_version() == 4
    assert hip_lib.nplda_ahc_max_n() == 16384 and hip_lib.nplda_ahc_block() % 64 == 0 and 64 <= hip_lib.nplda_ahc_block() <= 1024
    assert hip_lib.nplda_ahc_block() < hip_lib.nplda_ahc_small_n() < hip_lib.nplda_ahc_max_n()
    assert "typedef struct nplda_ahc_merge" in hdr and ar.MERGE_DTYPE.itemsize == 24


def _offs(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_abi_sizes_and_argument_checks(hip_lib):
    EINVAL, EUNSUP, ENOSPC = -22, -95, -28
    L = hip_lib
    dummy = ctypes.create_string_buffer(4096)
    p16 = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40
    good = _offs(0, 0, 5, 6, 6, 16)
    maxn = L.nplda_ahc_max_n()
    assert L.nplda_score_matrix_bytes(good, 5) == 4 * (25 + 1 + 100)
    need = L.nplda_ahc_workspace_bytes(good, 5)
    assert need >= 8 * (25 + 1 + 100) + 24 * 16 and need % 256 == 0
    assert L.nplda_ahc_workspace_bytes(_offs(0, maxn), 1) >= 8 * maxn * maxn
    assert L.nplda_ahc_workspace_bytes(_offs(0), 0) > 0 and L.nplda_score_matrix_bytes(_offs(0), 0) == 0
    for bad, P in ((_offs(0, 5, 4), 2), (_offs(1, 5), 1), (_offs(0, maxn + 1), 1), (good, -1)):
        assert L.nplda_ahc_workspace_bytes(bad, P) == 0 and L.nplda_score_matrix_bytes(bad, P) == 0
    assert L.nplda_ahc_workspace_bytes(None, 1) == 0

    def ahc(S=p16, oh=good, od=p16, P=5, linkage=0, thr=0.0, minc=1, merges=p16, nm=p16, nc=p16, labels=p16, ws=p16, wsb=big):
        return L.nplda_ahc_f32(S, oh, od, P, linkage, thr, minc, merges, nm, nc, labels, ws, wsb, None)

    assert ahc(P=0) == 0 and ahc(P=0, S=None, oh=None, od=None, merges=None, nm=None, nc=None, labels=None, ws=None) == 0
    for kw in (dict(S=None), dict(oh=None), dict(od=None), dict(merges=None), dict(nm=None), dict(nc=None), dict(labels=None),
               dict(ws=None)):
        assert ahc(**kw) == EINVAL, kw
    assert ahc(thr=float("nan")) == EINVAL and ahc(minc=0) == EINVAL and ahc(minc=-3) == EINVAL
    assert ahc(linkage=3) == EINVAL and ahc(linkage=-1) == EINVAL
    assert ahc(oh=_offs(0, 5, 4), P=2) == EINVAL and ahc(oh=_offs(2, 5), P=1) == EINVAL and ahc(P=-1) == EINVAL
    assert ahc(oh=_offs(0, maxn + 1), P=1) == EUNSUP and ahc(P=1 << 22) == EUNSUP
    assert ahc(wsb=need - 1) == ENOSPC and ahc(wsb=0) == ENOSPC
    assert ahc(ws=p16 + 8) == EINVAL and ahc(merges=p16 + 4) == EINVAL

    def sm(z=p16, ldz=160, q=p16, oh=good, od=p16, P=5, packed=p16, D0=512, D1=150, D2=150, out=p16):
        return L.nplda_score_matrix_f32(z, ldz, q, oh, od, P, packed, D0, D1, D2, out, None)

    assert sm(P=0) == 0 and sm(P=0, z=None, q=None, oh=None, od=None, packed=None, out=None) == 0
    assert sm(oh=_offs(0, 0, 0), P=2, z=None, q=None, out=None) == 0             # an empty table
    for kw in (dict(z=None), dict(q=None), dict(oh=None), dict(od=None), dict(packed=None), dict(out=None)):
        assert sm(**kw) == EINVAL, kw
    assert sm(oh=_offs(0, 5, 4), P=2) == EINVAL and sm(P=-1) == EINVAL and sm(D2=0) == EINVAL and sm(D0=510) == EINVAL
    assert sm(ldz=150) == EINVAL and sm(ldz=162) == EINVAL and sm(z=p16 + 4) == EINVAL and sm(packed=p16 + 8) == EINVAL
    assert sm(D2=193, ldz=208) == EUNSUP and sm(oh=_offs(0, maxn + 1), P=1) == EUNSUP


# ---- kernel resources --------------------------------------------------------------------------------------------------------------

def test_resource_budget_of_the_ahc_kernels():
    """design/k21_ahc.md: no scratch in either kernel; the score kernel keeps two blocks of four waves per CU (at most 256
    registers) with the 16-row stage as its only LDS; the clustering block of 1024 threads is sixteen waves on one CU, four
    per SIMD (at most 128 registers), with a few hundred bytes of LDS."""
    res = _resources("nplda_ahc.hip")
    score = {k: v for k, v in res.items() if "score_matrix_kernelILi" in k}
    assert len(score) == 6, sorted(res)
    for name, v in score.items():
        nb = int(re.search(r"score_matrix_kernelILi(\d+)E", name).group(1))
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (name, v)
        assert v["LDS"] <= 16 * (16 * nb + 4) * 4 + 64 + 48 * 8 + 64, (name, v)
    rest = {k: v for k, v in res.items() if k not in score}
    assert len(rest) == 1 and "ahc_kernel" in next(iter(rest)), sorted(res)
    for name, v in rest.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 4 and v["VGPRs"] + v["AGPRs"] <= 128 and v["LDS"] <= 1024, (name, v)
