"""Spectral clustering without a GPU: the numpy twin of tests/spectral_ref.py stage by stage (the graph against a brute-force
sort, the Jacobi sweep against LAPACK, the k-means against a vectorised restatement), the planted partitions it must recover,
the recorded long-double spectra, the argument checks of the C entry points (status codes come before any launch), the
declared names and the resource budget of csrc/nplda_spectral.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import spectral_ref as sr
from tests.test_topk_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_partition(a, b):
    return np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])


# ---- the twin ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planted", "ties"])
def test_graph_against_a_brute_force_sort(kind):
    for n in (1, 2, 3, 9, 40):
        S = sr.planted(n, 2 if n > 3 else 1, 3.0, n)[0] if kind == "planted" else sr.tie_heavy(n, n)
        if kind == "ties" and n == 40:
            assert np.unique(S).size <= 3 and np.signbit(S[S == 0]).any() and not np.signbit(S[S == 0]).all()
        for c in (1, 3, 8, 100):
            L, d = sr.graph(S, c)
            m = min(c, n - 1)
            B = np.zeros((n, n))
            for i in range(n):
                cols = sorted((j for j in range(n) if j != i), key=lambda j: (-float(S[i, j]), j))   # -0.0 == +0.0
                B[i, cols[:m]] = 1
            A = (B + B.T) / 2
            assert np.array_equal(L, np.diag(A.sum(1)) - A) and np.array_equal(d, A.sum(1))
            assert np.array_equal(L * 2, np.round(L * 2)) and np.array_equal(L, L.T) and (B.sum(1) == m).all()


@pytest.mark.parametrize("n", [1, 2, 5, 16, 33, 64])
def test_jacobi_against_lapack(n):
    L = sr.graph(sr.planted(n, 3 if n >= 9 else 1, 3.0, 7 * n)[0], 4)[0]
    lam, V, sweeps, conv = sr.jacobi(L)
    assert conv and 1 <= sweeps <= 12 and lam.shape == (n,) and V.shape == (n, n)
    w = np.linalg.eigvalsh(L)
    scale = max(np.linalg.norm(L), 1.0)
    assert np.abs(lam - w).max() <= 8 * np.finfo(np.float64).eps * scale
    assert np.linalg.norm(L @ V.T - V.T * lam) <= 8 * np.finfo(np.float64).eps * scale * np.sqrt(n)
    assert np.linalg.norm(V @ V.T - np.eye(n)) <= 64 * np.finfo(np.float64).eps * np.sqrt(n)
    if n > 1:   # one zero eigenvalue per connected component, and the constant vector in their span
        assert abs(lam[0]) <= 8 * np.finfo(np.float64).eps * scale and lam[-1] > 0
    # the long-double run agrees to float64 rounding and is better than it
    ld = sr.jacobi(L, np.longdouble, vectors=False)[0]
    assert np.abs(ld - lam).max() <= 8 * np.finfo(np.float64).eps * scale
    # repeated eigenvalues: disconnected pairs, every eigenvalue 0 or 2
    S = np.full((6, 6), -5.0, np.float32)
    for a in (0, 2, 4):
        S[a, a + 1] = S[a + 1, a] = 5.0
    lam, V, _, conv = sr.jacobi(sr.graph(S, 1)[0])
    assert conv and np.allclose(lam, [0, 0, 0, 2, 2, 2], atol=1e-15) and np.linalg.norm(V @ V.T - np.eye(6)) < 1e-14


def test_choose_by_hand():
    ev = np.full(66, np.nan)
    ev[:5], ev[-1] = [0.0, 0.0, 0.5, 3.0, 3.25], 4.0
    assert sr.choose(ev, 6, 5) == (3, 6 / (2.5 / 4.0))
    assert sr.choose(ev, 6, 5, min_clusters=4) == (4, 6 / (0.25 / 4.0))
    assert sr.choose(ev, 6, 5, max_clusters=2) == (2, 6 / (0.5 / 4.0))
    assert sr.choose(ev, 6, 5, min_clusters=5) == (5, np.inf)          # no k in range
    tie = ev.copy()
    tie[:5] = [0.0, 1.0, 2.0, 2.5, 3.5]
    assert sr.choose(tie, 2, 5)[0] == 1                                 # the lowest k among equal gaps
    flat = np.full(66, np.nan)
    flat[:3], flat[-1] = 0.0, 0.0
    assert sr.choose(flat, 2, 3) == (1, np.inf) and sr.choose(flat, 2, 3, min_clusters=2) == (2, np.inf)
    assert sr.choose(ev, 2, 1) == (1, np.inf) and sr.choose(ev, 2, 0, min_clusters=3) == (1, np.inf)
    assert sr.choose(ev, 2, 2, min_clusters=3) == (2, np.inf)


@pytest.mark.parametrize("k", [1, 2, 5, 9])
def test_kmeans_against_a_vectorised_restatement(k):
    rng = np.random.default_rng(21)
    E = rng.standard_normal((130, 5))
    labels, ncl, iters = sr.kmeans(E, k)
    cen = [E[0]]
    for _ in range(1, k):
        d = np.min([((E - c) ** 2).sum(1) for c in cen], axis=0)
        cen.append(E[int(np.argmax(d))])
    cen, prev, count = np.array(cen), None, 0
    while True:
        D = ((E[:, None, :] - cen[None]) ** 2).sum(2)
        srt = np.sort(D, axis=1)
        assert k == 1 or (srt[:, 1] - srt[:, 0]).min() > 1e-9          # no near-tie for rounding to move
        asg = D.argmin(1)
        count += 1
        if prev is not None and np.array_equal(asg, prev):
            break
        prev = asg
        cen = np.array([E[asg == c].mean(0) if (asg == c).any() else cen[c] for c in range(k)])
    assert iters == count and same_partition(labels, prev) and ncl == np.unique(prev).size
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(ncl)]
    assert first == sorted(first) and labels[0] == 0
    assert iters == {1: 2, 2: 9, 5: 10, 9: 9}[k]                        # the loop runs: what this seed needs
    one = sr.kmeans(E, k, max_iters=1)
    assert one[2] == 1
    assert sr.kmeans(E[:4], 9)[1] == 4 and sr.kmeans(E[:0], 3)[1:] == (0, 0)


LADDER = (2, 3, 4, 6, 8, 12, 16, 24, 32)
PLANTED = [(17, 2, 3.0, (4, 6, 8), True), (24, 3, 3.0, (4, 6), True), (33, 2, 3.0, (4, 6, 8, 12), True),
           (64, 3, 3.0, LADDER, False), (65, 4, 3.0, LADDER, False), (130, 5, 3.0, LADDER, False), (130, 1, 3.0, LADDER, False),
           (130, 5, 1.5, LADDER, False)]


@pytest.mark.parametrize("n,clusters,sep,cands,equal", PLANTED)
def test_planted_partitions_are_recovered(n, clusters, sep, cands, equal):
    S, truth = sr.planted(n, clusters, sep, 0, equal)
    assert np.unique(truth).size == clusters and (np.diff(truth) >= 0).all()
    r = sr.spectral(S, cands, max_clusters=16)
    margin = r["margins"][r["chosen"]]
    print(f"n = {n}, {clusters} clusters, sep {sep}: chosen c = {cands[r['chosen']]}, gap margin / l_n = {margin:.2f}")
    assert margin > 1e-3
    assert r["k"] == clusters and r["n_clusters"] == clusters and same_partition(r["labels"], truth)
    assert r["converged"].all() and (r["n_sweeps"] <= sr.MAX_SWEEPS).all()
    # against LAPACK: the same count from numpy.linalg.eigh
    lam = np.linalg.eigvalsh(sr.graph(S, cands[r["chosen"]])[0])
    assert int(np.argmax(np.diff(lam[:17]))) + 1 == clusters


def test_recorded_spectra_are_the_twins():
    g = np.load(os.path.join(ROOT, "tests", "golden", sr.GOLDEN))
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "the recorded reference needs a long double wider than float64"
    for n in sr.SPECTRUM_NS:
        for c in sr.SPECTRUM_CANDIDATES:
            assert g[f"hi_{n}_{c}"].shape == (n,) and g[f"f64_{n}_{c}"].shape == (n,)
    for n in (2, 3, 17, 63):
        for c in sr.SPECTRUM_CANDIDATES:
            hi, lo, f64 = sr.spectrum_reference(n, c)
            assert np.array_equal(f64, g[f"f64_{n}_{c}"])
            assert np.abs((hi - g[f"hi_{n}_{c}"]) + (lo - g[f"lo_{n}_{c}"])).max() <= 2.0 ** -60 * max(abs(hi).max(), 1.0)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

NAMES = ["nplda_spectral_max_n", "nplda_spectral_max_k", "nplda_spectral_max_candidates", "nplda_spectral_max_sweeps",
         "nplda_spectral_block", "nplda_spectral_small_n", "nplda_spectral_small_block", "nplda_spectral_workspace_bytes",
         "nplda_spectral_f32", "nplda_spectral_kmeans_workspace_bytes", "nplda_spectral_kmeans_f64"]


def test_declared_names_are_present(hip_lib):
    from neuralplda_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(hip_lib, n) and re.search(r"\b%s\(" % n, hdr), n
    assert hip_lib.nplda_abi_version() == 4
    L = hip_lib
    assert L.nplda_spectral_max_n() >= 2048 and L.nplda_spectral_max_k() == 64 == L.nplda_vbhmm_max_speakers() == L.nplda_der_max_speakers()
    assert L.nplda_spectral_max_candidates() == 16 and L.nplda_spectral_max_sweeps() == sr.MAX_SWEEPS
    for b in (L.nplda_spectral_block(), L.nplda_spectral_small_block()):
        assert b % 64 == 0 and 64 <= b <= 1024
    assert L.nplda_spectral_small_block() < L.nplda_spectral_block() and 2 < L.nplda_spectral_small_n() < L.nplda_spectral_max_n()
    assert len(ops.SPECTRAL_NEIGHBOURS) <= 16 and list(ops.SPECTRAL_NEIGHBOURS) == sorted(set(ops.SPECTRAL_NEIGHBOURS))


def _offs(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _tab(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_abi_sizes_and_argument_checks(hip_lib):
    EINVAL, EUNSUP, ENOSPC = -22, -95, -28
    L = hip_lib
    dummy = ctypes.create_string_buffer(4096)
    p16 = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40
    good = _offs(0, 0, 5, 6, 6, 16)
    maxn = L.nplda_spectral_max_n()
    need = L.nplda_spectral_workspace_bytes(good, 5, 3)
    assert need >= 3 * 16 * (36 + 4 + 100) and need % 256 == 0
    assert L.nplda_spectral_workspace_bytes(good, 5, 6) > need
    assert L.nplda_spectral_workspace_bytes(_offs(0, maxn), 1, 1) >= 16 * maxn * maxn
    assert L.nplda_spectral_workspace_bytes(_offs(0), 0, 1) > 0 and L.nplda_spectral_kmeans_workspace_bytes(_offs(0), 0) > 0
    for bad, P in ((_offs(0, 5, 4), 2), (_offs(1, 5), 1), (_offs(0, maxn + 1), 1), (good, -1)):
        assert L.nplda_spectral_workspace_bytes(bad, P, 3) == 0 and L.nplda_spectral_kmeans_workspace_bytes(bad, P) == 0
    assert L.nplda_spectral_workspace_bytes(None, 1, 3) == 0
    assert L.nplda_spectral_workspace_bytes(good, 5, 0) == 0 and L.nplda_spectral_workspace_bytes(good, 5, 17) == 0

    def sp(S=p16, oh=good, od=p16, P=5, tab=_tab(2, 4, 8), C=3, minc=1, maxc=16, iters=100, ev=p16, ks=p16, ratio=p16, sw=p16,
           conv=p16, chosen=p16, ncl=p16, nit=p16, labels=p16, emb=None, deg=None, vec=None, ws=p16, wsb=big):
        return L.nplda_spectral_f32(S, oh, od, P, tab, C, minc, maxc, iters, ev, ks, ratio, sw, conv, chosen, ncl, nit, labels,
                                    emb, deg, vec, ws, wsb, None)

    assert sp(P=0) == 0
    assert sp(P=0, S=None, oh=None, od=None, ev=None, ks=None, ratio=None, sw=None, conv=None, chosen=None, ncl=None, nit=None,
              labels=None, ws=None) == 0
    for kw in (dict(tab=None), dict(C=0), dict(C=17), dict(tab=_tab(0, 4, 8)), dict(tab=_tab(2, 2, 8)), dict(tab=_tab(4, 2, 8)),
               dict(tab=_tab(-1, 2, 8))):
        assert sp(**kw) == EINVAL, kw
    assert sp(minc=0) == EINVAL and sp(minc=3, maxc=2) == EINVAL and sp(maxc=65) == EINVAL and sp(iters=0) == EINVAL
    assert sp(maxc=65, oh=_offs(0, maxn + 1), P=1) == EINVAL                       # the arguments before the offsets
    for kw in (dict(S=None), dict(oh=None), dict(od=None), dict(ev=None), dict(ks=None), dict(ratio=None), dict(sw=None),
               dict(conv=None), dict(chosen=None), dict(ncl=None), dict(nit=None), dict(labels=None), dict(ws=None)):
        assert sp(**kw) == EINVAL, kw
    assert sp(oh=_offs(0, 5, 4), P=2) == EINVAL and sp(oh=_offs(2, 5), P=1) == EINVAL and sp(P=-1) == EINVAL
    assert sp(oh=_offs(0, maxn + 1), P=1) == EUNSUP and sp(P=1 << 22) == EUNSUP
    assert sp(wsb=need - 1) == ENOSPC and sp(wsb=0) == ENOSPC
    assert sp(ws=p16 + 8) == EINVAL and sp(ev=p16 + 4) == EINVAL and sp(emb=p16 + 4) == EINVAL and sp(vec=p16 + 2) == EINVAL

    kneed = L.nplda_spectral_kmeans_workspace_bytes(good, 5)
    assert kneed >= 8 * 16 and kneed % 256 == 0

    def km(E=p16, oh=good, od=p16, P=5, dim=3, k=2, iters=100, ncl=p16, nit=p16, labels=p16, ws=p16, wsb=big):
        return L.nplda_spectral_kmeans_f64(E, oh, od, P, dim, k, iters, ncl, nit, labels, ws, wsb, None)

    assert km(P=0) == 0 and km(P=0, E=None, oh=None, od=None, ncl=None, nit=None, labels=None, ws=None) == 0
    assert km(dim=0) == EINVAL and km(dim=65) == EINVAL and km(k=0) == EINVAL and km(k=65) == EINVAL and km(iters=0) == EINVAL
    for kw in (dict(E=None), dict(oh=None), dict(od=None), dict(ncl=None), dict(nit=None), dict(labels=None), dict(ws=None)):
        assert km(**kw) == EINVAL, kw
    assert km(oh=_offs(0, 5, 4), P=2) == EINVAL and km(oh=_offs(0, maxn + 1), P=1) == EUNSUP
    assert km(wsb=kneed - 1) == ENOSPC and km(ws=p16 + 8) == EINVAL and km(E=p16 + 4) == EINVAL


def test_host_layer_without_a_device():
    from neuralplda_amd import cluster, diarize, ops
    assert ops.spectral_workspace_bytes([0, 5, 9], 2) > 0 and ops.spectral_workspace_bytes([0, 5, 4], 2) == 0
    offs = np.array([0, 10, 30, 35], np.int64)
    runs = cluster._spectral_batches(offs, 2, None)
    assert runs == [(0, 3)]
    limit = ops.spectral_workspace_bytes([0, 20], 2)
    assert cluster._spectral_batches(offs, 2, limit) == [(0, 1), (1, 2), (2, 3)]
    assert cluster._spectral_batches(offs, 2, ops.spectral_workspace_bytes([0, 20, 25], 2)) == [(0, 1), (1, 3)]
    with pytest.raises(ValueError, match="does not hold problem 1"):
        cluster._spectral_batches(offs, 2, ops.spectral_workspace_bytes([0, 10], 2))
    sc = cluster.SpectralClustering(np.array([0, 1, 0, 2]), np.array([2, 1]), np.array([0, 3, 4]), np.arange(4), np.array([2, 4]),
                                    np.array([1, 0]), None, None, None, None, None)
    assert sc.neighbours.tolist() == [4, 2] and len(sc) == 4
    assert sc.spk2utt("abcd") == [("c0000", ["a", "c"]), ("c0001", ["b"]), ("c0002", ["d"])]
    d = diarize.Diarization(["r"], [], np.zeros((4, 4), np.int64), [], None, sc.labels, np.zeros((0, 4), np.int64), sc, None)
    with pytest.raises(ValueError, match="no dendrogram to cut"):
        diarize.sweep_thresholds(d, np.zeros((0, 4), np.int64), [0.0])


# ---- kernel resources --------------------------------------------------------------------------------------------------------------

def test_resource_budget_of_the_spectral_kernels():
    """design/k25_spectral.md has the table: no scratch anywhere, and the registers and LDS bytes of every kernel as the note
    states them (the table is parsed from the note, so the two cannot drift apart)."""
    res = _resources("nplda_spectral.hip")
    note = open(os.path.join(ROOT, "design", "k25_spectral.md")).read()
    rows = re.findall(r"^\| `(\w+)(?:<(\d+)>)?` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", note, re.M)
    assert len(rows) == 5 == len(res), (rows, sorted(res))
    for name, tpl, threads, vgprs, lds, occ in rows:
        key = [k for k in res if name in k and (not tpl or f"ILi{tpl}E" in k)]
        assert len(key) == 1, (name, tpl, sorted(res))
        v = res[key[0]]
        assert v["ScratchSize"] == 0, (name, v)
        assert v["VGPRs"] + v["AGPRs"] == int(vgprs) and v["LDS"] == int(lds) and v["Occupancy"] == int(occ), (name, tpl, v)
        assert int(threads) // 64 <= 4 * v["Occupancy"] * 4 and v["LDS"] <= 160 * 1024
    big = [v for k, v in res.items() if "jacobi_kernelILi1024E" in k][0]
    assert big["VGPRs"] + big["AGPRs"] <= 128                            # sixteen waves of one block: four per SIMD
