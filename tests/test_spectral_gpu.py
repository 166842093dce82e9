"""ops.spectral / ops.spectral_kmeans (csrc/nplda_spectral.hip), cluster.spectral_cluster and diarize(clusterer="spectral") on
the GPU, stage by stage against the numpy twin of tests/spectral_ref.py: the graph bit for bit, the spectrum in units of the
float64 twin's own error against its long-double run (recorded in tests/golden/spectral_spectrum.npz), the count and the
k-means bit for bit on the DEVICE's eigenvalues and eigenvectors, so that no test rests on a near-tie rounding could move."""
import os

import numpy as np
import pytest
import torch

from tests import spectral_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def run(mats, neighbours, **kw):
    from neuralplda_amd import ops
    offs = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    flat = np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0, np.float32)
    return ops.spectral(_dev(flat.astype(np.float32)), offs, neighbours, **kw), offs


# ---- 1. the graph ---------------------------------------------------------------------------------------------------------------------

RAGGED = [0, 1, 2, 3, 17, 64, 65, 130, 0]


@pytest.mark.parametrize("kind", ["planted", "ties"])
def test_graph_is_the_twins_bit_for_bit(kind):
    cands = (1, 4, 200)
    mats = [sr.planted(n, 2 if n >= 4 else 1, 3.0, 50 + n)[0] if kind == "planted" else sr.tie_heavy(n, 60 + n) for n in RAGGED]
    res, offs = run(mats, cands, return_embedding=True, return_degrees=True)
    ev = res.eigenvalues.cpu().numpy()
    for p, S in enumerate(mats):
        n = S.shape[0]
        for ci, c in enumerate(cands):
            d = res.degrees_of(p, ci).cpu().numpy()
            want = sr.graph(S, c)[1]
            assert np.array_equal(bits(d), bits(want)), (kind, n, c)
            if n == 0:
                assert np.isnan(ev[p, ci]).all()
    # the trace: the eigenvalues of a whole spectrum (n <= max_clusters + 1 = 65 rows: all are returned) sum to the degree sum,
    # an integer or half-integer; each computed eigenvalue carries a few 2^-53 ||L||_F and the sum here its own rounding
    for p, S in enumerate(mats):
        n = S.shape[0]
        if 1 <= n <= 65:
            for ci, c in enumerate(cands):
                lam = ev[p, ci, :n]
                L, d = sr.graph(S, c)
                dsum = float(d.sum())
                assert abs(lam.sum() - dsum) <= n * (5 * 2.0 ** -53 * np.linalg.norm(L) + np.finfo(np.float64).eps * dsum), (kind, n, c)
                assert ev[p, ci, -1] == lam[-1]


# ---- 2. the spectrum --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", sr.GOLDEN))


def test_sizes_straddle_the_kernels_paths(hip_lib):
    small, blk, sblk = hip_lib.nplda_spectral_small_n(), hip_lib.nplda_spectral_block(), hip_lib.nplda_spectral_small_block()
    ns = sr.SPECTRUM_NS
    assert small in ns and small + 1 in ns and 63 in ns and 64 in ns and 65 in ns
    assert max(ns) > sblk and (max(ns) // 2) ** 2 > blk                     # more pieces than threads: the strided loops wrap
    assert hip_lib.nplda_spectral_max_n() >= 2048


@pytest.mark.parametrize("n", sr.SPECTRUM_NS)
def test_spectrum_in_units_of_the_twins_error(n, golden, hip_lib):
    """Eigenvalues: |device - long double| in units of max(|float64 twin - long double|, 2^-53 ||L||_F) per eigenvalue, gates
    3 rms / 5 max.  Eigenvectors: ||L V - V D||_F and ||V^T V - I||_F of the device's K + 1 columns against the same two
    quantities of numpy.linalg.eigh's columns, gate 4 x.  Measured on an MI355X: eigenvalues 0.19 - 0.47 rms and at most 1.00
    max at every size (the device runs the twin's operations in the twin's order); residual 0.8 - 1.4 x LAPACK's,
    orthogonality 0.7 - 2.1 x (the largest at n = 257); 7 - 10 sweeps."""
    S = sr.spectrum_case(n)
    res, _ = run([S], sr.SPECTRUM_CANDIDATES, return_vectors=True)
    ev = res.eigenvalues.cpu().numpy()[0]
    assert (res.converged.cpu().numpy() == 1).all()
    sweeps = res.n_sweeps.cpu().numpy()
    assert (sweeps >= 1).all() and (sweeps <= hip_lib.nplda_spectral_max_sweeps()).all()
    K = min(64, n - 1)
    for ci, c in enumerate(sr.SPECTRUM_CANDIDATES):
        L = sr.graph(S, c)[0]
        hi, lo, f64 = golden[f"hi_{n}_{c}"], golden[f"lo_{n}_{c}"], golden[f"f64_{n}_{c}"]
        idx = np.concatenate([np.arange(K + 1), [n - 1]])
        got = np.concatenate([ev[ci, :K + 1], [ev[ci, -1]]])
        unit = np.maximum(np.abs((f64[idx] - hi[idx]) - lo[idx]), 2.0 ** -53 * np.linalg.norm(L))
        err = np.abs((got - hi[idx]) - lo[idx]) / unit
        rms, mx = float(np.sqrt((err ** 2).mean())), float(err.max())
        V = res.vectors_of(0, ci).cpu().numpy().T                      # columns
        lam = ev[ci, :K + 1]
        w, Q = np.linalg.eigh(L)
        Q = Q[:, :K + 1]
        r_dev, o_dev = np.linalg.norm(L @ V - V * lam), np.linalg.norm(V.T @ V - np.eye(K + 1))
        r_lap, o_lap = np.linalg.norm(L @ Q - Q * w[:K + 1]), np.linalg.norm(Q.T @ Q - np.eye(K + 1))
        floor = np.finfo(np.float64).eps * np.linalg.norm(L)
        print(f"n = {n} c = {c}: eigenvalues {rms:.2f} rms {mx:.2f} max units, sweeps {sweeps[0, ci]}; residual {r_dev:.2e} "
              f"(eigh {r_lap:.2e}), orthogonality {o_dev:.2e} (eigh {o_lap:.2e})")
        assert rms <= 3.0 and mx <= 5.0, (n, c, rms, mx)
        assert r_dev <= 4.0 * max(r_lap, floor) and o_dev <= 4.0 * max(o_lap, np.finfo(np.float64).eps), (n, c)


# ---- 3. the count and the choice --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(min_clusters=2, max_clusters=5), dict(min_clusters=3, max_clusters=3)])
def test_count_and_choice_on_the_devices_eigenvalues(kw):
    cands = (1, 4, 200)
    mats = [sr.planted(n, 3 if n >= 6 else 1, 3.0, 70 + n)[0] for n in RAGGED]
    res, offs = run(mats, cands, **kw)
    ev, ks, ratio = res.eigenvalues.cpu().numpy(), res.kstar.cpu().numpy(), res.ratio.cpu().numpy()
    chosen = res.chosen.cpu().numpy()
    mc = kw.get("max_clusters", 64)
    assert ev.shape == (len(mats), 3, mc + 2)
    for p, S in enumerate(mats):
        n = S.shape[0]
        want = [sr.choose(ev[p, ci], c, n, kw.get("min_clusters", 1), mc) for ci, c in enumerate(cands)]
        assert [w[0] for w in want] == ks[p].tolist(), (n, kw)
        assert np.array_equal(bits(np.array([w[1] for w in want], np.float64)), bits(ratio[p])), (n, kw)
        assert chosen[p] == int(np.argmin([w[1] for w in want])), (n, kw)
        if n >= 2 and n - 1 <= 4:
            assert ev[p, 1].tobytes() == ev[p, 2].tobytes() and chosen[p] != 2     # a repeated candidate never wins


# ---- 4. the k-means -----------------------------------------------------------------------------------------------------------------------

def test_kmeans_of_the_call_on_the_devices_embedding():
    cands = (4, 8, 200)
    mats = [sr.planted(n, 3 if n >= 6 else 1, 3.0, 80 + n)[0] for n in RAGGED]
    res, offs = run(mats, cands, return_embedding=True, max_clusters=16)
    labels, ncl, iters = res.labels.cpu().numpy(), res.n_clusters.cpu().numpy(), res.n_kmeans_iters.cpu().numpy()
    for p, S in enumerate(mats):
        n = S.shape[0]
        if n == 0:
            assert ncl[p] == 0 and iters[p] == 0
            continue
        E = res.embedding_of(p).cpu().numpy()
        assert E.shape == (n, res.k_of(p))
        assert np.abs(np.linalg.norm(E, axis=0) - 1.0).max() <= 4 * np.finfo(np.float64).eps
        wl, wn, wi = sr.kmeans(E, E.shape[1])
        assert np.array_equal(labels[offs[p]:offs[p + 1]], wl) and ncl[p] == wn and iters[p] == wi, n


@pytest.mark.parametrize("k,iters", [(2, None), (5, None), (9, None), (1, 1)])
def test_kmeans_on_random_rows(k, iters):
    from neuralplda_amd import ops
    rng = np.random.default_rng(21)
    E = rng.standard_normal((130, 5))
    for max_iters in (100, 1):
        lab, ncl, it = ops.spectral_kmeans(_dev(E), None, k, max_iters)
        wl, wn, wi = sr.kmeans(E, k, max_iters)
        assert np.array_equal(lab.cpu().numpy(), wl) and ncl.item() == wn and it.item() == wi, (k, max_iters)
        if max_iters == 100 and k > 1:
            assert wi >= 3                                                        # the loop ran


def test_kmeans_ragged_k_equals_n_and_empty_centres():
    from neuralplda_amd import ops
    rng = np.random.default_rng(22)
    sizes = [0, 1, 7, 64, 3, 300]
    E = rng.standard_normal((sum(sizes), 3))
    E[8 + 64:8 + 64 + 3] = E[8 + 64]                                              # three equal rows: centres without rows
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for k in (7, 64):
        lab, ncl, it = ops.spectral_kmeans(_dev(E), offs, k)
        lab, ncl, it = lab.cpu().numpy(), ncl.cpu().numpy(), it.cpu().numpy()
        for p, n in enumerate(sizes):
            wl, wn, wi = sr.kmeans(E[offs[p]:offs[p + 1]], k)
            assert np.array_equal(lab[offs[p]:offs[p + 1]], wl) and ncl[p] == wn and it[p] == wi, (k, n)
        assert ncl[2] == 7 and ncl[4] == 1
    assert ncl[3] == 64


# ---- 4b. a batch with more problems than a block has threads -----------------------------------------------------------------------------

def per_problem(res, offs):
    """Every output of ops.spectral (embedding, degrees and vectors included) on the host, split by problem."""
    host = lambda t: t.cpu().numpy()  # noqa: E731
    ev, ks, ratio, sw, cv = host(res.eigenvalues), host(res.kstar), host(res.ratio), host(res.n_sweeps), host(res.converged)
    chosen, ncl, it, lab = host(res.chosen), host(res.n_clusters), host(res.n_kmeans_iters), host(res.labels)
    emb, deg, vec = host(res.embedding).reshape(-1), host(res.degrees), host(res.vectors)
    n, C, mc = np.diff(offs), len(res.neighbours), res.max_clusters
    voff = np.concatenate([[0], np.cumsum(C * np.minimum(mc + 1, n) * n)])
    out = []
    for p in range(n.size):
        r0, k = int(offs[p]), min(int(ks[p, chosen[p]]), int(n[p]))
        out.append((ev[p], ks[p], ratio[p], sw[p], cv[p], chosen[p:p + 1], ncl[p:p + 1], it[p:p + 1], lab[r0:r0 + n[p]],
                    emb[r0 * mc:r0 * mc + n[p] * k], deg[r0 * C:(r0 + n[p]) * C], vec[voff[p]:voff[p + 1]]))
    return out


def test_batch_past_the_block_equals_the_single_runs_bit_for_bit():
    """P = 300 problems against blocks of 256 threads (graph, small eigensolver, finish, k-means): where a problem's matrix,
    workspace and vectors start is a sum over the problems in front of it, and from problem 256 on a thread of that sum adds
    more than one term.  Fifteen distinct tiny problems in turn (0, 1, 2, 3, 5 rows) and one of 20 rows last, whose starts
    depend on every term: every problem's outputs equal, bit for bit, those of a call of its own on the same data."""
    from neuralplda_amd import ops
    P, cands = 300, (1, 4, 200)
    sizes = [(0, 1, 2, 3, 5)[i % 5] for i in range(15)] + [20]
    pick = [p % 15 for p in range(P - 1)] + [15]
    kw = dict(return_embedding=True, return_degrees=True, return_vectors=True)
    mats = [sr.planted(n, 2 if n >= 4 else 1, 3.0, 300 + i)[0] for i, n in enumerate(sizes)]
    res, offs = run([mats[i] for i in pick], cands, **kw)
    got = per_problem(res, offs)
    singles = [per_problem(*run([m], cands, **kw))[0] for m in mats]
    assert singles[15][6][0] >= 2 and singles[15][4].all()                        # the last problem: clusters, every cell converged
    for p, i in enumerate(pick):
        assert len(got[p]) == len(singles[i]) == 12
        for f, (a, b) in enumerate(zip(got[p], singles[i])):
            assert np.array_equal(bits(a), bits(b)), (p, f)
    # ops.spectral_kmeans on rows that repeat with the problems
    rng = np.random.default_rng(23)
    E = [rng.standard_normal((n, 3)) for n in sizes]
    rows = np.concatenate([[0], np.cumsum([sizes[i] for i in pick])]).astype(np.int64)
    lab, ncl, it = (t.cpu().numpy() for t in ops.spectral_kmeans(_dev(np.concatenate([E[i] for i in pick])), rows, 4))
    alone = [[t.cpu().numpy() for t in ops.spectral_kmeans(_dev(e), [0, e.shape[0]], 4)] for e in E]
    assert alone[15][1][0] == 4
    for p, i in enumerate(pick):
        assert np.array_equal(lab[rows[p]:rows[p + 1]], alone[i][0]) and ncl[p] == alone[i][1][0] and it[p] == alone[i][2][0], p


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------------

class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 170, 170
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


@pytest.fixture(scope="module")
def kaldi():
    from neuralplda_amd import models
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_kaldi_params.npz"))
    m = models.NeuralPlda(NC())
    sd = m.state_dict()
    for k, a in (("centering_and_LDA.weight", "W1"), ("centering_and_LDA.bias", "b1"), ("centering_and_wccn_plda.weight", "W2"),
                 ("centering_and_wccn_plda.bias", "b2"), ("P_sqrt", "P_sqrt"), ("Q", "Q")):
        sd[k].copy_(torch.from_numpy(g1[a]))
    return m.to(DEV), g1


def planted_xvectors(g1, n, clusters, seed, equal=True, noise=1.0):
    """x-vectors of `clusters` synthetic speakers under the Kaldi-initialised model, contiguous, sized as sr.planted does;
    noise: the within-speaker spread (the counterpart of a smaller separation)."""
    from tests import synth
    truth = sr.planted(n, clusters, 0.0, seed, equal)[1]
    U = int(np.bincount(truth).max())
    x, spk = synth.speaker_structured_xvectors(g1["W1"], g1["b1"], g1["W2"].astype(np.float64), g1["plda_mean"], g1["psi"],
                                               clusters, U, noise, 100 + seed)
    rows = np.concatenate([np.flatnonzero(spk == s)[:(truth == s).sum()] for s in range(clusters)])
    return x[rows], truth


LADDER = (2, 3, 4, 6, 8, 12, 16, 24, 32)
CASES = [(17, 2, (4, 6, 8), True, 1.0), (24, 3, (4, 6), True, 1.0), (33, 2, (4, 6, 8, 12), True, 1.0)] + \
        [(n, cl, LADDER, False, noise) for n, cl, noise in ((64, 3, 1.0), (65, 4, 1.0), (130, 5, 1.0), (130, 1, 1.0), (130, 5, 2.0))]


def same_partition(a, b):
    return np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])


@pytest.mark.parametrize("n,clusters,cands,equal,noise", CASES)
def test_cluster_end_to_end_on_planted_speakers(kaldi, n, clusters, cands, equal, noise):
    from neuralplda_amd import cluster, ops
    from neuralplda_amd.adaptive_score_normalization import _model_params
    from neuralplda_amd.search import embed_table
    m, g1 = kaldi
    x, truth = planted_xvectors(g1, n, clusters, n + clusters, equal, noise)
    X = _dev(x)
    got = m.spectral_cluster(X, neighbours=list(cands), max_clusters=16)
    with torch.no_grad():
        packed = ops.pack_params(*_model_params(m, torch.device(DEV)))
    z, q = embed_table(m, X, packed)
    S = ops.score_matrix(z, q, packed).cpu().numpy()
    want = sr.spectral(S, cands, max_clusters=16)
    margin = want["margins"][want["chosen"]]
    print(f"n = {n}, {clusters} speakers: chosen c = {cands[want['chosen']]}, k = {want['k']}, gap margin / l_n = {margin:.3f}")
    assert margin > 1e-3
    assert got.chosen[0] == want["chosen"] and got.neighbours[0] == cands[want["chosen"]]
    assert got.n_clusters[0] == want["n_clusters"] == clusters and got.kstar[0, want["chosen"]] == want["k"]
    assert same_partition(got.labels, want["labels"]) and same_partition(got.labels, truth)
    assert np.array_equal(got.labels, want["labels"])              # (one group: the labels themselves)


def test_groups_workspace_limit_repeats_and_capture(kaldi):
    from neuralplda_amd import cluster, ops
    m, g1 = kaldi
    parts = [planted_xvectors(g1, n, cl, 7 * n, True) for n, cl in ((17, 2), (24, 3), (33, 2), (1, 1))]
    x = np.concatenate([p[0] for p in parts])
    groups = np.concatenate([np.full(p[0].shape[0], g) for g, p in enumerate(parts)])
    cands = [4, 6, 8]
    base = cluster.spectral_cluster(m, _dev(x), groups=groups, neighbours=cands)
    assert base.n_clusters.tolist() == [2, 3, 2, 1]
    for g, p in enumerate(parts):
        assert same_partition(base.labels[groups == g], p[1])
    assert base.labels.max() + 1 == 8 and base.ratio.shape == (4, 3) and base.eigenvalues.shape == (4, 3, 18)
    # the groups' rows interleaved (each group's own order kept): every row keeps its cluster
    seq = np.random.default_rng(3).permutation(groups)
    nxt = {g: iter(np.flatnonzero(groups == g).tolist()) for g in range(len(parts))}
    perm = np.array([next(nxt[g]) for g in seq.tolist()])
    mixed = cluster.spectral_cluster(m, _dev(x[perm]), groups=groups[perm], neighbours=cands)
    assert np.array_equal(mixed.labels, base.labels[perm]) and mixed.ratio.tobytes() == base.ratio.tobytes()
    # a workspace limit that holds one group at a time; and the same call again
    limit = ops.spectral_workspace_bytes([0, 33], 3)
    assert limit < ops.spectral_workspace_bytes([0, 17, 41, 74, 75], 3)
    for other in (cluster.spectral_cluster(m, _dev(x), groups=groups, neighbours=cands, workspace_bytes=limit),
                  cluster.spectral_cluster(m, _dev(x), groups=groups, neighbours=cands)):
        assert np.array_equal(other.labels, base.labels)
        for name in ("eigenvalues", "ratio", "kstar", "n_sweeps", "n_kmeans_iters", "chosen"):
            assert getattr(other, name).tobytes() == getattr(base, name).tobytes(), name
    with pytest.raises(ValueError):
        cluster.spectral_cluster(m, _dev(x), groups=groups, neighbours=cands, workspace_bytes=1024)
    one = cluster.spectral_cluster(m, _dev(x), groups=groups, neighbours=6)
    assert one.neighbours.tolist() == [6] * 4 and one.ratio.shape == (4, 1)
    names = base.spk2utt([f"u{i}" for i in range(x.shape[0])])
    assert len(names) == 8 and names[0][0] == "c0000"
    # under graph capture
    mats = [sr.planted(n, 2, 3.0, 90 + n)[0] for n in (17, 130, 0, 33)]
    offs = ops.RaggedOffsets(np.concatenate([[0], np.cumsum([a.shape[0] for a in mats])]), torch.device(DEV))
    flat = _dev(np.concatenate([a.reshape(-1) for a in mats]))
    fields = ("eigenvalues", "ratio", "kstar", "n_sweeps", "converged", "chosen", "n_clusters", "n_kmeans_iters", "labels")
    eager = ops.spectral(flat, offs, (4, 8))
    a = [getattr(eager, f).cpu().numpy().tobytes() for f in fields]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.spectral(flat, offs, (4, 8))
    for _ in range(2):
        for f in fields:
            getattr(out, f).zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert [getattr(out, f).cpu().numpy().tobytes() for f in fields] == a


def test_arguments_raise():
    from neuralplda_amd import models, ops
    S = _dev(sr.planted(5, 1, 3.0, 1)[0])
    for bad in ([], [0, 2], [3, 3], [4, 2], list(range(1, 18)), [1.5]):
        with pytest.raises(ValueError):
            ops.spectral(S, None, bad)
    for kw in (dict(min_clusters=0), dict(min_clusters=3, max_clusters=2), dict(max_clusters=65), dict(max_iters=0)):
        with pytest.raises(ValueError):
            ops.spectral(S, None, (2,), **kw)
    with pytest.raises(ValueError):
        ops.spectral(torch.zeros(2049 * 2049, device=DEV), [0, 2049], (2,))
    empty = ops.spectral(torch.zeros(0, device=DEV), [0], (2,))
    assert empty.labels.numel() == 0 and empty.ratio.shape == (0, 1)
    for cls in (models.DPlda, models.GaussianBackend):
        with pytest.raises(NotImplementedError):
            cls(NC).spectral_cluster(torch.zeros(4, 512, device=DEV))


# ---- 6. the diarizer ------------------------------------------------------------------------------------------------------------------------

from tests.test_xvec_windows_gpu import NC as NC150, extractors, params  # noqa: E402,F401  (module-scoped fixtures)


def test_diarize_with_the_spectral_clusterer(extractors):  # noqa: F811
    from neuralplda_amd import cluster, diarize, models
    from tests import xvec_ref
    from tests.test_diarize_cpu import twin_turns
    ext = extractors["std"]
    head = xvec_ref.load_into(models.NeuralPlda(NC150()), xvec_ref.make_head()).to(DEV)
    lengths = [600, 580]
    rng = np.random.default_rng(8)
    level = np.repeat(rng.standard_normal((8, 30)), 150, axis=0)[:sum(lengths)]
    frames = torch.from_numpy((level + rng.standard_normal((sum(lengths), 30))).astype(np.float32)).to(DEV)
    segs = [np.array([[20, 280], [330, 590]]), np.array([[50, 575]])]
    kw = dict(segments=segs, window=60, shift=30)
    opts = dict(neighbours=[2, 4, 6], max_clusters=4)
    res = diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], clusterer="spectral", spectral=opts, **kw)
    assert isinstance(res.clustering, cluster.SpectralClustering)
    c = cluster.spectral_cluster(head, res.xvectors, groups=res.windows[:, 0], **opts)
    assert np.array_equal(res.labels, c.labels) and np.array_equal(res.clustering.ratio, c.ratio)
    assert (c.n_clusters >= 1).all() and (c.n_clusters <= 4).all() and set(c.neighbours.tolist()) <= {2, 4, 6}
    assert np.array_equal(res.turns, twin_turns(res.windows, c.labels))
    with pytest.raises(ValueError, match="no dendrogram to cut"):
        diarize.sweep_thresholds(res, res.turns, [0.0])
    # the default clusterer, named or not, is the same call bit for bit
    a = diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], threshold=float("-inf"), min_clusters=3, **kw)
    b = diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], threshold=float("-inf"), min_clusters=3, clusterer="ahc", **kw)
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.turns, b.turns)
    assert a.clustering.merges.tobytes() == b.clustering.merges.tobytes() and torch.equal(a.xvectors, b.xvectors)
    with pytest.raises(ValueError):
        diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], clusterer="kmeans", **kw)
    with pytest.raises(ValueError):
        diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], spectral=opts, **kw)
    # the VB-HMM takes the result as its initial clustering, and so does diarize
    psi = np.random.default_rng(9).uniform(0.5, 4.0, 150)
    vb = dict(Fa=0.5, Fb=5.0, loop_prob=0.9, max_iters=10)
    r = cluster.vb_refine(head, res.xvectors, c, psi, groups=res.windows[:, 0], **vb)
    r2 = cluster.vb_refine(head, res.xvectors, c.labels, psi, groups=res.windows[:, 0], **vb)
    assert np.array_equal(r.labels, r2.labels) and len(r) == len(c)
    res2 = diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], clusterer="spectral", spectral=opts, vb_psi=psi, vb=vb, **kw)
    assert np.array_equal(res2.labels, r.labels)
