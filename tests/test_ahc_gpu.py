"""ops.score_matrix / ops.ahc (csrc/nplda_ahc.hip), cluster.cluster and tools/cluster_xvectors.py on the GPU: the score matrix
against the float64 evaluation and bit for bit against ops.topk_scores; the clustering bit for bit against the numpy twin of
tests/ahc_ref.py, on exact inputs and on the kernel's own float32 matrices."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import ahc_ref as ar
from tests import topk_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LINKS = ["average", "complete", "single"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_PACKED = {}


def packed_for(P_sqrt, Q):
    """A parameter image that carries P_sqrt, Q (the layers are not used here: D0 = 16, D1 = D2, zero weights)."""
    from neuralplda_amd import ops
    key = (P_sqrt.tobytes(), Q.tobytes())
    if key not in _PACKED:
        D2 = P_sqrt.size
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        _PACKED[key] = ops.pack_params(z(D2, 16), z(D2), z(D2, D2), z(D2), _dev(P_sqrt), _dev(Q))
    return _PACKED[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def table(D2, N, seed):
    """Seeded normal z (scale 0.1, zero pad columns), P_sqrt, Q ~ U, q from the float32 inputs."""
    rng = np.random.default_rng([seed, D2, N])
    P_sqrt, Q = rng.uniform(0.2, 1.5, D2).astype(np.float32), (-rng.uniform(0.0, 1.0, D2)).astype(np.float32)
    z = np.zeros((N, tr.padded_dim(D2)), np.float32)
    z[:, :D2] = 0.1 * rng.standard_normal((N, D2))
    return z, tr.qvec(z, Q, np.float32), P_sqrt, Q


def blocks(flat, offs):
    n = np.diff(offs)
    e = np.concatenate([[0], np.cumsum(n * n)])
    return [flat[e[p]:e[p + 1]].reshape(n[p], n[p]) for p in range(n.size)]


# ---- 1. the score matrix -------------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 15, 16, 17, 63, 64, 65]
RAGGED = [0, 0, 17, 1, 0, 65, 300, 0, 64, 2, 0]      # empty problems first, in the middle and last; 300: two column chunks


@pytest.mark.parametrize("D2", [150, 170])
def test_score_matrix(D2):
    from neuralplda_amd import ops
    sizes = SIZES + RAGGED
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(offs[-1])
    z, q, P_sqrt, Q = table(D2, N, 1)
    packed = packed_for(P_sqrt, Q)
    zd, qd = _dev(z), _dev(q)
    singles = [ops.score_matrix(zd[offs[p]:offs[p + 1]], qd[offs[p]:offs[p + 1]], packed).cpu().numpy() for p in range(len(SIZES))]
    r_offs = offs[len(SIZES):] - offs[len(SIZES)]
    ragged = ops.score_matrix(zd[offs[len(SIZES)]:], qd[offs[len(SIZES)]:], packed, r_offs)
    assert ragged.shape == (int((np.diff(r_offs) ** 2).sum()),) and ragged.dtype == torch.float32
    worst = 0.0
    for p, S in enumerate(singles + blocks(ragged.cpu().numpy(), r_offs)):
        n = sizes[p]
        assert S.shape == (n, n)
        if n == 0:
            continue
        zp, qp = z[offs[p]:offs[p + 1]], q[offs[p]:offs[p + 1]]
        S64 = tr.scores(zp, qp, zp, qp, P_sqrt, np.float64)
        tol = tr.tolerance(D2, tr.magnitude(zp, qp, zp, qp, P_sqrt))
        off = ~np.eye(n, dtype=bool)
        assert (np.abs(S - S64)[off] <= tol[off]).all(), (D2, n)
        worst = max(worst, float((np.abs(S - S64) / tol)[off].max())) if n > 1 else worst
        assert np.array_equal(bits(S), bits(S.T.copy())), (D2, n, "symmetric")
        assert (bits(S)[np.diag_indices(n)] == 0).all(), (D2, n, "diagonal +0.0")
        # for i < j the bits of ops.topk_scores (row i, column j)
        k = min(128, n)
        vals, idx = ops.topk_scores(_dev(zp), _dev(qp), _dev(zp), _dev(qp), packed, k)
        vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
        rows = np.broadcast_to(np.arange(n)[:, None], idx.shape)
        up = (idx > rows)
        if n <= 128:
            assert up.sum() == n * (n - 1) // 2          # k = n: every column of every row comes back
        assert np.array_equal(bits(S[rows[up], idx[up]]), bits(vals[up])), (D2, n, "topk bits")
    print(f"D2 = {D2}: worst |S - S64| / tolerance = {worst:.4f}")


def test_score_matrix_reads_no_neighbour_and_no_pad_column():
    from neuralplda_amd import ops
    D2 = 150
    offs = np.array([0, 40, 40 + 65, 40 + 65 + 30], np.int64)
    z, q, P_sqrt, Q = table(D2, int(offs[-1]), 2)
    packed = packed_for(P_sqrt, Q)
    alone = ops.score_matrix(_dev(z[40:105]), _dev(q[40:105]), packed).cpu().numpy()
    zb, qb = z.copy(), q.copy()
    zb[:40], zb[105:], qb[:40], qb[105:] = 1e30, 1e30, 1e30, 1e30          # huge values in the neighbouring problems
    got = blocks(ops.score_matrix(_dev(zb), _dev(qb), packed, offs).cpu().numpy(), offs)[1]
    assert np.array_equal(bits(got), bits(alone))
    zp = z[40:105].copy()
    zp[:, D2:] = 1e30                                                      # finite pad columns meet P = 0
    assert np.array_equal(bits(ops.score_matrix(_dev(zp), _dev(q[40:105]), packed).cpu().numpy()), bits(alone))


# ---- 2. clustering ---------------------------------------------------------------------------------------------------------------------

def run_ahc(mats, linkage, threshold=-np.inf, min_clusters=1, offsets=None):
    from neuralplda_amd import ops
    data, offs = ar.flat(mats)
    merges, nm, nc, labels = ops.ahc(_dev(data), offs if offsets is None else offsets, linkage, threshold, min_clusters)
    assert merges.dtype == torch.uint8 and nm.dtype == nc.dtype == labels.dtype == torch.int32
    rec = merges.cpu().numpy().view(ar.MERGE_DTYPE).reshape(-1)
    return rec, nm.cpu().numpy(), nc.cpu().numpy(), labels.cpu().numpy()


def assert_same(got, want, what):
    rec, nm, nc, lab = got
    wrec, wnm, wnc, wlab = want
    assert np.array_equal(nm, wnm), (what, "n_merges", nm, wnm)
    assert np.array_equal(nc, wnc), (what, "n_clusters")
    assert rec.shape == wrec.shape
    for f in ("a", "b", "size_after", "reserved"):
        assert np.array_equal(rec[f], wrec[f]), (what, f, np.flatnonzero(rec[f] != wrec[f])[:5])
    assert np.array_equal(bits(rec["value"]), bits(wrec["value"])), (what, "value", np.flatnonzero(bits(rec["value"]) != bits(wrec["value"]))[:5])
    assert np.array_equal(lab, wlab), (what, "labels")


def check(mats, linkage, what, **kw):
    assert_same(run_ahc(mats, linkage, **kw), ar.batch(mats, linkage, **kw), (what, linkage, kw))


@pytest.mark.parametrize("linkage", LINKS)
def test_exact_small_and_structured(linkage):
    mats = [ar.int_matrix(n, 0) for n in (0, 1, 2, 3, 5, 70)]
    mats += [ar.equal_matrix(33), ar.equal_matrix(130, -2.0), ar.ordered_matrix(40), ar.ordered_matrix(200),
             ar.ordered_matrix(40, False), ar.ordered_matrix(200, False)]
    check(mats, linkage, "small and structured")
    for m in mats[:4]:                                         # n = 0, 1, 2, 3 each as a call of its own
        check([m], linkage, f"alone n = {m.shape[0]}")


@pytest.mark.parametrize("linkage", LINKS)
def test_exact_sizes_around_the_block(linkage):
    from neuralplda_amd import _lib
    B = _lib.load().nplda_ahc_block()
    check([ar.int_matrix(n, 1) for n in (B - 1, B, B + 1)], linkage, "block - 1, block, block + 1")


@pytest.mark.parametrize("linkage", LINKS)
def test_exact_ragged_batch_of_forty(linkage):
    rng = np.random.default_rng(40)
    sizes = rng.integers(0, 71, 40)
    sizes[[0, 7, 39]], sizes[[3, 20]] = 0, 70
    check([ar.int_matrix(int(n), 2 + p) for p, n in enumerate(sizes)], linkage, "forty problems")


@pytest.mark.parametrize("linkage", LINKS)
def test_exact_stops(linkage):
    S = ar.int_matrix(50, 3)
    n = 50
    full = ar.ahc(S, linkage)[0]
    for at in (5, 20, 40):
        h = float(full["value"][at])
        got = run_ahc([S], linkage, threshold=h)
        assert got[1][0] == (full["value"] >= h).sum() > at            # a threshold ON a height: that merge executes
        assert_same(got, ar.batch([S], linkage, threshold=h), ("threshold on a height", at))
        check([S], linkage, "just above", threshold=float(np.nextafter(h, np.inf)))
    for mc in (1, 2, n, n + 3):
        got = run_ahc([S], linkage, min_clusters=mc)
        assert got[2][0] == min(max(mc, 1), n)
        assert_same(got, ar.batch([S], linkage, min_clusters=mc), ("min_clusters", mc))
    check([S, ar.int_matrix(9, 1)], linkage, "both stops", threshold=1.0, min_clusters=4)


@pytest.mark.parametrize("D2", [150, 170])
def test_float_cases_on_the_kernels_own_matrix(D2):
    """The kernel's OWN float32 score matrix goes to kernel and twin: the full merge sequence and the float64 heights are
    bit-equal — one addition per update and one division per value, not a tolerance."""
    from neuralplda_amd import ops
    sizes = [300, 0, 65, 130]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    z, q, P_sqrt, Q = table(D2, int(offs[-1]), 3)
    ro = ops.RaggedOffsets(offs, torch.device(DEV))
    S = ops.score_matrix(_dev(z), _dev(q), packed_for(P_sqrt, Q), ro)
    mats = blocks(S.cpu().numpy(), offs)
    for linkage in LINKS:
        merges, nm, nc, labels = ops.ahc(S, ro, linkage)
        got = (merges.cpu().numpy().view(ar.MERGE_DTYPE).reshape(-1), nm.cpu().numpy(), nc.cpu().numpy(), labels.cpu().numpy())
        assert_same(got, ar.batch(mats, linkage), (D2, linkage))
        assert (got[1] == np.maximum(np.array(sizes) - 1, 0)).all()
        rec = got[0][:299]
        assert (np.diff(rec["value"]) <= 0).all() and np.unique(rec["value"]).size > 250     # real float heights


@pytest.mark.parametrize("linkage", LINKS)
def test_float_sizes_around_small_n(linkage):
    """Above nplda_ahc_small_n() rows a merge with few rows to scan again scans them with the whole workgroup, a wave per row
    otherwise: untied float matrices on both sides of that size take the two paths, the tie-heavy exact one the wave path."""
    from neuralplda_amd import _lib, ops
    N0 = _lib.load().nplda_ahc_small_n()
    sizes = [N0, N0 + 1]
    offs = np.array([0, N0, 2 * N0 + 1], np.int64)
    z, q, P_sqrt, Q = table(150, int(offs[-1]), 6)
    ro = ops.RaggedOffsets(offs, torch.device(DEV))
    S = ops.score_matrix(_dev(z), _dev(q), packed_for(P_sqrt, Q), ro)
    merges, nm, nc, labels = ops.ahc(S, ro, linkage)
    got = (merges.cpu().numpy().view(ar.MERGE_DTYPE).reshape(-1), nm.cpu().numpy(), nc.cpu().numpy(), labels.cpu().numpy())
    assert_same(got, ar.batch(blocks(S.cpu().numpy(), offs), linkage), ("float", sizes, linkage))
    if linkage == "average":
        check([ar.int_matrix(N0 + 1, 5)], linkage, "exact above small_n")


def test_batch_past_the_block_equals_the_single_runs_bit_for_bit():
    """P = 1100 problems against the 1024 threads of ahc_kernel (and the 256 of score_matrix_kernel): where a problem's
    regions start is a sum over the problems in front of it, and from problem `block` on a thread of that sum adds more than
    one term.  Fifteen distinct tiny problems in turn (0, 1, 2, 3, 5 rows) and one of 70 rows last, whose starts depend on
    every term: every problem's outputs equal, bit for bit, those of a call of its own on the same data."""
    from neuralplda_amd import _lib, ops
    P = 1100
    assert P - 1 > _lib.load().nplda_ahc_block()
    sizes = [(0, 1, 2, 3, 5)[i % 5] for i in range(15)] + [70]
    pick = [p % 15 for p in range(P - 1)] + [15]
    offs = np.concatenate([[0], np.cumsum([sizes[i] for i in pick])]).astype(np.int64)
    # the score matrix of a table whose rows repeat with the problems
    roff = np.concatenate([[0], np.cumsum(sizes)])
    z, q, P_sqrt, Q = table(150, int(roff[-1]), 7)
    packed = packed_for(P_sqrt, Q)
    rows = np.concatenate([np.arange(roff[i], roff[i + 1]) for i in pick])
    got = blocks(ops.score_matrix(_dev(z[rows]), _dev(q[rows]), packed, offs).cpu().numpy(), offs)
    alone = [ops.score_matrix(_dev(z[roff[i]:roff[i + 1]]), _dev(q[roff[i]:roff[i + 1]]), packed).cpu().numpy() if n else
             np.zeros((0, 0), np.float32) for i, n in enumerate(sizes)]
    for p, i in enumerate(pick):
        assert np.array_equal(bits(got[p]), bits(alone[i])), ("score_matrix", p)
    # the clustering, on exact matrices
    mats = [ar.int_matrix(n, 100 + i) for i, n in enumerate(sizes)]
    rec, nm, nc, lab = run_ahc([mats[i] for i in pick], "average")
    ro = np.concatenate([[0], np.cumsum([max(sizes[i] - 1, 0) for i in pick])])
    singles = [run_ahc([m], "average") for m in mats]
    assert singles[15][1][0] == 69
    for p, i in enumerate(pick):
        assert_same((rec[ro[p]:ro[p + 1]], nm[p:p + 1], nc[p:p + 1], lab[offs[p]:offs[p + 1]]), singles[i], ("ahc", p))


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------

class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 170, 170
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


def kaldi_model():
    from neuralplda_amd import models
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_kaldi_params.npz"))
    m = models.NeuralPlda(NC())
    sd = m.state_dict()
    for k, a in (("centering_and_LDA.weight", "W1"), ("centering_and_LDA.bias", "b1"), ("centering_and_wccn_plda.weight", "W2"),
                 ("centering_and_wccn_plda.bias", "b2"), ("P_sqrt", "P_sqrt"), ("Q", "Q")):
        sd[k].copy_(torch.from_numpy(g1[a]))
    return m.to(DEV), g1


def speakers(g1, S_=12, U=9):
    from tests import synth
    return synth.speaker_structured_xvectors(g1["W1"], g1["b1"], g1["W2"].astype(np.float64), g1["plda_mean"], g1["psi"], S_, U,
                                             1.0, 11)


def test_cluster_end_to_end_recovers_the_speakers():
    from neuralplda_amd import backend
    from neuralplda_amd.sv_trials_loaders import XvectorTable
    S_, U = 12, 9
    m, g1 = kaldi_model()
    x, spk = speakers(g1, S_, U)
    rng = np.random.default_rng(5)
    perm = rng.permutation(S_ * U)                       # the caller's rows come in no particular order
    x, spk = x[perm], spk[perm]
    groups = spk % 3
    X = torch.from_numpy(x).to(DEV)
    # precondition, on the float64 twin: within every group the last within-speaker height and the first cross-speaker
    # height lie at least 100 score tolerances apart
    with torch.no_grad():
        z = m.extract_plda_embeddings(X).cpu().numpy()
    P_sqrt, Q = g1["P_sqrt"], g1["Q"]
    q = tr.qvec(z, Q, np.float64)
    lo, hi, tol = np.inf, -np.inf, 0.0
    for g in range(3):
        ix = np.flatnonzero(groups == g)
        zg, qg = z[ix], q[ix]
        rec = ar.ahc(tr.scores(zg, qg, zg, qg, P_sqrt, np.float64), "average")[0]
        tol = max(tol, float(tr.tolerance(170, tr.magnitude(zg, qg, zg, qg, P_sqrt)).max()))
        members = {i: {int(spk[ix[i]])} for i in range(ix.size)}
        for r in rec:
            both = members[r["a"]] | members.pop(r["b"])
            members[r["a"]] = both
            if len(both) == 1:
                lo = min(lo, r["value"])
            else:
                hi = max(hi, r["value"])
    print(f"last within-speaker height {lo:.4f}, first cross-speaker height {hi:.4f}, score tolerance {tol:.2e}")
    assert lo - hi >= 100.0 * tol
    thr = 0.5 * (lo + hi)
    c = m.cluster(X, groups=groups, threshold=thr)
    assert c.labels.shape == (S_ * U,) and c.n_clusters.tolist() == [4, 4, 4] and len(c) == S_ * U
    pairs = {(int(a), int(b)) for a, b in zip(c.labels, spk)}
    assert len(pairs) == S_ and np.unique(c.labels).size == S_          # cluster <-> speaker one to one
    assert (c.labels // 4 == groups).all()                               # clusters numbered group by group
    full = m.cluster(X, groups=groups)
    assert full.n_clusters.tolist() == [1, 1, 1] and (full.n_merges == 35).all()
    for cut in (full.cut(n_clusters=4), full.cut(threshold=thr)):
        assert np.array_equal(cut.labels, c.labels) and cut.n_clusters.tolist() == [4, 4, 4]
    assert np.array_equal(bits(full.cut(threshold=thr).merges["value"]), bits(c.merges["value"]))
    # the pseudo-speakers feed the back-end estimation
    ids = [f"utt{i:03d}" for i in range(S_ * U)]
    s2u = c.spk2utt(ids)
    assert len(s2u) == S_ and all(len(u) == U for _, u in s2u) and s2u[0][0] == "c0000"
    tab = XvectorTable.from_matrix(ids, x)
    rows, offs, names, missing = backend.class_layout(tab, s2u)
    assert not missing and len(names) == S_ and (np.diff(offs) == U).all()
    # (the LDA alone: fitted on 108 rows of 512 dimensions it maps a speaker's rows onto one point, which leaves a PLDA
    # step no within-class scatter to estimate — a matter of the set's size, not of where its labels come from)
    with pytest.warns(UserWarning, match="floored"):
        be = backend.fit_backend(tab, s2u, 8, plda=False, device=DEV)
    assert be.transform_mat.shape == (8, 513) and np.isfinite(be.transform_mat).all()
    from neuralplda_amd import models
    for cls in (models.DPlda, models.GaussianBackend):
        with pytest.raises(NotImplementedError):
            cls(NC).cluster(X)


# ---- 4. housekeeping -------------------------------------------------------------------------------------------------------------------

def test_repeatable_and_capturable():
    """Two calls give identical bytes, and so does the pair score_matrix + ahc captured in a graph (one stream, no branches)
    and replayed twice."""
    from neuralplda_amd import ops
    offs = np.array([0, 130, 130, 200, 217], np.int64)
    z, q, P_sqrt, Q = table(150, 217, 4)
    packed = packed_for(P_sqrt, Q)
    zd, qd = _dev(z), _dev(q)
    ro = ops.RaggedOffsets(offs, torch.device(DEV))

    def pair():
        S = ops.score_matrix(zd, qd, packed, ro)
        return (S,) + ops.ahc(S, ro, "average", -0.5, 2)

    a, b = [t.cpu().numpy().tobytes() for t in pair()], [t.cpu().numpy().tobytes() for t in pair()]
    assert a == b
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pair()
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert [t.cpu().numpy().tobytes() for t in out] == a


def test_degenerate_arguments_raise():
    from neuralplda_amd import ops
    z, q, P_sqrt, Q = table(150, 20, 5)
    packed = packed_for(P_sqrt, Q)
    zd, qd = _dev(z), _dev(q)
    S = ops.score_matrix(zd, qd, packed)
    assert S.shape == (20, 20)
    empty = ops.score_matrix(zd[:0], qd[:0], packed)
    assert empty.shape == (0, 0)
    out = ops.ahc(empty)
    assert out[0].shape == (0, 24) and out[1].tolist() == [0] and out[2].tolist() == [0] and out[3].shape == (0,)
    out = ops.ahc(torch.zeros(0, device=DEV), [0])           # P = 0
    assert out[1].shape == (0,) and out[3].shape == (0,)
    for bad in (dict(threshold=float("nan")), dict(min_clusters=0), dict(linkage="ward")):
        with pytest.raises(ValueError):
            ops.ahc(S, **bad)
    with pytest.raises(ValueError):
        ops.ahc(S, [0, 19])                                   # the matrix does not fit the offsets
    with pytest.raises(ValueError):
        ops.ahc(S.view(-1), [0, 25, 20])                      # unsorted
    with pytest.raises(ValueError):
        ops.score_matrix(zd, qd, packed, [0, 19])             # the offsets do not cover the table
    with pytest.raises(ValueError):
        ops.score_matrix(zd[:, :150], qd, packed)
    with pytest.raises(ValueError):
        ops.RaggedOffsets([0, 16385], torch.device(DEV))
    with pytest.raises(Exception):
        ops.ahc(S.cpu())


def test_cluster_tool_writes_utt2spk_and_spk2utt(tmp_path):
    import pickle
    from neuralplda_amd import backend, kaldi_format
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cluster_xvectors
    m, g1 = kaldi_model()
    x, spk = speakers(g1, 6, 9)
    ids = [f"r{s % 2}-u{i:03d}" for i, s in enumerate(spk)]
    kaldi_format.write_vector_ark(str(tmp_path / "x.ark"), ids, x, scp_path=str(tmp_path / "x.scp"))
    with open(tmp_path / "model.pt", "wb") as fh:
        pickle.dump(m, fh)
    reco = {f"reco{r}": [u for u, s in zip(ids, spk) if s % 2 == r] for r in (0, 1)}
    (tmp_path / "reco2utt").write_text("".join(f"{r} {' '.join(u)}\n" for r, u in reco.items()))
    cluster_xvectors.main(["--model", str(tmp_path / "model.pt"), "--xvectors", str(tmp_path / "x.scp"), "--reco2utt",
                           str(tmp_path / "reco2utt"), "--threshold", "-0.4", "--out-dir", str(tmp_path / "out")])
    s2u = backend.read_spk2utt(str(tmp_path / "out" / "spk2utt"))
    assert len(s2u) == 6 and sorted(u for _, us in s2u for u in us) == sorted(ids)
    for name, us in s2u:
        assert len({spk[ids.index(u)] for u in us}) == 1 and len(us) == 9
    u2s = dict(ln.split() for ln in (tmp_path / "out" / "utt2spk").read_text().splitlines())
    assert u2s == {u: name for name, us in s2u for u in us} and list(u2s) == sorted(ids)
