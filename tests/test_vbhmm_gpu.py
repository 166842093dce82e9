"""ops.vbhmm (csrc/nplda_vbhmm.hip), cluster.vb_refine and tools/cluster_xvectors.py --vb-plda on the GPU, against the numpy
twins of tests/vbhmm_ref.py: the error against the longdouble twin in units of the float64 twin's own error (gates 3 rms / 5
max, as tests/fp32_units.py one precision up).  The ratios measured on an MI355X stand next to each use."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import vbhmm_ref as vr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [0, 0, 17, 1, 0, 65, 300, 0, 64, 2, 0]     # empty problems first, in the middle and last
RAGGED_S = [0, 3, 5, 1, 0, 64, 7, 2, 12, 2, 4]      # empty problems with and without speaker slots; 64: every lane


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def padded(x, fill=0.0):
    """The rows as embed() lays them out: a row stride of the next multiple of 16, `fill` in the pad columns."""
    T, D = x.shape
    z = np.full((T, (D + 15) // 16 * 16), fill, np.float32)
    z[:, :D] = x
    return z


class Got:
    """The outputs of ops.vbhmm for ONE problem, on the host."""

    def __init__(self, out, T, S):
        gamma, pi, elbo, n_iters, labels, n_speakers = (t.cpu().numpy() for t in out)
        self.gamma, self.pi, self.elbo = gamma.reshape(T, S), pi, elbo[0]
        self.n_iters, self.labels, self.n_speakers = int(n_iters[0]), labels, int(n_speakers[0])
        self.raw = out


def run_one(x, psi, S, fill=0.0, **kw):
    from neuralplda_amd import ops
    if "gamma_init" in kw:
        kw["gamma_init"] = _dev(np.asarray(kw["gamma_init"], np.float64).ravel())
    return Got(ops.vbhmm(_dev(padded(x, fill)), [0, x.shape[0]], [0, S], _dev(psi), **kw), x.shape[0], S)


def report(what, r):
    print(f"{what}: " + ", ".join(f"{k} {v[0]:.3f} rms / {v[1]:.3f} max" for k, v in r.items()))


def test_longdouble_is_wider_than_float64():
    assert np.finfo(np.longdouble).nmant >= 63


# ---- 1. a single iteration ---------------------------------------------------------------------------------------------------------

SINGLE = [(T, S) for T in (1, 2, 63, 64, 65, 300) for S in (1, 2, 7, 64)]


@functools.lru_cache(maxsize=None)
def single_case(D2, T, S):
    x, psi, lab, _ = vr.make_problem(1000 * D2 + 10 * T + S, T, S, D2, 0.25)
    g0 = vr.gamma_from_labels(lab, S)
    kw = dict(max_iters=1)
    return x, psi, g0, vr.vbhmm(x, psi, g0, dtype=np.longdouble, **kw), vr.vbhmm(x, psi, g0, **kw)


@pytest.mark.parametrize("D2", [150, 170])
def test_single_iteration(D2):
    """max_iters = 1 from gamma_init at every T in {1, 2, 63, 64, 65, 300} x S in {1, 2, 7, 64}; sep = 0.25, where the rows
    are soft: at least a tenth of the rows with a choice (S >= 2) have max gamma < 0.99 on the twin.
    Measured on an MI355X, the worst of the 24 shapes (rms / max): D2 = 150 gamma 0.93 / 0.82, pi 0.95 / 1.16, ELBO 2.15;
    D2 = 170 gamma 0.81 / 0.76, pi 1.16 / 1.13, ELBO 1.71.  The worst sit at T <= 2 (one ELBO against a floor of half an
    ulp); at T >= 63 gamma and pi stay below 0.2.  Before G_t was summed with compensation and pi's normaliser as a tree
    the ELBO stood at 3.9 (T = 2, S = 1) and pi at 7.9 rms (T = 1, S = 64)."""
    cases = [single_case(D2, T, S) for T, S in SINGLE]
    soft = np.concatenate([c[3].gamma.max(axis=1) < 0.99 for c, (T, S) in zip(cases, SINGLE) if S >= 2])
    assert soft.mean() >= 0.1, soft.mean()
    worst = {}
    for (x, psi, g0, ld, r64), (T, S) in zip(cases, SINGLE):
        got = run_one(x, psi, S, gamma_init=g0, max_iters=1)
        assert got.n_iters == 1
        r = vr.check_result(got, ld, r64, f"D2 = {D2}, T = {T}, S = {S}")
        report(f"D2 = {D2}, T = {T}, S = {S}", r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, (0, 0)), v, key=lambda u: u[1])
    report(f"D2 = {D2}, worst", worst)


# ---- 2. a full run -------------------------------------------------------------------------------------------------------------------

FULL = [(300, 7, 150, 2.0, 3), (64, 64, 170, 2.0, 1), (65, 12, 150, 1.0, 2)]     # T, S, D2, sep, seed


@functools.lru_cache(maxsize=None)
def full_case(T, S, D2, sep, seed):
    x, psi, lab, _ = vr.make_problem(seed, T, S, D2, sep)
    g0 = vr.gamma_from_labels(lab, S)
    free = vr.vbhmm(x, psi, g0, eps=-np.inf, max_iters=40, dtype=np.longdouble)
    picked = vr.pick_epsilon(free.elbo)
    assert picked is not None, "no pair of consecutive ELBO gains 4x apart with every gain outside [eps / 2, 2 eps]"
    eps, n = picked
    ld, r64 = vr.vbhmm(x, psi, g0, eps=eps, max_iters=40, dtype=np.longdouble), vr.vbhmm(x, psi, g0, eps=eps, max_iters=40)
    return x, psi, lab, eps, n, ld, r64


@pytest.mark.parametrize("case", FULL, ids=lambda c: "T%d-S%d-D%d" % c[:3])
def test_full_run(case):
    """max_iters = 40 from labels, the stop at an epsilon no rounding can move (every ELBO gain of the twin's never-stopping
    trace outside [eps / 2, 2 eps]) and every row's top-two margin >= 1e-3: n_iters and labels equal the twin's, gamma, pi
    and the ELBO trace within the gates.  Measured on an MI355X (rms / max): T = 300, S = 7: gamma 0.001 / 0.001,
    pi 0.001 / 0.001, ELBO 0.002 / 0.002 over 6 iterations; T = 64, S = 64: 0.000, 0.001, 0.066 / 0.067 over 8;
    T = 65, S = 12: 0.000, 0.000, 0.003 / 0.002 over 6."""
    T, S, D2 = case[:3]
    x, psi, lab, eps, n, ld, r64 = full_case(*case)
    assert ld.n_iters == r64.n_iters == n and 3 <= n < 40
    assert vr.top_two_margin(ld.gamma) >= 1e-3 and ld.n_speakers >= 2
    got = run_one(x, psi, S, labels_init=_dev(lab), epsilon=eps, max_iters=40)
    assert got.n_iters == n
    assert np.array_equal(got.labels, ld.labels) and got.n_speakers == ld.n_speakers
    assert np.isnan(got.elbo[n:]).all() and np.isfinite(got.elbo[:n]).all()
    report(f"T = {T}, S = {S}, D2 = {D2}, {n} iterations", vr.check_result(got, ld, r64, f"T = {T}, S = {S}"))


# ---- 3. a ragged batch ---------------------------------------------------------------------------------------------------------------

def ragged_inputs(D2=150):
    rng = np.random.default_rng(9)
    xs, labs = [], []
    for p, (T, S) in enumerate(zip(RAGGED, RAGGED_S)):
        x, psi, lab, _ = vr.make_problem(40 + p, T, max(S, 1), D2, 1.0)
        xs.append(x)
        labs.append(lab)
    pi0 = rng.dirichlet(np.ones(sum(RAGGED_S)))
    return xs, psi, labs, pi0


def test_ragged_batch_equals_the_single_runs_bit_for_bit():
    from neuralplda_amd import ops
    xs, psi, labs, pi0 = ragged_inputs()
    offs, spk = np.concatenate([[0], np.cumsum(RAGGED)]), np.concatenate([[0], np.cumsum(RAGGED_S)])
    pis = [pi0[spk[p]:spk[p + 1]] / max(pi0[spk[p]:spk[p + 1]].sum(), 1e-300) for p in range(len(RAGGED))]
    kw = dict(epsilon=1e-3, max_iters=12)

    def batch(fill, nan_slots):
        pi_all = np.concatenate(pis)
        if nan_slots:                                   # the speaker slots of the problems without rows are never read
            for p, T in enumerate(RAGGED):
                if T == 0:
                    pi_all[spk[p]:spk[p + 1]] = np.nan
        out = ops.vbhmm(_dev(padded(np.concatenate(xs), fill)), offs, spk, _dev(psi), labels_init=_dev(np.concatenate(labs)),
                        pi_init=_dev(pi_all), **kw)
        return [t.cpu().numpy() for t in out]

    gamma, pi, elbo, n_iters, labels, n_spk = batch(0.0, False)
    goff = np.concatenate([[0], np.cumsum(np.array(RAGGED) * np.array(RAGGED_S))])
    for p, (T, S) in enumerate(zip(RAGGED, RAGGED_S)):
        if T == 0:
            assert n_iters[p] == 0 and n_spk[p] == 0 and np.isnan(elbo[p]).all()
            continue
        one = run_one(xs[p], psi, S, labels_init=_dev(labs[p]), pi_init=_dev(pis[p]), **kw)
        assert np.array_equal(bits(gamma[goff[p]:goff[p + 1]]), bits(one.gamma.ravel())), p
        assert np.array_equal(bits(pi[spk[p]:spk[p + 1]]), bits(one.pi)) and np.array_equal(bits(elbo[p]), bits(one.elbo)), p
        assert n_iters[p] == one.n_iters and n_spk[p] == one.n_speakers, p
        assert np.array_equal(labels[offs[p]:offs[p + 1]], one.labels), p
        assert 1 <= one.n_iters <= 12 and np.isfinite(one.gamma).all()
    # NaN in the pad columns D2 .. ldz and in the slots of the zero-length problems changes no bit
    again = batch(np.nan, True)
    live = np.concatenate([np.arange(spk[p], spk[p + 1]) for p, T in enumerate(RAGGED) if T > 0])
    for a, b in zip((gamma, pi[live], elbo, n_iters, labels, n_spk),
                    (again[0], again[1][live], again[2], again[3], again[4], again[5])):
        assert np.array_equal(bits(a), bits(b))


def test_batch_past_the_block_equals_the_single_runs_bit_for_bit():
    """P = 600 problems against the 512 threads of the workgroup: where a problem's posteriors and workspace slice start is a
    sum over the problems in front of it, and from problem 512 on a thread of that sum adds more than one term.  Fifteen
    distinct tiny problems in turn (0, 1, 2, 3, 5 rows) and one of 40 rows and 3 speakers last, whose starts depend on every
    term: every problem's outputs equal, bit for bit, those of a call of its own on the same data."""
    from neuralplda_amd import _lib, ops
    P, D2 = 600, 150
    assert P - 1 > _lib.load().nplda_vbhmm_block()
    Ts = [(0, 1, 2, 3, 5)[i % 5] for i in range(15)] + [40]
    Ss = [0, 1, 2, 3, 2, 2, 1, 1, 2, 3, 1, 1, 2, 1, 4, 3]     # empty problems with and without speaker slots
    rng = np.random.default_rng(10)
    probs = [vr.make_problem(60 + i, T, max(S, 1), D2, 1.0) for i, (T, S) in enumerate(zip(Ts, Ss))]
    psi = probs[0][1]
    pis = [rng.dirichlet(np.ones(S)) if S else np.zeros(0) for S in Ss]
    pick = [p % 15 for p in range(P - 1)] + [15]
    offs = np.concatenate([[0], np.cumsum([Ts[i] for i in pick])])
    spk = np.concatenate([[0], np.cumsum([Ss[i] for i in pick])])
    goff = np.concatenate([[0], np.cumsum([Ts[i] * Ss[i] for i in pick])])
    kw = dict(epsilon=1e-3, max_iters=12)
    out = ops.vbhmm(_dev(padded(np.concatenate([probs[i][0] for i in pick]))), offs, spk, _dev(psi),
                    labels_init=_dev(np.concatenate([probs[i][2] for i in pick])),
                    pi_init=_dev(np.concatenate([pis[i] for i in pick])), **kw)
    gamma, pi, elbo, n_iters, labels, n_spk = (t.cpu().numpy() for t in out)
    singles = [run_one(probs[i][0], psi, Ss[i], labels_init=_dev(probs[i][2]), pi_init=_dev(pis[i]), **kw) if Ts[i] else None
               for i in range(16)]
    assert 1 <= singles[15].n_iters <= 12 and np.isfinite(singles[15].gamma).all()
    for p, i in enumerate(pick):
        one = singles[i]
        if one is None:
            assert n_iters[p] == 0 and n_spk[p] == 0 and np.isnan(elbo[p]).all(), p
            continue
        assert np.array_equal(bits(gamma[goff[p]:goff[p + 1]]), bits(one.gamma.ravel())), p
        assert np.array_equal(bits(pi[spk[p]:spk[p + 1]]), bits(one.pi)) and np.array_equal(bits(elbo[p]), bits(one.elbo)), p
        assert n_iters[p] == one.n_iters and n_spk[p] == one.n_speakers, p
        assert np.array_equal(labels[offs[p]:offs[p + 1]], one.labels), p


# ---- 4. the initialisers -------------------------------------------------------------------------------------------------------------

def test_initialisers():
    """Measured on an MI355X (rms / max): labels init and gamma_init alike gamma 0.000 / 0.001, pi 0.000 / 0.000, ELBO
    0.116 / 0.111; pi_init with zeros gamma 0.000 / 0.000, pi 0.198 / 0.198, ELBO 0.247 / 0.273."""
    T, S, D2 = 65, 7, 150
    x, psi, lab, _ = vr.make_problem(77, T, S, D2, 1.0)
    lab = lab.copy()
    lab[[3, 40]] = [-1, S]                                  # outside 0 .. S - 1: the uniform row
    g0 = vr.gamma_from_labels(lab, S)
    assert np.array_equal(g0[3], np.full(S, 1.0 / S)) and np.array_equal(g0[40], np.full(S, 1.0 / S))
    kw = dict(max_iters=3, eps=-np.inf)
    ld, r64 = vr.vbhmm(x, psi, g0, dtype=np.longdouble, **kw), vr.vbhmm(x, psi, g0, **kw)
    a = run_one(x, psi, S, labels_init=_dev(lab), max_iters=3, epsilon=-np.inf)
    b = run_one(x, psi, S, gamma_init=g0, max_iters=3, epsilon=-np.inf)
    report("labels init", vr.check_result(a, ld, r64, "labels init"))
    report("gamma init", vr.check_result(b, ld, r64, "gamma init"))
    # (the twin ran from posteriors with the uniform rows 3 and 40: a kernel that treated those labels otherwise misses it)
    # pi_init with exact zeros keeps those speakers dead
    pi0 = np.array([0.3, 0.0, 0.2, 0.0, 0.5, 0.0, 0.0])
    kw = dict(max_iters=5, eps=-np.inf)
    ld, r64 = vr.vbhmm(x, psi, g0, pi0, dtype=np.longdouble, **kw), vr.vbhmm(x, psi, g0, pi0, **kw)
    c = run_one(x, psi, S, gamma_init=g0, pi_init=_dev(pi0), max_iters=5, epsilon=-np.inf)
    dead = pi0 == 0
    assert (c.gamma[:, dead] == 0).all() and (c.pi[dead] == 0).all() and (c.pi[~dead] > 0).all()
    assert (ld.gamma[:, dead] == 0).all() and (ld.pi[dead] == 0).all()
    report("dead speakers", vr.check_result(c, ld, r64, "pi_init with zeros"))
    assert np.array_equal(c.labels, ld.labels) and c.n_speakers == ld.n_speakers <= 3


# ---- 5. the stops -------------------------------------------------------------------------------------------------------------------

def test_stops():
    T, S, D2 = 64, 3, 150
    x, psi, lab, _ = vr.make_problem(5, T, S, D2, 1.0)
    never = run_one(x, psi, S, labels_init=_dev(lab), epsilon=-np.inf, max_iters=9)
    assert never.n_iters == 9 and np.isfinite(never.elbo).all()
    at_once = run_one(x, psi, S, labels_init=_dev(lab), epsilon=np.inf, max_iters=9)
    assert at_once.n_iters == 2 and np.isnan(at_once.elbo[2:]).all()
    assert np.array_equal(bits(at_once.elbo[:2]), bits(never.elbo[:2]))
    single = run_one(x, psi, S, labels_init=_dev(lab), epsilon=np.inf, max_iters=1)
    assert single.n_iters == 1 and np.array_equal(bits(single.elbo), bits(never.elbo[:1]))


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------

def test_vb_refine_end_to_end_recovers_the_speakers():
    """The data of test_cluster_end_to_end_recovers_the_speakers with a time order: every group's rows come speaker by
    speaker in runs of three.  The model length-normalises in front of its PLDA layer, which leaves these rows a within-class
    deviation of 0.078 per dimension where the VB-HMM takes 1: the fixture model's PLDA layer is rescaled by the pooled
    within-class deviation of its own embeddings (as a PLDA layer estimated on them would be).  The clustering over-clusters
    (a threshold inside the within-speaker heights, chosen on the twin: 8 or 9 clusters per group of 4 speakers, no cut
    afterwards), vb_refine recovers the speakers."""
    from neuralplda_amd import backend, models
    from neuralplda_amd.sv_trials_loaders import XvectorTable
    from tests import ahc_ref as ar
    from tests import topk_ref as tr
    from tests.test_ahc_gpu import NC, kaldi_model, speakers
    S_, U = 12, 9
    vb = dict(Fa=0.5, Fb=5.0, loop_prob=0.9)              # 36 rows a group in runs of three: a weaker prior, shorter stays
    m, g1 = kaldi_model()
    x, spk = speakers(g1, S_, U)
    order = np.concatenate([np.flatnonzero(spk == s)[3 * r:3 * r + 3] for r in range(3) for s in range(S_)])
    x, spk = x[order], spk[order]                         # time: runs of three rows of a speaker, every speaker three times
    groups = spk % 3
    X = torch.from_numpy(x).to(DEV)
    psi = g1["psi"].astype(np.float64)
    with torch.no_grad():
        z = m.extract_plda_embeddings(X).cpu().numpy().astype(np.float64)
        within = np.concatenate([z[spk == s] - z[spk == s].mean(axis=0) for s in range(S_)])
        sigma = float(np.sqrt((within ** 2).sum() / (S_ * (U - 1) * z.shape[1])))
        assert 0.05 < sigma < 0.12, sigma
        m.centering_and_wccn_plda.weight.div_(sigma)
        m.centering_and_wccn_plda.bias.div_(sigma)
        z = m.extract_plda_embeddings(X).cpu().numpy()
    q = tr.qvec(z, g1["Q"], np.float64)
    # the threshold: in every group the height at which 8 clusters remain, on the float64 twin of the clustering
    heights = []
    for g in range(3):
        ix = np.flatnonzero(groups == g)
        rec = ar.ahc(tr.scores(z[ix], q[ix], z[ix], q[ix], g1["P_sqrt"], np.float64), "average")[0]
        heights.append((rec["value"][ix.size - 9], rec["value"][ix.size - 8]))
    thr = max(0.5 * (a + b) for a, b in heights)
    c = m.cluster(X, groups=groups, threshold=thr)
    assert (c.n_clusters > 4).all() and (c.n_clusters <= 64).all(), c.n_clusters
    # precondition on the twin: from these clusters it recovers the speakers with margin
    base = np.concatenate([[0], np.cumsum(c.n_clusters)])
    for g in range(3):
        ix = np.flatnonzero(groups == g)
        S = int(c.n_clusters[g])
        tw = vr.vbhmm(z[ix].astype(np.float32), psi, vr.gamma_from_labels(c.labels[ix] - base[g], S), Fa=0.5, Fb=5.0, loop=0.9)
        assert tw.n_speakers == 4 and vr.top_two_margin(tw.gamma) >= 0.5
        assert len({(int(a), int(b)) for a, b in zip(tw.labels, spk[ix])}) == 4
    r = m.vb_refine(X, c, psi, groups=groups, **vb)
    assert r.n_clusters.tolist() == [4, 4, 4] and len(r) == S_ * U and r.labels.shape == (S_ * U,)
    pairs = {(int(a), int(b)) for a, b in zip(r.labels, spk)}
    assert len(pairs) == S_ and np.unique(r.labels).size == S_          # refined speaker <-> speaker one to one
    assert (r.labels // 4 == groups).all()
    assert [g.shape for g in r.gamma] == [(36, int(s)) for s in c.n_clusters] and r.elbo.shape == (3, 40)
    assert (r.n_iters >= 2).all() and all(abs(p.sum() - 1) < 1e-12 for p in r.pi)
    # integer labels, global or local, give the same result
    for init in (c.labels, c.labels - base[groups]):
        again = m.vb_refine(X, init, psi, groups=groups, **vb)
        assert np.array_equal(again.labels, r.labels)
    ids = [f"utt{i:03d}" for i in range(S_ * U)]
    s2u = r.spk2utt(ids)
    assert len(s2u) == S_ and all(len(u) == U for _, u in s2u) and s2u[0][0] == "c0000"
    rows, offs, names, missing = backend.class_layout(XvectorTable.from_matrix(ids, x), s2u)
    assert not missing and len(names) == S_ and (np.diff(offs) == U).all()
    with pytest.raises(ValueError, match="cut"):
        m.vb_refine(X, np.arange(S_ * U), psi)               # 108 slots in one group
    with pytest.raises(ValueError):
        m.vb_refine(X, c, psi)                                # the clustering had groups
    for cls in (models.DPlda, models.GaussianBackend):
        with pytest.raises(NotImplementedError):
            cls(NC).vb_refine(X, c, psi)


# ---- 7. housekeeping ---------------------------------------------------------------------------------------------------------------

def test_repeatable_and_capturable():
    """Two calls give identical bytes, and so does score_matrix + ahc + vbhmm captured in one graph on one stream and
    replayed twice."""
    from neuralplda_amd import ops
    from tests.test_ahc_gpu import packed_for, table
    offs = np.array([0, 130, 130, 200, 217], np.int64)
    z, q, P_sqrt, Q = table(150, 217, 4)
    packed = packed_for(P_sqrt, Q)
    zd, qd = _dev(10.0 * z), _dev(q)
    psi = _dev(0.5 * 0.97 ** np.arange(150))
    ro = ops.RaggedOffsets(offs, torch.device(DEV))
    so = ops.RaggedOffsets([0, 6, 6, 12, 18], torch.device(DEV))

    def chain():
        S = ops.score_matrix(zd, qd, packed, ro)
        out = ops.ahc(S, ro, "average", float("-inf"), 6)          # six clusters per problem: labels 0 .. 5
        return (S,) + out + ops.vbhmm(zd, ro, so, psi, labels_init=out[3], max_iters=6, epsilon=-np.inf)

    a, b = [t.cpu().numpy().tobytes() for t in chain()], [t.cpu().numpy().tobytes() for t in chain()]
    assert a == b
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain()
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert [t.cpu().numpy().tobytes() for t in out] == a


def test_degenerate_arguments_raise():
    from neuralplda_amd import ops
    x, psi, lab, _ = vr.make_problem(1, 20, 3, 150, 1.0)
    zd, pd, ld = _dev(padded(x)), _dev(psi), _dev(lab)
    ok = ops.vbhmm(zd, [0, 20], [0, 3], pd, labels_init=ld)
    assert ok[0].shape == (60,) and ok[2].shape == (1, 40) and ok[4].shape == (20,)
    out = ops.vbhmm(zd[:0], [0], [0], pd, labels_init=ld[:0])                       # P = 0
    assert out[0].shape == (0,) and out[2].shape == (0, 40) and out[3].shape == (0,)
    out = ops.vbhmm(zd[:0], [0, 0], [0, 2], pd, labels_init=ld[:0], max_iters=5)      # one problem without rows
    assert out[3].tolist() == [0] and out[5].tolist() == [0] and torch.isnan(out[2]).all() and out[2].shape == (1, 5)
    for bad in (dict(Fa=0.0), dict(Fb=-1.0), dict(Fa=float("nan")), dict(loop_prob=1.0), dict(loop_prob=-0.1),
                dict(epsilon=float("nan")), dict(init_smoothing=-1.0), dict(max_iters=0), dict(max_iters=257)):
        with pytest.raises(ValueError):
            ops.vbhmm(zd, [0, 20], [0, 3], pd, labels_init=ld, **bad)
    g0 = _dev(vr.gamma_from_labels(lab, 3).ravel())
    for kw in (dict(), dict(labels_init=ld, gamma_init=g0), dict(gamma_init=g0[:-1]), dict(labels_init=ld[:-1]),
               dict(labels_init=ld, pi_init=_dev(np.ones(2) / 2))):
        with pytest.raises(ValueError):
            ops.vbhmm(zd, [0, 20], [0, 3], pd, **kw)
    for offs, spk in (([0, 19], [0, 3]), ([0, 20], [0, 0]), ([0, 20], [0, 65]), ([0, 20], [0, 3, 4]), ([0, 20], None)):
        with pytest.raises(ValueError):
            ops.vbhmm(zd, offs, spk, pd, labels_init=ld)
    with pytest.raises(ValueError):
        ops.vbhmm(zd[:, 1:151], [0, 20], [0, 3], pd, labels_init=ld)                 # rows that do not start on 16 bytes
    view = ops.vbhmm(zd[:, :150], [0, 20], [0, 3], pd, labels_init=ld)              # a view of the padded rows is what it is
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(view, ok))
    with pytest.raises(ValueError):
        ops.vbhmm(zd, [0, 20], [0, 3], _dev(np.ones(161)), labels_init=ld)           # more variances than columns
    with pytest.raises(Exception):
        ops.vbhmm(zd.cpu(), [0, 20], [0, 3], pd, labels_init=ld)


def test_cluster_tool_with_and_without_vb(tmp_path):
    import pickle
    from neuralplda_amd import backend, cluster, kaldi_format
    from tests.test_ahc_gpu import kaldi_model, speakers
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
    D = g1["psi"].size
    kaldi_format.write_plda_binary(str(tmp_path / "plda"), np.zeros(D), np.eye(D), g1["psi"].astype(np.float64))
    common = ["--model", str(tmp_path / "model.pt"), "--xvectors", str(tmp_path / "x.scp"), "--reco2utt", str(tmp_path / "reco2utt")]
    # without --vb-plda: what the tool writes today (the clustering alone)
    cluster_xvectors.main(common + ["--threshold", "-0.4", "--out-dir", str(tmp_path / "plain")])
    X = torch.from_numpy(x).to(DEV)
    groups = (spk % 2).tolist()
    sel = np.concatenate([np.flatnonzero(spk % 2 == r) for r in (0, 1)])
    c = cluster.cluster(m, X[_dev(sel)], groups=sorted(groups), threshold=-0.4)
    s2u = c.spk2utt([ids[i] for i in sel])
    assert (tmp_path / "plain" / "spk2utt").read_text() == "".join(f"{n} {' '.join(u)}\n" for n, u in s2u)
    assert (tmp_path / "plain" / "utt2spk").read_text() == "".join(
        f"{u} {n}\n" for u, n in sorted((u, n) for n, us in s2u for u in us))
    # with it: over-clustered at a high threshold, refined; consistent with vb_refine on the same rows
    cluster_xvectors.main(common + ["--min-clusters", "8", "--vb-plda", str(tmp_path / "plda"), "--vb-max-iters", "30",
                                    "--out-dir", str(tmp_path / "vb")])
    c8 = cluster.cluster(m, X[_dev(sel)], groups=sorted(groups), min_clusters=8)
    psi = kaldi_format.read_plda(str(tmp_path / "plda"))["Psi_across_covar_diag"]
    r = cluster.vb_refine(m, X[_dev(sel)], c8, psi, groups=sorted(groups), max_iters=30)
    want = r.spk2utt([ids[i] for i in sel])
    got = backend.read_spk2utt(str(tmp_path / "vb" / "spk2utt"))
    assert [(n, list(u)) for n, u in got] == [(n, list(u)) for n, u in want]
    u2s = dict(ln.split() for ln in (tmp_path / "vb" / "utt2spk").read_text().splitlines())
    assert u2s == {u: n for n, us in want for u in us} and list(u2s) == sorted(ids)
