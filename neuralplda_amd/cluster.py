"""Agglomerative clustering of embeddings under the model's own score (csrc/nplda_ahc.hip, design/k21_ahc.md), spectral
clustering with an auto-tuned neighbour count (csrc/nplda_spectral.hip, design/k25_spectral.md), and their refinement by the Bayesian HMM over each group's rows in time order (VBx: csrc/nplda_vbhmm.hip, design/k22_vbhmm.md).

Unlabelled x-vectors become pseudo-speakers: the set is embedded once (search.embed_table), every group of rows (one
recording, one domain, or the whole set) is one PROBLEM whose dense score matrix ops.score_matrix writes and ops.ahc
partitions, and the result maps back to the caller's row order.  What Kaldi's agglomerative-cluster does over a PLDA score
matrix; the reference has no counterpart."""
import numpy as np
import torch

from . import _lib, ops
from .adaptive_score_normalization import _model_params
from .search import _search_device, embed_table


def _rank_roots(rep):
    """Dense ranks of the clusters in order of their smallest members, from absorbed-into links (rep[k] <= k)."""
    n = rep.size
    root = np.arange(n)
    for k in np.flatnonzero(rep != root):    # ascending: rep[k] < k, so the root of rep[k] is final when k comes up
        root[k] = root[rep[k]]
    rank = np.cumsum(rep == np.arange(n)) - 1
    return rank[root]


def _spk2utt(labels, n_clusters, ids, prefix):
    ids = list(ids)
    if len(ids) != int(labels.shape[0]):
        raise ValueError("one id per clustered row")
    total = int(n_clusters.sum())
    width = max(4, len(str(max(total - 1, 0))))
    out = [(f"{prefix}{c:0{width}d}", []) for c in range(total)]
    for i, c in enumerate(labels.tolist()):
        out[c][1].append(ids[i])
    return out


class Clustering:
    """The result of cluster(): `labels` (N,) int64 in the CALLER's row order, unique over the whole call (the clusters of
    problem p follow those of problem p - 1; inside a problem in order of their smallest member), `n_clusters` (P,),
    `merges` (numpy records a, b, value, size_after with problem-local SORTED row indices, problem by problem, max(n_p - 1, 0)
    each, the ones not executed (-1, -1, NaN, 0)), `offsets` (P + 1,) and `order` (N,): sorted row k is caller row order[k]."""

    def __init__(self, labels, n_clusters, merges, offsets, order, n_merges):
        self.labels, self.n_clusters, self.merges, self.offsets, self.order = labels, n_clusters, merges, offsets, order
        self.n_merges = n_merges

    def __len__(self):
        return int(self.labels.shape[0])

    def _moffs(self):
        n = np.diff(self.offsets)
        return np.concatenate([[0], np.cumsum(np.maximum(n - 1, 0))])

    def cut(self, threshold=None, n_clusters=None):
        """Re-cut on the host, no GPU call: per problem the recorded merges are applied in order while their value is
        >= threshold and more than n_clusters clusters remain -> a new Clustering.  The executed values never increase (all
        three linkages are reducible), so cutting a FULL dendrogram at t equals clustering with threshold = t."""
        if threshold is not None and threshold != threshold:
            raise ValueError("threshold must not be NaN")
        if n_clusters is not None and n_clusters < 1:
            raise ValueError("n_clusters must be at least 1")
        mo = self._moffs()
        labels = np.empty(len(self), np.int64)
        counts = np.zeros(self.offsets.size - 1, np.int32)
        done = np.zeros(self.offsets.size - 1, np.int32)
        base = 0
        for p in range(self.offsets.size - 1):
            r0, r1 = int(self.offsets[p]), int(self.offsets[p + 1])
            n = r1 - r0
            rep = np.arange(n)
            left = n
            for m in self.merges[mo[p]:mo[p + 1]]:
                if m["a"] < 0 or (threshold is not None and m["value"] < threshold) or \
                        (n_clusters is not None and left <= n_clusters):
                    break
                rep[m["b"]] = m["a"]
                left -= 1
            labels[self.order[r0:r1]] = base + _rank_roots(rep)
            counts[p], done[p] = left, n - left
            base += left
        merges = self.merges.copy()
        for p in range(counts.size):
            tail = merges[mo[p] + done[p]:mo[p + 1]]
            tail["a"], tail["b"], tail["value"], tail["size_after"] = -1, -1, np.nan, 0
        return Clustering(labels, counts, merges, self.offsets, self.order, done)

    def spk2utt(self, ids, prefix="c"):
        """[(cluster name, [id, ...]), ...] in label order, ids in the caller's row order: what backend.class_layout,
        fit_backend, InitFromXvectors and the loaders take as a spk2utt."""
        return _spk2utt(self.labels, self.n_clusters, ids, prefix)


def _group_order(groups, N):
    """(order (N,) int64: caller rows sorted stably by group, offsets (P + 1,) int64)."""
    if groups is None:
        return np.arange(N, dtype=np.int64), np.array([0, N], np.int64)
    g = np.asarray(groups.cpu() if isinstance(groups, torch.Tensor) else groups)
    if g.shape != (N,):
        raise ValueError(f"groups must name one group per row: ({N},), got {g.shape}")
    _, inv, counts = np.unique(g, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable").astype(np.int64)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def cluster(model, x, groups=None, threshold=float("-inf"), min_clusters=1, linkage="average"):
    """Cluster the rows of x (whatever model.extract_plda_embeddings takes: x-vectors, or features for an extractor-backed
    model) under the model's score, each group of `groups` (N labels of any sortable kind; None: one group) on its own ->
    Clustering.  Merging stops before the first linkage value < threshold or at min_clusters clusters per group;
    threshold = -inf, min_clusters = 1 records the full dendrogram, which Clustering.cut re-cuts without the GPU."""
    if not hasattr(model, "P_sqrt") or not hasattr(model, "centering_and_wccn_plda"):
        raise NotImplementedError("cluster scores with the NeuralPlda score (P_sqrt, Q); this model has another head")
    if linkage not in ops.AHC_LINKAGES:
        raise ValueError(f"linkage must be one of {sorted(ops.AHC_LINKAGES)}")
    threshold = float(threshold)
    if threshold != threshold or int(min_clusters) < 1:
        raise ValueError("threshold must not be NaN and min_clusters must be at least 1")
    dev = _search_device(model, x)
    with torch.no_grad():
        packed = ops.pack_params(*_model_params(model, dev))
    z, q = embed_table(model, x, packed)
    N = z.shape[0]
    order, offsets = _group_order(groups, N)
    if groups is not None:
        idx = torch.from_numpy(order).to(dev)
        z, q = z.index_select(0, idx), q.index_select(0, idx)
    offs = ops.RaggedOffsets(offsets, dev)
    S = ops.score_matrix(z, q, packed, offs)
    merges, n_merges, n_clusters, labels = ops.ahc(S, offs, linkage, threshold, int(min_clusters))
    n_clusters = n_clusters.cpu().numpy()
    local = labels.cpu().numpy().astype(np.int64)
    base = np.concatenate([[0], np.cumsum(n_clusters)])[:-1]
    out = np.empty(N, np.int64)
    out[order] = local + np.repeat(base, np.diff(offsets))
    rec = merges.cpu().numpy().view(ops.AHC_MERGE_DTYPE).reshape(-1)
    return Clustering(out, n_clusters, rec, offsets, order, n_merges.cpu().numpy())


class SpectralClustering:
    """The result of spectral_cluster(): `labels` (N,) int64 in the CALLER's row order, unique over the whole call (as
    Clustering), `n_clusters` (P,), `offsets` (P + 1,) and `order` (N,) as in Clustering, `candidates` (C,) the neighbour
    counts tried, `neighbours` (P,) the count chosen per problem, `chosen` (P,) its index, `eigenvalues` (P, C,
    max_clusters + 2: the K + 1 smallest of each cell, NaN, the largest in the last slot), `kstar` and `ratio` (P, C),
    `n_sweeps` (P, C) and `n_kmeans_iters` (P,)."""

    def __init__(self, labels, n_clusters, offsets, order, candidates, chosen, eigenvalues, kstar, ratio, n_sweeps,
                 n_kmeans_iters):
        self.labels, self.n_clusters, self.offsets, self.order = labels, n_clusters, offsets, order
        self.candidates, self.chosen, self.neighbours = candidates, chosen, candidates[chosen]
        self.eigenvalues, self.kstar, self.ratio, self.n_sweeps = eigenvalues, kstar, ratio, n_sweeps
        self.n_kmeans_iters = n_kmeans_iters

    def __len__(self):
        return int(self.labels.shape[0])

    def spk2utt(self, ids, prefix="c"):
        """As Clustering.spk2utt."""
        return _spk2utt(self.labels, self.n_clusters, ids, prefix)


def _spectral_batches(offsets, C, limit):
    """Runs of whole problems whose workspace fits `limit` bytes (None: one run) -> [(first problem, end problem), ...]."""
    P = offsets.size - 1
    if limit is None or P == 0:
        return [(0, P)]
    out, p0 = [], 0
    while p0 < P:
        p1 = p0 + 1
        if ops.spectral_workspace_bytes(offsets[p0:p1 + 1] - offsets[p0], C) > int(limit):
            raise ValueError(f"workspace_bytes = {int(limit)} does not hold problem {p0} alone "
                             f"({ops.spectral_workspace_bytes(offsets[p0:p1 + 1] - offsets[p0], C)} bytes)")
        while p1 < P and ops.spectral_workspace_bytes(offsets[p0:p1 + 2] - offsets[p0], C) <= int(limit):
            p1 += 1
        out.append((p0, p1))
        p0 = p1
    return out


def spectral_cluster(model, x, groups=None, neighbours=None, min_clusters=1, max_clusters=16, workspace_bytes=None,
                     max_iters=100):
    """Spectral clustering of the rows of x (as cluster()) under the model's score, each group on its own, with the neighbour
    count of the affinity graph tuned per group by the normalised maximum eigengap (NME-SC; csrc/nplda_spectral.hip,
    design/k25_spectral.md) -> SpectralClustering.  No threshold: the number of clusters of a group, between min_clusters
    and max_clusters, is read from the eigengap.  neighbours: None (ops.SPECTRAL_NEIGHBOURS), a strictly increasing list of
    candidates, or one int.  workspace_bytes: the groups are worked through in runs of whole groups whose workspace fits
    (the result does not change by a bit).  Raises where a group's eigensolver did not converge."""
    if not hasattr(model, "P_sqrt") or not hasattr(model, "centering_and_wccn_plda"):
        raise NotImplementedError("spectral_cluster scores with the NeuralPlda score (P_sqrt, Q); this model has another head")
    cand = np.atleast_1d(np.asarray(ops.SPECTRAL_NEIGHBOURS if neighbours is None else neighbours))
    dev = _search_device(model, x)
    with torch.no_grad():
        packed = ops.pack_params(*_model_params(model, dev))
    z, q = embed_table(model, x, packed)
    N = z.shape[0]
    order, offsets = _group_order(groups, N)
    limit = int(_lib.load().nplda_spectral_max_n())
    if offsets.size > 1 and int(np.diff(offsets).max()) > limit:
        raise ValueError(f"a group has {int(np.diff(offsets).max())} rows, spectral_cluster takes at most {limit}")
    if groups is not None:
        idx = torch.from_numpy(order).to(dev)
        z, q = z.index_select(0, idx), q.index_select(0, idx)
    parts = []
    for p0, p1 in _spectral_batches(offsets, cand.size, workspace_bytes):
        r0, r1 = int(offsets[p0]), int(offsets[p1])
        offs = ops.RaggedOffsets(offsets[p0:p1 + 1] - r0, dev)
        S = ops.score_matrix(z[r0:r1], q[r0:r1], packed, offs)
        parts.append(ops.spectral(S, offs, cand, int(min_clusters), int(max_clusters), int(max_iters)))
    cat = lambda name: torch.cat([getattr(r, name) for r in parts]).cpu().numpy()  # noqa: E731
    conv = cat("converged")
    if not conv.all():
        p, c = np.argwhere(conv == 0)[0]
        raise _lib.NpldaHipError(f"spectral_cluster: the eigensolver of group {p} (candidate {int(cand[c])}) did not converge "
                                 f"within {int(_lib.load().nplda_spectral_max_sweeps())} sweeps")
    n_clusters = cat("n_clusters")
    base = np.concatenate([[0], np.cumsum(n_clusters)])[:-1]
    out = np.empty(N, np.int64)
    out[order] = cat("labels").astype(np.int64) + np.repeat(base, np.diff(offsets))
    return SpectralClustering(out, n_clusters, offsets, order, cand.astype(np.int64), cat("chosen").astype(np.int64),
                              cat("eigenvalues"), cat("kstar"), cat("ratio"), cat("n_sweeps"), cat("n_kmeans_iters"))


class Refined:
    """The result of vb_refine(): `labels` (N,) int64 in the CALLER's row order, unique over the whole call (the speakers of
    group p follow those of group p - 1; inside a group in order of their slot), `n_clusters` (P,) speakers that own a row,
    `gamma` and `pi` (lists, one per group: (T_p, S_p) posteriors with rows in the group's time order, and (S_p,) priors, over
    the S_p slots the initial clustering had), `elbo` (P, max_iters; NaN where not executed), `n_iters` (P,), `offsets` and
    `order` as in Clustering."""

    def __init__(self, labels, n_clusters, gamma, pi, elbo, n_iters, offsets, order):
        self.labels, self.n_clusters, self.gamma, self.pi, self.elbo = labels, n_clusters, gamma, pi, elbo
        self.n_iters, self.offsets, self.order = n_iters, offsets, order

    def __len__(self):
        return int(self.labels.shape[0])

    def spk2utt(self, ids, prefix="c"):
        """As Clustering.spk2utt."""
        return _spk2utt(self.labels, self.n_clusters, ids, prefix)


def _local_init(init, order, offsets):
    """(labels (N,) int32 in sorted row order and local to each group, S (P,) slots per group) of a Clustering or of an
    integer label array (local per group or global: each group's distinct values are ranked)."""
    N, P = order.size, offsets.size - 1
    if isinstance(init, (Clustering, SpectralClustering)):
        if len(init) != N or not np.array_equal(init.offsets, offsets) or not np.array_equal(init.order, order):
            raise ValueError("init must come from cluster() on the same x and groups")
        S = np.asarray(init.n_clusters, np.int64)
        base = np.concatenate([[0], np.cumsum(S)])[:-1]
        return (init.labels[order] - np.repeat(base, np.diff(offsets))).astype(np.int32), S
    lab = np.asarray(init.cpu() if isinstance(init, torch.Tensor) else init)
    if lab.shape != (N,) or lab.dtype.kind not in "iu":
        raise ValueError(f"init must be a Clustering or ({N},) integer labels")
    lab = lab[order]
    out, S = np.empty(N, np.int32), np.zeros(P, np.int64)
    for p in range(P):
        r0, r1 = int(offsets[p]), int(offsets[p + 1])
        u, inv = np.unique(lab[r0:r1], return_inverse=True)
        out[r0:r1], S[p] = inv, u.size
    return out, S


def vb_refine(model, x, init, psi, groups=None, **vb):
    """Refine a clustering of the rows of x by VB-HMM resegmentation (VBx), each group of `groups` on its own -> Refined.
    The rows of a group are taken IN THE CALLER'S ORDER, AND THAT ORDER IS THE TIME ORDER of the HMM: pass the segments of a
    recording in the order they were spoken (groups may interleave; the order inside each group is kept).  `init`: the
    Clustering that cluster() returned for the same x and groups (over-clustered: its clusters are the speaker slots), the
    SpectralClustering of spectral_cluster(), or
    (N,) integer labels, local per group or global.  `psi`: (D2,) between-class variances of the PLDA model in the space of
    model.extract_plda_embeddings (backend.Backend.psi, kaldi_format.read_plda).  **vb: Fa, Fb, loop_prob, epsilon,
    init_smoothing, max_iters of ops.vbhmm."""
    if not hasattr(model, "P_sqrt") or not hasattr(model, "centering_and_wccn_plda"):
        raise NotImplementedError("vb_refine works on the NeuralPlda embeddings (P_sqrt, Q); this model has another head")
    dev = _search_device(model, x)
    with torch.no_grad():
        packed = ops.pack_params(*_model_params(model, dev))
    z, _ = embed_table(model, x, packed)
    N = z.shape[0]
    order, offsets = _group_order(groups, N)
    local, S = _local_init(init, order, offsets)
    limit = int(_lib.load().nplda_vbhmm_max_speakers())
    if S.size and int(S.max()) > limit:
        raise ValueError(f"a group has {int(S.max())} clusters, vb_refine takes at most {limit} speaker slots per group: "
                         f"cut the initial clustering first, e.g. init.cut(n_clusters={limit})")
    if groups is not None:
        z = z.index_select(0, torch.from_numpy(order).to(dev))
    offs = ops.RaggedOffsets(offsets, dev)
    spk = np.concatenate([[0], np.cumsum(S)]).astype(np.int64)
    gamma, pi, elbo, n_iters, labels, n_spk = ops.vbhmm(z, offs, ops.RaggedOffsets(spk, dev), psi,
                                                        labels_init=torch.from_numpy(local).to(dev), **vb)
    n_spk = n_spk.cpu().numpy()
    base = np.concatenate([[0], np.cumsum(n_spk)])[:-1]
    out = np.empty(N, np.int64)
    out[order] = labels.cpu().numpy().astype(np.int64) + np.repeat(base, np.diff(offsets))
    T = np.diff(offsets)
    goff = np.concatenate([[0], np.cumsum(T * S)])
    gamma, pi = gamma.cpu().numpy(), pi.cpu().numpy()
    gl = [gamma[goff[p]:goff[p + 1]].reshape(int(T[p]), int(S[p])) for p in range(T.size)]
    pl = [pi[spk[p]:spk[p + 1]] for p in range(T.size)]
    return Refined(out, n_spk, gl, pl, elbo.cpu().numpy(), n_iters.cpu().numpy(), offsets, order)
