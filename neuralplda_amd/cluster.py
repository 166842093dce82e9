"""Agglomerative clustering of embeddings under the model's own score (csrc/nplda_ahc.hip, design/k21_ahc.md).

Unlabelled x-vectors become pseudo-speakers: the set is embedded once (search.embed_table), every group of rows (one
recording, one domain, or the whole set) is one PROBLEM whose dense score matrix ops.score_matrix writes and ops.ahc
partitions, and the result maps back to the caller's row order.  What Kaldi's agglomerative-cluster does over a PLDA score
matrix; the reference has no counterpart."""
import numpy as np
import torch

from . import ops
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
        ids = list(ids)
        if len(ids) != len(self):
            raise ValueError("one id per clustered row")
        total = int(self.n_clusters.sum())
        width = max(4, len(str(max(total - 1, 0))))
        out = [(f"{prefix}{c:0{width}d}", []) for c in range(total)]
        for i, c in enumerate(self.labels.tolist()):
            out[c][1].append(ids[i])
        return out


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
