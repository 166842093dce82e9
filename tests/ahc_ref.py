"""Numpy float64 twin and case generators of the agglomerative clustering (csrc/nplda_ahc.hip; a plain helper of
tests/test_ahc_*.py).  design/k21_ahc.md states the contract; this file performs the same single additions and the same
division, so the kernel must agree with it bit for bit on ANY float32 matrix (NaN aside).

Every cluster is named by its smallest member row.  A step merges the live pair (a, b), a < b, with the LARGEST linkage
value; np.argmax over the masked upper triangle in row-major order returns the first maximum, which IS the tie rule (the
lexicographically lowest (a, b))."""
import numpy as np

LINKAGES = {"average": 0, "complete": 1, "single": 2}
MERGE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("value", "<f8"), ("size_after", "<i4"), ("reserved", "<i4")])
assert MERGE_DTYPE.itemsize == 24


def empty_records(m):
    """m records as the kernel leaves the ones it did not execute: (-1, -1, NaN, 0)."""
    r = np.zeros(m, MERGE_DTYPE)
    r["a"], r["b"], r["value"] = -1, -1, np.nan
    return r


def labels_of(rep):
    """Dense ranks of the clusters in order of their smallest members, from the absorbed-into links (rep[k] <= k)."""
    n = rep.size
    root = np.arange(n)
    for k in range(n):                       # rep[k] < k for an absorbed k: its root is known when k comes up
        root[k] = k if rep[k] == k else root[rep[k]]
    rank = np.cumsum(rep == np.arange(n)) - 1
    return rank[root].astype(np.int32)


def ahc(S, linkage="average", threshold=-np.inf, min_clusters=1):
    """One problem: S (n, n), only its strict upper triangle is read -> (merges (n - 1 records, the tail not executed),
    n_merges, n_clusters, labels int32)."""
    link = LINKAGES[linkage] if isinstance(linkage, str) else int(linkage)
    S = np.asarray(S)
    n = S.shape[0]
    rec = empty_records(max(n - 1, 0))
    if n <= 1:
        return rec, 0, n, np.zeros(n, np.int32)
    up = np.triu(np.ones((n, n), bool), 1)
    D = np.where(up, S, 0).astype(np.float64)
    D = D + D.T                                        # (x + 0: exact)
    M = np.where(up, D, -np.inf)                       # linkage values of the live pairs a < b, -inf elsewhere
    size = np.ones(n, np.int64)
    alive = np.ones(n, bool)
    rep = np.arange(n)
    done = 0
    while n - done > min_clusters:
        a, b = divmod(int(np.argmax(M)), n)
        V = M[a, b]
        if not a < b or V < threshold:
            break
        k = np.flatnonzero(alive)
        k = k[(k != a) & (k != b)]
        da, db = D[a, k], D[b, k]
        nw = da + db if link == 0 else np.where(db < da, db, da) if link == 1 else np.where(db > da, db, da)
        D[a, k] = nw
        D[k, a] = nw
        size[a] += size[b]
        alive[b] = False
        rep[b] = a
        val = nw / (size[k] * size[a]).astype(np.float64) if link == 0 else nw
        M[b, :] = -np.inf
        M[:, b] = -np.inf
        lo = k < a
        M[k[lo], a] = val[lo]
        M[a, k[~lo]] = val[~lo]
        rec[done] = (a, b, V, size[a], 0)
        done += 1
    return rec, done, n - done, labels_of(rep)


def cut(rec, n, threshold=None, n_clusters=None):
    """Host re-cut of a full dendrogram: apply the records in order while value >= threshold and more than n_clusters
    clusters remain -> labels.  The executed values are non-increasing, so this equals a run with that threshold."""
    rep = np.arange(n)
    left = n
    for r in rec:
        if r["a"] < 0 or (threshold is not None and r["value"] < threshold) or (n_clusters is not None and left <= n_clusters):
            break
        rep[r["b"]] = r["a"]
        left -= 1
    return labels_of(rep)


def batch(mats, linkage, threshold=-np.inf, min_clusters=1):
    """The outputs of one call over the problems `mats`: (merges, n_merges, n_clusters, labels), concatenated."""
    out = [ahc(m, linkage, threshold, min_clusters) for m in mats]
    return (np.concatenate([o[0] for o in out]) if out else empty_records(0), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.int32), np.concatenate([o[3] for o in out]) if out else np.zeros(0, np.int32))


def flat(mats):
    """(flat float32 matrices one after the other, offsets int64)."""
    offs = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    data = np.concatenate([np.asarray(m, np.float32).ravel() for m in mats]) if mats else np.zeros(0, np.float32)
    return data.astype(np.float32), offs


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def int_matrix(n, seed):
    """Symmetric small integers in [-8, 8]: every fp64 sum is exact in any order, and ties occur at nearly every step."""
    rng = np.random.default_rng([seed, n])
    A = np.triu(rng.integers(-8, 9, (n, n)), 1)
    return (A + A.T).astype(np.float32)


def equal_matrix(n, v=1.0):
    return np.full((n, n), v, np.float32)


def ordered_matrix(n, ascending=True):
    """Scores that ascend (descend) with (i, j) in row-major order over the upper triangle; integers below 2^24."""
    S = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    r = np.arange(iu[0].size, dtype=np.float32)
    S[iu] = r if ascending else -r
    return S + S.T


def exactness_bound(S, n):
    """Largest magnitude any numerator can reach: n^2 max|S|; below 2^53 with integer entries every sum is exact."""
    return float(n) * n * float(np.abs(S).max() if S.size else 0.0)
