"""The numpy twin of csrc/nplda_spectral.hip (include/nplda_hip.h has the definitions), stage by stage, and the planted
partitions the tests cluster.  Nothing here uses ndarray.sum where the order of a floating-point sum matters."""
import numpy as np

MAX_SWEEPS = 30


def planted(n, clusters, sep, seed, equal=True):
    """S = (G + G^T) / 2 + sep [same cluster], G standard normal, rounded to fp32, zero diagonal; clusters contiguous, of
    near-equal size or (equal=False) of random sizes >= 2 -> (S (n, n) float32, truth (n,) int)."""
    rng = np.random.default_rng(seed)
    if equal:
        truth = (np.arange(n) * clusters) // n
    else:
        cuts = np.sort(rng.choice(np.arange(1, n // 2), clusters - 1, replace=False)) * 2 if clusters > 1 else np.array([], int)
        truth = np.searchsorted(cuts, np.arange(n), side="right")
    G = rng.standard_normal((n, n))
    S = (G + G.T) / 2 + sep * (truth[:, None] == truth[None, :])
    S = S.astype(np.float32)
    np.fill_diagonal(S, 0.0)
    return S, truth


def tie_heavy(n, seed):
    """A symmetric fp32 matrix whose scores take three values (one of them -0.0 / +0.0 mixed)."""
    rng = np.random.default_rng(seed)
    v = np.array([-1.5, 0.0, 2.0], np.float32)[rng.integers(0, 3, (n, n))]
    S = np.triu(v, 1) + np.triu(v, 1).T
    Z = (S == 0) & (rng.random((n, n)) < 0.5)
    S[Z] = np.float32(-0.0)
    np.fill_diagonal(S, 0.0)
    return S


def graph(S, c):
    """-> (L (n, n) float64, d (n,) float64): the m = min(c, n - 1) largest off-diagonal scores of each row, equal scores by
    ascending column, symmetrised by the mean."""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    m = min(int(c), n - 1)
    B = np.zeros((n, n))
    for i in range(n):
        cols = np.array([j for j in range(n) if j != i], int)
        if m > 0:
            keys = -(S[i, cols].astype(np.float64) + 0.0)
            take = cols[np.lexsort((cols, keys))[:m]]
            B[i, take] = 1.0
    A = (B + B.T) / 2
    d = np.zeros(n)
    for j in range(n):
        d = d + A[:, j]        # multiples of 1/2: exact in any order
    return np.diag(d) - A, d


def _pairs(r, ne):
    """The ne / 2 pairs of round r of the circle method with player ne - 1 fixed -> (p, q) arrays, p < q."""
    i = np.arange(ne // 2)
    mod = ne - 1
    x = (r + i) % mod
    y = np.where(i == 0, mod, (r - i) % mod)
    return np.minimum(x, y), np.maximum(x, y)


def jacobi(L, dtype=np.float64, vectors=True, max_sweeps=MAX_SWEEPS):
    """Cyclic Jacobi with the kernel's ordering, threshold and formulae in `dtype` (float64, or np.longdouble with the
    threshold scaled by that type's epsilon) -> (eigenvalues ascending (n,), eigenvectors as ROWS in that order or None,
    n_sweeps, converged).  Equal computed eigenvalues keep their order on the diagonal."""
    L = np.asarray(L)
    n = L.shape[0]
    if n == 0:
        return np.zeros(0, dtype), (np.zeros((0, 0), dtype) if vectors else None), 0, True
    ne = n + (n & 1)
    A = np.zeros((ne, ne), dtype)
    A[:n, :n] = L
    W = np.eye(ne, dtype=dtype) if vectors else None
    sq = A * A
    ss = dtype(0)
    for v in sq.ravel():
        ss = ss + v            # exact
    thr = np.sqrt(ss) * dtype(np.finfo(dtype).eps / 2) / dtype(ne)
    one, two = dtype(1), dtype(2)
    sweeps, conv = 0, False
    while sweeps < max_sweeps and not conv:
        anyrot = False
        for r in range(ne - 1):
            p, q = _pairs(r, ne)
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            rot = np.abs(apq) > thr
            if not rot.any():
                continue
            anyrot = True
            safe = np.where(rot, apq, one)
            theta = (aqq - app) / (two * safe)
            t = one / (np.abs(theta) + np.sqrt(theta * theta + one))
            t = np.where(theta < 0, -t, t)
            c = one / np.sqrt(t * t + one)
            s = t * c
            c, s, t = np.where(rot, c, one), np.where(rot, s, 0 * one), np.where(rot, t, 0 * one)
            m00, m01, m10, m11 = A[np.ix_(p, p)], A[np.ix_(p, q)], A[np.ix_(q, p)], A[np.ix_(q, q)]
            cc, cs, sc, s2 = np.outer(c, c), np.outer(c, s), np.outer(s, c), np.outer(s, s)
            n00 = (cc * m00 + s2 * m11) - (cs * m01 + sc * m10)
            n01 = (cc * m01 - s2 * m10) + (cs * m00 - sc * m11)
            n10 = (cc * m10 - s2 * m01) + (sc * m00 - cs * m11)
            n11 = (s2 * m00 + cc * m11) + (cs * m10 + sc * m01)
            k = np.flatnonzero(rot)
            x = t[k] * apq[k]
            n00[k, k], n11[k, k], n01[k, k], n10[k, k] = app[k] - x, aqq[k] + x, 0, 0
            A[np.ix_(p, p)], A[np.ix_(p, q)], A[np.ix_(q, p)], A[np.ix_(q, q)] = n00, n01, n10, n11
            if vectors:
                w0, w1 = W[p], W[q]
                W[p], W[q] = c[:, None] * w0 - s[:, None] * w1, s[:, None] * w0 + c[:, None] * w1
        sweeps += 1
        conv = not anyrot
    dg = np.diag(A)[:n]
    order = np.argsort(dg, kind="stable")
    V = None
    if vectors:
        V = W[order][:, :n].copy()
        for r in range(n):
            s2 = dtype(0)
            for v in V[r]:
                s2 = s2 + v * v
            V[r] = V[r] / np.sqrt(s2)
    return dg[order].copy(), V, sweeps, conv


def choose(ev, c, n, min_clusters=1, max_clusters=64):
    """The count of one cell from its eigenvalue slots (max_clusters + 2 of them: the K + 1 smallest, NaN, the largest last)
    -> (k*, r)."""
    kfloor = max(int(min_clusters), 1)
    K = min(int(max_clusters), n - 1)
    degenerate = (min(kfloor, max(n, 1)), np.inf)
    if n <= 1 or kfloor > K:
        return degenerate
    ev = np.asarray(ev, np.float64)
    top = ev[-1]
    best, gap = None, None
    for k in range(kfloor, K + 1):
        g = ev[k] - ev[k - 1]
        if best is None or g > gap:
            best, gap = k, g
    if not top > 0.0:
        return degenerate
    g = gap / top
    if not g > 0.0:
        return degenerate
    return best, np.float64(c) / g


def _dist2(E, cen):
    acc = np.zeros(E.shape[0])
    for j in range(E.shape[1]):
        diff = E[:, j] - cen[j]
        acc = acc + diff * diff
    return acc


def kmeans(E, k, max_iters=100):
    """-> (labels (n,) int32, n_clusters, n_iters): farthest-first centres from row 0, Lloyd iterations until an assignment
    repeats, sums in explicit row order."""
    E = np.asarray(E, np.float64)
    n, d = E.shape
    if n == 0:
        return np.zeros(0, np.int32), 0, 0
    k = min(int(k), n)
    cen = np.empty((k, d))
    cen[0] = E[0]
    mind = _dist2(E, cen[0])
    for c in range(1, k):
        row = int(np.argmax(mind))           # the first of equal maxima
        cen[c] = E[row]
        mind = np.minimum(mind, _dist2(E, cen[c]))
    asg, iters = None, 0
    for it in range(int(max_iters)):
        D = np.stack([_dist2(E, cen[c]) for c in range(k)], axis=1)
        new = np.argmin(D, axis=1)           # the first of equal minima
        iters += 1
        if asg is not None and np.array_equal(new, asg):
            break
        asg = new
        for c in range(k):
            rows = np.flatnonzero(asg == c)
            if rows.size:
                s = np.zeros(d)
                for i in rows:
                    s = s + E[i]
                cen[c] = s / np.float64(rows.size)
    first = np.array([np.flatnonzero(asg == c)[0] if (asg == c).any() else n for c in range(k)])
    rank = np.array([(first < first[c]).sum() for c in range(k)])
    return rank[asg].astype(np.int32), int((first < n).sum()), iters


def spectral(S, neighbours, min_clusters=1, max_clusters=64, max_iters=100, dtype=np.float64):
    """One problem through every stage -> dict(eigenvalues (C, max_clusters + 2), kstar, ratio, n_sweeps, converged, chosen,
    k, E, labels, n_clusters, n_kmeans_iters, margins (C,): (largest - second largest gap) / l_n of each cell)."""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    C = len(neighbours)
    ev = np.full((C, max_clusters + 2), np.nan)
    kstar, ratio = np.zeros(C, np.int32), np.full(C, np.inf)
    sweeps, conv, vecs, margins = np.zeros(C, np.int32), np.ones(C, bool), [], np.full(C, np.nan)
    K = min(max_clusters, n - 1)
    for ci, c in enumerate(neighbours):
        V = None
        if n > 0:
            lam, V, sweeps[ci], conv[ci] = jacobi(graph(S, c)[0], dtype)
            ev[ci, :K + 1], ev[ci, -1] = lam[:K + 1], lam[-1]
            gaps = np.sort(np.diff(lam[:K + 1])[max(min_clusters, 1) - 1:])
            if gaps.size >= 2 and lam[-1] > 0:
                margins[ci] = (gaps[-1] - gaps[-2]) / lam[-1]
        vecs.append(V)
        kstar[ci], ratio[ci] = choose(ev[ci], c, n, min_clusters, max_clusters)
    chosen = int(np.argmin(ratio))           # the first of equal minima
    k = min(int(kstar[chosen]), n)
    E = vecs[chosen][:k].T.copy() if n > 0 else np.zeros((0, 0))
    labels, ncl, iters = kmeans(E, k, max_iters) if n > 0 else (np.zeros(0, np.int32), 0, 0)
    return dict(eigenvalues=ev, kstar=kstar, ratio=ratio, n_sweeps=sweeps, converged=conv, chosen=chosen, k=k, E=E, labels=labels,
                n_clusters=ncl, n_kmeans_iters=iters, margins=margins)


# ---- the spectrum cases of tests/test_spectral_gpu.py and their recorded references ---------------------------------------

SPECTRUM_NS = (2, 3, 17, 63, 64, 65, 128, 129, 130, 257)   # both sides of the wave, of nplda_spectral_small_n() and of a block
SPECTRUM_CANDIDATES = (4, 12)
GOLDEN = "spectral_spectrum.npz"


def spectrum_case(n):
    return planted(n, 3 if n >= 9 else 1, 3.0, 1000 + n)[0]


def spectrum_reference(n, c):
    """-> (eigenvalues of the np.longdouble run as a float64 pair hi + lo, eigenvalues of the float64 run)."""
    L = graph(spectrum_case(n), c)[0]
    ld = jacobi(L, np.longdouble, vectors=False)[0]
    hi = ld.astype(np.float64)
    return hi, (ld - hi).astype(np.float64), jacobi(L, np.float64, vectors=False)[0]


def write_golden(path):
    """Record spectrum_reference for every case (python -c "from tests import spectral_ref as s; s.write_golden(...)"): the
    long-double run of the largest cases takes a minute, the file a few kilobytes."""
    out = {}
    for n in SPECTRUM_NS:
        for c in SPECTRUM_CANDIDATES:
            out[f"hi_{n}_{c}"], out[f"lo_{n}_{c}"], out[f"f64_{n}_{c}"] = spectrum_reference(n, c)
    np.savez(path, **out)
