"""CPU reference of the PAV / ROC-convex-hull feature (design/k18_pav_rocch.md), written from the definitions: the O(n)
integer stack over the cumulative (trials, targets) points, then min Cllr, the ROCCH equal error rate, the block
log-likelihood ratios and the calibration map in numpy fp64.  Hull decisions use Python integers only."""
import math

import numpy as np


def bins(scores, target):
    """-> (values (M,), n (M,) int, t (M,) int, N_t, N_n): the kept trials (label > 0.5 target, < 0.5 non-target, score not
    NaN) sorted by score, equal scores (==) as one bin.  values holds (first, last) score of each bin's run."""
    s = np.asarray(scores)
    y = np.asarray(target, dtype=np.float64)
    keep = ((y > 0.5) | (y < 0.5)) & ~np.isnan(s)
    s = s[keep].astype(np.float64)  # exact for fp32
    tg = (y[keep] > 0.5).astype(np.int64)
    order = np.argsort(s, kind="stable")
    s, tg = s[order], tg[order]
    if s.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return np.zeros((0, 2)), z, z, 0, 0
    new = np.flatnonzero(s[1:] != s[:-1]) + 1
    start = np.concatenate(([0], new))
    end = np.concatenate((new, [s.size]))
    ct = np.concatenate(([0], np.cumsum(tg)))
    n = end - start
    t = ct[end] - ct[start]
    vals = np.stack([s[start], s[end - 1]], axis=1)
    return vals, n.astype(np.int64), t.astype(np.int64), int(tg.sum()), int(s.size - tg.sum())


def hull(n, t):
    """Indices (into P_0 .. P_M) of the strict lower convex hull of the cumulative points: pop the top b while
    cross(b - a, c - b) <= 0."""
    xs = [0] + np.cumsum(np.asarray(n, dtype=np.int64)).tolist()
    ys = [0] + np.cumsum(np.asarray(t, dtype=np.int64)).tolist()
    st = []
    for c in range(len(xs)):
        cx, cy = xs[c], ys[c]
        while len(st) >= 2:
            a, b = st[-2], st[-1]
            if (xs[b] - xs[a]) * (cy - ys[b]) - (ys[b] - ys[a]) * (cx - xs[b]) > 0:
                break
            st.pop()
        st.append(c)
    return st


def fit(scores, target, laplace=True):
    """The block table and the counts: dict(lo, hi, n, t, llr, N_t, N_n, M, nb, min_cllr, rocch_eer)."""
    vals, n, t, Nt, Nn = bins(scores, target)
    M = n.size
    lo_v, hi_v = vals[:, 0], vals[:, 1]
    if laplace:
        n = np.concatenate(([2], n, [2]))
        t = np.concatenate(([1], t, [1]))
        lo_v = np.concatenate(([-np.inf], lo_v, [np.inf]))
        hi_v = np.concatenate(([-np.inf], hi_v, [np.inf]))
    real = np.ones(n.size, dtype=bool)
    if laplace:
        real[0] = real[-1] = False
    v = hull(n, t)
    cn = np.concatenate(([0], np.cumsum(n)))
    ct = np.concatenate(([0], np.cumsum(t)))
    nb = len(v) - 1
    bn = np.array([cn[v[b + 1]] - cn[v[b]] for b in range(nb)], dtype=np.int64)
    bt = np.array([ct[v[b + 1]] - ct[v[b]] for b in range(nb)], dtype=np.int64)
    lo, hi = np.empty(nb), np.empty(nb)
    for b in range(nb):
        k0, k1 = v[b], v[b + 1] - 1  # first and last bin of the block
        if real[k0:k1 + 1].any():
            first = k0 if real[k0] else k0 + 1
            last = k1 if real[k1] else k1 - 1
            lo[b], hi[b] = lo_v[first], hi_v[last]
        else:
            lo[b], hi[b] = lo_v[k0], hi_v[k1]
    Ntp, Nnp = (Nt + 2, Nn + 2) if laplace else (Nt, Nn)
    with np.errstate(divide="ignore", invalid="ignore"):
        llr = np.log(bt.astype(np.float64) / (bn - bt).astype(np.float64)) - np.log(np.float64(Ntp) / np.float64(Nnp))
    out = dict(lo=lo, hi=hi, n=bn, t=bt, llr=llr, N_t=Nt, N_n=Nn, M=M, nb=nb)
    out["min_cllr"], out["rocch_eer"] = block_metrics(bn, bt)
    return out


def block_metrics(bn, bt):
    """(min Cllr, ROCCH EER) of a block table, the class counts being its column sums."""
    bn = np.asarray(bn, dtype=np.int64)
    bt = np.asarray(bt, dtype=np.int64)
    Nt, Nn = int(bt.sum()), int((bn - bt).sum())
    if Nt == 0 or Nn == 0:
        return float("nan"), float("nan")
    t = bt.astype(np.float64)
    f = (bn - bt).astype(np.float64)
    rt, rn = np.float64(Nt) / np.float64(Nn), np.float64(Nn) / np.float64(Nt)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(t > 0, t * np.log1p(f / t * rt), 0.0)
        b = np.where(f > 0, f * np.log1p(t / f * rn), 0.0)
    mc = (math.fsum(a.tolist()) / Nt + math.fsum(b.tolist()) / Nn) / (2.0 * math.log(2.0))
    # vertices: T_v, F_v below the vertex; the sign of d_v = T_v / N_t - 1 + F_v / N_n in exact integers
    T = [0] + np.cumsum(bt).tolist()
    F = [0] + np.cumsum(bn - bt).tolist()
    eer = float("nan")
    for v in range(len(T) - 1):
        if T[v] * Nn + F[v] * Nt < Nt * Nn <= T[v + 1] * Nn + F[v + 1] * Nt:
            pm0, pf0 = np.float64(T[v]) / Nt, 1.0 - np.float64(F[v]) / Nn
            pm1, pf1 = np.float64(T[v + 1]) / Nt, 1.0 - np.float64(F[v + 1]) / Nn
            d0, d1 = pm0 - pf0, pm1 - pf1
            w = -d0 / (d1 - d0)
            eer = float(pm0 + w * (pm1 - pm0))
            break
    return float(mc), eer


def rocch(bn, bt):
    """(P_fa, P_miss) at the vertices."""
    bn = np.asarray(bn, dtype=np.int64)
    bt = np.asarray(bt, dtype=np.int64)
    T = np.concatenate(([0], np.cumsum(bt))).astype(np.float64)
    F = np.concatenate(([0], np.cumsum(bn - bt))).astype(np.float64)
    return 1.0 - F / F[-1], T / T[-1]


def apply(lo, hi, llr, scores):
    """The map of the issue's table, row by row, fp64."""
    lo, hi, llr = (np.asarray(x, dtype=np.float64) for x in (lo, hi, llr))
    s = np.asarray(scores, dtype=np.float64)
    out = np.empty(s.shape, dtype=np.float64)
    nb = lo.size
    for i, v in enumerate(s.tolist()):
        if v != v:
            out[i] = np.nan
            continue
        b = int(np.searchsorted(hi, v, side="left"))  # first block with hi >= v
        if b >= nb:
            out[i] = llr[nb - 1]
        elif lo[b] <= v or b == 0:
            out[i] = llr[b]
        else:
            h, l, y0, y1 = hi[b - 1], lo[b], llr[b - 1], llr[b]
            if np.isinf(h):
                out[i] = y0
            elif np.isinf(l):
                out[i] = y1
            elif np.isinf(y0):
                out[i] = y0
            elif np.isinf(y1):
                out[i] = y1
            else:
                w = (v - h) / (l - h)
                out[i] = min(max(y0 + w * (y1 - y0), y0), y1)
    return out


def fitted_values(scores, target):
    """p_k of every BIN (no Laplace rule): the isotonic regression of the labels on the scores."""
    _, n, t, _, _ = bins(scores, target)
    v = hull(n, t)
    cn = np.concatenate(([0], np.cumsum(n)))
    ct = np.concatenate(([0], np.cumsum(t)))
    p = np.empty(n.size)
    for b in range(len(v) - 1):
        p[v[b]:v[b + 1]] = (ct[v[b + 1]] - ct[v[b]]) / (cn[v[b + 1]] - cn[v[b]])
    return p, n, t
