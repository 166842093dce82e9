"""CPU twin of the group bootstrap (design/k20_bootstrap.md), written from the note: the counter-based generator in
uint64 arrays, the draw counts by np.bincount, and per replicate the weighted sweep of the once-sorted trial list in
numpy fp64 (integer counts in int64)."""
import math

import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
M64 = (1 << 64) - 1


def mix(x):
    """The splitmix64 finaliser on uint64 arrays (arithmetic mod 2^64)."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def draws(seed, b, side, G):
    """The G group indices replicate b >= 1 draws on `side` (0 or 1)."""
    with np.errstate(over="ignore"):
        key = mix(np.uint64(int(seed) & M64) + GOLD * np.uint64(2 * b + side + 1))
        x = mix(key + GOLD * np.arange(1, G + 1, dtype=np.uint64))
        return (((x >> np.uint64(32)) * np.uint64(G)) >> np.uint64(32)).astype(np.int64)


def counts(seed, b, side, G):
    """How often every group was drawn: (G,) int64; replicate 0 is the point estimate, all ones."""
    if b == 0:
        return np.ones(G, dtype=np.int64)
    return np.bincount(draws(seed, b, side, G), minlength=G).astype(np.int64)


def column_count(K, llr):
    return K + 1 + (K + 1 if llr else 0)


def sort_trials(scores, target):
    """-> (order, key, code, start): the stable order by score of ALL trials (a NaN score sorts as -inf and is dead),
    label codes 1 target / 0 non-target / 2 neither / 3 dead, and the starts of the runs of equal keys."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(target, dtype=np.float32)
    nan = np.isnan(s)
    key = np.where(nan, -np.inf, s.astype(np.float64))
    code = np.where(y > 0.5, 1, np.where(y < 0.5, 0, 2))
    code = np.where(nan, 3, code)
    order = np.argsort(key, kind="stable")
    key, code = key[order], code[order]
    start = np.concatenate(([True], key[1:] != key[:-1]))
    return order, key, code, start


def sweep(key, code, start, w, betas, llr=False, sp=None):
    """One row: the metrics of the sorted list under the integer weights w (dead trials weigh 0) -> (values (ncol,), N_t,
    N_n).  Candidate thresholds are the run starts, with the targets strictly below and the non-targets at or above."""
    K = len(betas)
    w = np.where(code == 3, 0, np.asarray(w, dtype=np.int64))
    wt, wn = np.where(code == 1, w, 0), np.where(code == 0, w, 0)
    Nt, Nn = int(wt.sum()), int(wn.sum())
    row = np.full(column_count(K, llr), np.nan)
    if Nt == 0 or Nn == 0:
        return row, Nt, Nn
    below_t = np.cumsum(wt) - wt  # exclusive
    at_above_n = Nn - (np.cumsum(wn) - wn)
    pm = below_t[start] / Nt
    pf = at_above_n[start] / Nn
    pos = np.flatnonzero(start)
    for k, b in enumerate(betas):
        row[k] = min(float((pm + b * pf).min()), Nt / Nt)  # +inf: P_miss = 1, P_fa = 0
    last = int(np.flatnonzero(w > 0).max())  # thresholds beyond the last weighted trial are not in the expanded list
    ok = (pm - pf >= 0) & (pos <= last)
    if not ok.any():
        row[K] = 0.5  # (P_miss + P_fa) / 2 of the first threshold: (0 + 1) / 2
    else:
        i = int(np.argmax(ok))
        x0, x1 = pm[i - 1] - pf[i - 1], pm[i] - pf[i]
        ww = -x0 / (x1 - x0) if x1 != x0 else 0.5
        row[K] = pm[i - 1] + ww * (pm[i] - pm[i - 1])
    if llr:
        for k, b in enumerate(betas):
            th = math.log(b)
            miss, fa = int(wt[key < th].sum()), int(wn[key >= th].sum())
            row[K + 1 + k] = miss / Nt + b * (fa / Nn)
        with np.errstate(over="ignore"):
            ct = float((wt[wt > 0] * sp[wt > 0]).sum())
            cn = float((wn[wn > 0] * sp[wn > 0]).sum())
        row[2 * K + 1] = 0.5 * (ct * 1.4426950408889634 / Nt + cn * 1.4426950408889634 / Nn)
    return row, Nt, Nn


def softplus_terms(key, code):
    """log(1 + exp(-s)) on targets, log(1 + exp(s)) on non-targets, from the fp32 score in fp64; 0 elsewhere."""
    v = key.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sp = np.log1p(np.exp(-np.abs(v))) + np.maximum(np.where(code == 1, -v, v), 0.0)
    return np.where(code <= 1, sp, 0.0)


def bootstrap(scores, target, g1, G1, g2=None, G2=0, n_boot=10, seed=0, betas=(1.0,), llr=False):
    """-> (out (n_boot + 1, ncol) float64, totals (n_boot + 1, 2) int64)."""
    order, key, code, start = sort_trials(scores, target)
    g1 = np.asarray(g1, dtype=np.int64)[order]
    g2 = None if g2 is None else np.asarray(g2, dtype=np.int64)[order]
    sp = softplus_terms(key, code) if llr else None
    betas = [float(b) for b in betas]
    out = np.empty((n_boot + 1, column_count(len(betas), llr)))
    totals = np.empty((n_boot + 1, 2), dtype=np.int64)
    for b in range(n_boot + 1):
        w = counts(seed, b, 0, G1)[g1]
        if g2 is not None:
            w = w * counts(seed, b, 1, G2)[g2]
        out[b], totals[b, 0], totals[b, 1] = sweep(key, code, start, w, betas, llr, sp)
    return out, totals
