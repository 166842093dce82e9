"""NumPy twin of the detection-cost sweep (csrc/nplda_detcost.hip, design/k12_detcost.md): no torch, O(N log N).

sweep(s, t, betas, exact) states what nplda_detcost_sweep_f32 must return.

Classes: target t > 0.5, non-target t < 0.5, anything else excluded; a trial whose score is NaN is excluded whatever
its label.

Reference mode (exact=False) is NeuralPlda.minc with its quirks, float32 with one rounding per operation: thresholds
are the target scores in ascending order, the "count" is the last index of a where() (count - 1) or 1.0 when the set
is empty, and the normalisers are float32(sum t) and float32(sum (1 - t)) over ALL labels (excluded and NaN-score
trials too).  A cost that is NaN never wins; with no winner the result is NaN.

Exact mode (exact=True): the candidates are every distinct non-NaN score in ascending order (excluded trials'
scores too, -0.0 and +0.0 being one score), then the accept-nothing point (P_miss = Nt / max(Nt, 1), P_fa = 0,
threshold +inf).  Costs are exact rationals; a tie goes to the earlier candidate.  The EER is the kernel's: the
first candidate score with P_miss >= P_fa, linear interpolation from the previous one.

brute(s, t, betas) restates the reference-mode definition in O(N^2), for N <= 200.
"""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32


def classes(s, t):
    """-> (s, t as flat float32, target mask, non-target mask)."""
    s = np.asarray(s, dtype=F32).reshape(-1)
    t = np.asarray(t, dtype=F32).reshape(-1)
    if s.shape != t.shape:
        raise ValueError("scores and labels must have the same length")
    ok = ~np.isnan(s)
    return s, t, ok & (t > 0.5), ok & (t < 0.5)


def normalisers(t):
    """float32(sum t), float32(sum (1 - t)): each sum exact, rounded once (1 - t is formed in float32 as the reference does)."""
    t = np.asarray(t, dtype=F32).reshape(-1)
    return F32(math.fsum(t.astype(np.float64))), F32(math.fsum((F32(1) - t).astype(np.float64)))


def _first_min(c):
    """Index of the first smallest non-NaN entry, or None."""
    ok = np.nonzero(~np.isnan(c))[0]
    if ok.size == 0:
        return None
    return int(ok[int(np.argmin(c[ok]))])


def _average_f32(mincs):
    acc = mincs[0]
    for m in mincs[1:]:
        acc = F32(acc + m)
    return F32(acc / F32(len(mincs)))


def _sweep_reference(s, t, tgt, non, betas):
    K = len(betas)
    st, sn = np.sort(s[tgt]), np.sort(s[non])
    fnt, fnn = normalisers(t)
    minc, thr = np.full(K, np.nan, F32), np.full(K, np.nan, F32)
    if st.size:
        c_lt = np.searchsorted(st, st, side="left")
        c_ge = sn.size - np.searchsorted(sn, st, side="left")
        with np.errstate(all="ignore"):
            pm = np.where(c_lt > 0, c_lt - 1, 1).astype(F32) / fnt
            pf = np.where(c_ge > 0, c_ge - 1, 1).astype(F32) / fnn
            for k, b in enumerate(betas):
                c = pm + F32(b) * pf
                i = _first_min(c)
                if i is not None:
                    minc[k], thr[k] = c[i], st[i]
    with np.errstate(all="ignore"):
        avg = _average_f32([F32(m) for m in minc])
    return {"minc": minc, "thr": thr, "minc_avg": avg}


def _dyadic(b):
    """float32 beta -> (B, e) with beta = B / 2**e exactly."""
    fr = Fraction(float(F32(b)))
    if fr < 0:
        raise ValueError("negative betas are out of scope")
    e = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << e
    return fr.numerator, e


def _sweep_exact(s, t, tgt, non, betas):
    K = len(betas)
    ok = ~np.isnan(s)
    st, sn = np.sort(s[tgt]), np.sort(s[non])
    Nt, Nn = int(st.size), int(sn.size)
    Dt, Dn = max(Nt, 1), max(Nn, 1)
    th = np.unique(s[ok])  # ascending; -0.0 and +0.0 are one value
    ct = np.concatenate([np.searchsorted(st, th, side="left"), [Nt]]).astype(np.int64)  # targets below the threshold
    cn = np.concatenate([Nn - np.searchsorted(sn, th, side="left"), [0]]).astype(np.int64)  # non-targets at or above
    th = np.concatenate([th, [F32(np.inf)]]).astype(F32)
    minc_exact, gap, thr = [], [], np.empty(K, F32)
    for k, b in enumerate(betas):
        B, e = _dyadic(b)
        wt, wn = Dn << e, B * Dt  # cost * (Dt * Dn * 2^e) = ct * wt + cn * wn
        if (int(ct.max()) * wt + int(cn.max()) * wn).bit_length() < 62:
            num = ct * np.int64(wt) + cn * np.int64(wn)
            i = int(np.argmin(num))
            m = int(num[i])
            rest = num[num > m]
            m2 = int(rest.min()) if rest.size else None
        else:
            num = [int(a) * wt + int(c) * wn for a, c in zip(ct, cn)]
            m = min(num)
            i = num.index(m)
            rest = [v for v in num if v > m]
            m2 = min(rest) if rest else None
        tie = bool(np.any((num == m) & ((ct != ct[i]) | (cn != cn[i])))) if isinstance(num, np.ndarray) else any(
            v == m and (int(a), int(c)) != (int(ct[i]), int(cn[i])) for v, a, c in zip(num, ct, cn))
        minc_exact.append(Fraction(m, Dt * Dn << e))
        thr[k] = th[i]
        # relative distance from the minimum to the nearest cost formed from OTHER counts: 0 = a true tie
        gap.append(0.0 if tie else (math.inf if m2 is None else (math.inf if m == 0 else float(Fraction(m2 - m, m)))))
    out = {"minc_exact": minc_exact, "minc": np.asarray([float(m) for m in minc_exact]), "thr": thr,
           "minc_avg_exact": sum(minc_exact) / K, "gap": gap}
    out["minc_avg"] = float(out["minc_avg_exact"])
    eer = math.nan
    if Nt > 0 and Nn > 0:
        d = ct[:-1] * Dn - cn[:-1] * Dt  # (P_miss - P_fa) * Nt * Nn over the score candidates
        hit = np.nonzero(d >= 0)[0]
        i = int(hit[0]) if hit.size else 0
        pm = lambda j: Fraction(int(ct[j]), Nt)  # noqa: E731
        pf = lambda j: Fraction(int(cn[j]), Nn)  # noqa: E731
        if i == 0:
            e_ = (pm(0) + pf(0)) / 2
        else:
            x0, x1 = pm(i - 1) - pf(i - 1), pm(i) - pf(i)
            w = -x0 / (x1 - x0) if x1 != x0 else Fraction(1, 2)
            e_ = pm(i - 1) + w * (pm(i) - pm(i - 1))
        eer = float(e_)
    out["eer"] = eer
    return out


def sweep(s, t, betas, exact):
    """-> dict.  Reference mode: minc[K], thr[K] (float32), minc_avg (float32).  Exact mode: minc[K], minc_avg, eer
    (float64, the exact rationals rounded once), thr[K] (float32), minc_exact / minc_avg_exact (Fractions) and gap[K]."""
    betas = list(betas)
    if not betas:
        raise ValueError("at least one beta")
    s, t, tgt, non = classes(s, t)
    return (_sweep_exact if exact else _sweep_reference)(s, t, tgt, non, betas)


def brute(s, t, betas):
    """The reference-mode definition word for word, O(N^2): for every target score x in ascending order,
    P_miss = (last index of {targets < x} in the ascending target list, or 1.0 when empty) / sum t,
    P_fa = (last index of {non-targets >= x} in the DESCENDING non-target list, or 1.0 when empty) / sum (1 - t);
    the first smallest P_miss + beta * P_fa wins.  -> (minc[K], thr[K], minc_avg), float32."""
    s, t, tgt, non = classes(s, t)
    if s.size > 200:
        raise ValueError("brute is for N <= 200")
    st = sorted(float(v) for v in s[tgt])
    sn = sorted((float(v) for v in s[non]), reverse=True)
    nt, nn = F32(0), F32(0)
    for v in t:  # every partial sum of the labels used here is exact in float32
        nt, nn = F32(nt + v), F32(nn + F32(F32(1) - v))
    K = len(betas)
    minc, thr = np.full(K, np.nan, F32), np.full(K, np.nan, F32)
    with np.errstate(all="ignore"):
        for k, b in enumerate(betas):
            best = None
            for x in st:
                below = [j for j, v in enumerate(st) if v < x]
                above = [j for j, v in enumerate(sn) if v >= x]
                pm = F32(F32(below[-1] if below else 1.0) / nt)
                pf = F32(F32(above[-1] if above else 1.0) / nn)
                c = F32(pm + F32(F32(b) * pf))
                if not np.isnan(c) and (best is None or c < best[0]):
                    best = (c, x)
            if best is not None:
                minc[k], thr[k] = best[0], F32(best[1])
        avg = _average_f32([F32(m) for m in minc])
    return minc, thr, avg


def half_ulp32(x):
    """Half a float32 ulp at the magnitude of x (a Fraction or float), as a Fraction."""
    x = abs(Fraction(x))
    if x == 0:
        return Fraction(1, 1 << 150)
    e = math.frexp(float(x))[1]  # x in [2^(e-1), 2^e)
    return Fraction(2) ** (max(e - 24, -149) - 1)


def within_rounding(got, exact):
    """True when float32 `got` is `exact` (a Fraction or float) evaluated once in float64 and rounded once to float32:
    within half a float32 ulp times (1 + 2^-20)."""
    got = float(got)
    if isinstance(exact, float) and math.isnan(exact):
        return math.isnan(got)
    if math.isnan(got) or math.isinf(got):
        return False
    return abs(Fraction(got) - Fraction(exact)) <= half_ulp32(exact) * (1 + Fraction(1, 1 << 20))
