"""SoftCdet, hard Cdet and BCE in the numerically stable form (numpy only; a plain helper of the loss tests, not a conftest).

`dtype=np.float64` is the reference, `dtype=np.float32` the unit of tests/fp32_units.py: the same formulas with every
per-pair operation rounded to float32.  In both precisions the counts N_t, N_n are exact, the per-pair terms are summed in
float64 (as the kernels do), and theta, beta, alpha are the float32 values the C ABI receives.

SoftCdet, per threshold k:  v = alpha (theta_k - s),  e = exp(-|v|),  1/(1+e) = sigma(|v|),  e/(1+e) = sigma(-|v|),
sigma'(v) = e / (1+e)^2.  No `1 - sigma`: oracle.nplda_oracle.softcdet_grad forms sigma' as sg (1 - sg), which in float64
is wrong by ~2e-3 relative for 10 <= |v| < 30 (1 - sg keeps only the leading bits of e) and by 100 % beyond |v| ~ 37
(1 - sg == 0) — the cancellation the header of csrc/nplda_loss.hip says the kernel avoids.  The oracle is left as it is
(its callers compare to 1e-4 of max|g|); per-element comparisons use this file.

BCE, x = s - theta:  log sigma(x) = min(x, 0) - log1p(exp(-|x|)),  log(1 - sigma(x)) = min(-x, 0) - log1p(exp(-|x|)), each
clamped at -100 as torch.nn.functional.binary_cross_entropy does.  `bce(..., form="naive")` restates what torch (and the
kernel) evaluate instead, p = 1 / (1 + exp(-x)) then log(p), log(1 - p): in float32 p rounds to 1 for x >= ~17, so a
non-target there costs the clamp, 100, and not x.  The two forms agree to rounding only for |x| <= 8 or so.

Layout of `sums` (nplda_loss_nsums):  [N_t, N_n, {S_miss_k, S_fa_k, D_t_k, D_n_k} for k < K]   (SoftCdet, hard Cdet)
                                      [N_t, N_n, sum of BCE terms, sum (p - t)]                (BCE)
`terms` has one row per entry of `sums` (rows 0, 1 are t and 1 - t), so that sums == terms.sum(axis=1).
"""
from collections import namedtuple

import numpy as np

Loss = namedtuple("Loss", "terms sums loss dtheta g")

LOG2E_F32 = np.float32(1.4426950408889634)


def expf_intrinsic_model(x):
    """A model of the device's fast exponential: exp2 of the float32-rounded product x * log2(e), rounded to float32."""
    y = (np.asarray(x, np.float32) * LOG2E_F32).astype(np.float32)
    with np.errstate(under="ignore"):
        return np.exp2(y.astype(np.float64)).astype(np.float32)


def _abi(x, dtype):
    return dtype(np.float32(x))


def _prep(s, t, dtype):
    s = np.asarray(s, np.float32).astype(dtype)
    t = np.asarray(t, np.float32).astype(dtype)
    return s, t, dtype(1) - t


def _wide(a):
    """float64, or long double where that is what came in (the CPU test's check of the float64 reference)."""
    a = np.asarray(a)
    return a if a.dtype == np.longdouble else a.astype(np.float64)


def softcdet_scalars(sums, beta, alpha, K):
    """loss and dL/dtheta from the sums, in float64 (the formulas of csrc/nplda_loss_math.h)."""
    sums = _wide(sums)
    a = float(np.float32(alpha))
    nt, nn = sums[0], sums[1]
    L, dth = sums.dtype.type(0), np.zeros(K, sums.dtype)
    for k in range(K):
        b = float(np.float32(beta[k]))
        sm, sf, dt, dn = sums[2 + 4 * k:6 + 4 * k]
        L += sm / nt + b * sf / nn
        dth[k] = (a * dt / nt - b * a * dn / nn) / K
    return L / K, dth


def bce_scalars(sums):
    sums = _wide(sums)
    n = sums[0] + sums[1]
    return sums[2] / n, np.array([-sums[3] / n])


def softcdet(s, t, theta, beta, alpha, dtype=np.float64, hard=False, exp=None):
    """SoftCdet (hard=True: the hard detection cost, strict inequalities, no gradient) -> Loss.
    `exp`: a replacement for np.exp (expf_intrinsic_model) when emulating the kernel."""
    s, t, n = _prep(s, t, dtype)
    K = len(theta)
    a = _abi(alpha, dtype)
    one = dtype(1)
    t64 = _wide(t)
    nt, nn = t64.sum(), (1.0 - t64).sum()
    terms = np.zeros((2 + 4 * K, s.shape[0]), dtype)
    terms[0], terms[1] = t, n
    g = np.zeros_like(s)
    ct = dtype(-float(np.float32(alpha)) / (nt * K)) if nt > 0 else dtype(0)
    with np.errstate(under="ignore", over="ignore"):
        for k in range(K):
            th = _abi(theta[k], dtype)
            if hard:
                terms[2 + 4 * k] = (s < th).astype(dtype) * t
                terms[3 + 4 * k] = (s > th).astype(dtype) * n
                continue
            v = a * (th - s)
            e = (exp or np.exp)(-np.abs(v)).astype(dtype)
            inv = one / (one + e)
            pos, neg = inv, e * inv
            d = (e * inv) * inv
            terms[2 + 4 * k] = np.where(v >= 0, pos, neg) * t
            terms[3 + 4 * k] = np.where(v >= 0, neg, pos) * n
            terms[4 + 4 * k] = d * t
            terms[5 + 4 * k] = d * n
            cn = dtype(float(np.float32(beta[k])) * float(np.float32(alpha)) / (nn * K)) if nn > 0 else dtype(0)
            g = g + d * (ct * t + cn * n)
    sums = _wide(terms).sum(axis=1)
    sums[0], sums[1] = nt, nn
    with np.errstate(divide="ignore", invalid="ignore"):
        L, dth = softcdet_scalars(sums, beta, alpha, K)
    return Loss(terms, sums, dtype(L), dth.astype(dtype), None if hard else g)


def bce(s, t, theta, dtype=np.float64, form="stable", clamp=True):
    """F.binary_cross_entropy(sigmoid(s - theta), t), mean reduction -> Loss (terms rows: t, 1 - t, BCE term, p - t)."""
    s, t, n = _prep(s, t, dtype)
    one = dtype(1)
    x = s - _abi(theta, dtype)
    with np.errstate(under="ignore", over="ignore", divide="ignore"):
        if form == "stable":
            e = np.exp(-np.abs(x))
            l1 = np.log1p(e)
            lp, lq = np.minimum(x, 0) - l1, np.minimum(-x, 0) - l1
            inv = one / (one + e)
            p = np.where(x >= 0, inv, e * inv)
        else:
            p = one / (one + np.exp(-x))
            lp, lq = np.log(p), np.log(one - p)
        if clamp:
            lp, lq = np.maximum(lp, dtype(-100)), np.maximum(lq, dtype(-100))
    t64 = _wide(t)
    nt, nn = t64.sum(), (1.0 - t64).sum()
    terms = np.stack([t, n, -(t * lp + n * lq), p - t]).astype(dtype)
    sums = _wide(terms).sum(axis=1)
    sums[0], sums[1] = nt, nn
    L, dth = bce_scalars(sums)
    g = (p - t) * dtype(1.0 / (nt + nn))
    return Loss(terms, sums, dtype(L), dth.astype(dtype), g)


# ---- worst-case bound of the device's fp64 sums of fp32 terms ----------------------------------------------------------
U = 2.0 ** -24  # unit roundoff of float32


def softcdet_sum_bound(s, t, theta, alpha):
    """Per entry of `sums`: 2^-24 sum_i c_i |term_i| (+ an absolute 2^-120 per pair for the denormal range), where c_i
    counts the float32 roundings of softcdet_accumulate, first order in 2^-24 with 0.1 % on top:
      v = alpha * (theta - s)    two roundings: |dv| <= 2 u |v|
      e = __expf(-|v|)           exp2 of the rounded product |v| log2(e) (u |v|, and float32(log2 e) is 0.22 u off: 0.25 u |v|),
                                 the hardware exp2 to one ulp (2 u); with dv:       eps_e = (2 + 3.5 |v|) u
      inv = 1 / (1 + e)          the sum and the quotient round (2 u); eps_e enters scaled by e / (1 + e) = sigma(-|v|):
                                                                                     c_pos = 2 + eps_e sigma(-|v|)
      sigma(-|v|) = e * inv      one more product:                                   c_neg = 1 + eps_e + c_pos
      sigma'(v) = (e * inv) * inv                                                    c_d   = 2 + eps_e + 2 c_pos
    The products with t and 1 - t (0 or 1) and the conversions to double are exact; the fp64 accumulation adds at most
    B 2^-53 relative (< 1e-10 at the sizes tested), covered by the 0.1 %."""
    s = np.asarray(s, np.float32).astype(np.float64)
    r = softcdet(s, t, theta, [1.0] * len(theta), alpha, np.float64)
    bound = np.zeros(r.sums.shape)
    for k in range(len(theta)):
        c_pos, c_neg, c_d = _softcdet_counts(s, theta[k], alpha)
        v_pos = float(np.float32(theta[k])) - s >= 0
        c = [np.where(v_pos, c_pos, c_neg), np.where(v_pos, c_neg, c_pos), c_d, c_d]
        for j in range(4):
            bound[2 + 4 * k + j] = U * 1.001 * np.sum(c[j] * np.abs(r.terms[2 + 4 * k + j])) + s.size * 2.0 ** -120
    return bound


def _softcdet_counts(s64, theta_k, alpha):
    av = np.abs(float(np.float32(alpha)) * (float(np.float32(theta_k)) - s64))
    eps = 2 + 3.5 * av
    with np.errstate(under="ignore", over="ignore"):
        sneg = np.exp(-av) / (1 + np.exp(-av))
    c_pos = 2 + eps * sneg
    return c_pos, 1 + eps + c_pos, 2 + eps + 2 * c_pos


def softcdet_g_bound(s, t, theta, beta, alpha):
    """Per element: |g_i - g_i(float64)| <= 2^-24 sum_k (c_d + 4) |contribution_k| (+ 2^-120 times the coefficients for the
    denormal range): sigma' as above; the coefficients ct, cn_k are rounded to float32 once each, fma(ct, t, cn n) rounds
    once (one of its two terms is zero), and the accumulating fma once per k."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    t64 = np.asarray(t, np.float64)
    r = softcdet(s, t, theta, beta, alpha, np.float64)
    K = len(theta)
    a = float(np.float32(alpha))
    nt, nn = r.sums[0], r.sums[1]
    bound = np.zeros(s64.shape)
    for k in range(K):
        coef = np.where(t64 > 0.5, a / (nt * K), float(np.float32(beta[k])) * a / (nn * K))
        d = r.terms[4 + 4 * k] + r.terms[5 + 4 * k]
        bound += U * 1.001 * (_softcdet_counts(s64, theta[k], alpha)[2] + 4) * d * coef + 2.0 ** -120 * coef
    return bound


def bce_sum_bound(s, t, theta):
    """Per entry of the BCE `sums`, for |x| = |s - theta| <= 8 (beyond, float32 p saturates: see the module docstring):
      x = s - theta              one rounding: u |x|
      E = expf(-x)               one ulp (2 u) and the rounding of x:                    eps_E = (2 + |x|) u
      p = 1 / (1 + E)            the sum and the quotient round; eps_E scaled by E / (1 + E) <= 1:   c_p = 4 + |x|
      log(p)                     absolute error c_p u (p's relative error), logf itself to one ulp: 2 u |term|, 3 u taken
      log(1 - p)                 1 - p is exact for p >= 1/2 and rounds once below; p's error c_p u p is relative to 1 - p
                                 c_p u p / (1 - p) = c_p u e^x: absolute (c_p + 1) u (1 + e^max(x, 0))
      p - t                      c_p u p + u |p - t|
    The products with t, 1 - t and the sum of the two halves (one of them is zero) are exact."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    t64 = np.asarray(t, np.float64)
    r = bce(s, t, theta, np.float64)
    x = s64 - float(np.float32(theta))
    c_p = 4 + np.abs(x)
    p = 1.0 / (1.0 + np.exp(-x))
    absolute = np.where(t64 > 0.5, c_p + 1, (c_p + 1) * (1 + np.exp(np.maximum(x, 0))))
    bound = np.zeros(4)
    bound[2] = U * 1.001 * np.sum(absolute + 3 * np.abs(r.terms[2]))
    bound[3] = U * 1.001 * np.sum(c_p * p + np.abs(r.terms[3]))
    return bound


# ---- the inputs of tests/test_loss_fp32_gpu.py (here so that the CPU test can hold the float32 unit to the same bound) ---
THETA = [-0.8, -0.6, -1.1, 0.3]   # distinct, so that a swapped k shows
BETA = [99.0, 199.0, 9.9, 19.9]
ALPHA = 15.0
BANDS = ((0, 2), (2, 10), (10, 30), (30, 60), (60, 80))  # of min_k |alpha (theta_k - s)|
BATCHES = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 262144, 262145, 600001)


def vmin(s, K):
    s64 = np.asarray(s, np.float32).astype(np.float64)
    th = np.array([float(np.float32(x)) for x in THETA[:K]])
    return np.abs(float(np.float32(ALPHA)) * (th[:, None] - s64[None, :])).min(axis=0)


def make_scores(B, K, seed=0, bce=False):
    """(s, t) float32: scores N(-1, 2.5), targets ~15 % with both classes present (B >= 2).  From B = 64 on, 8 % of the
    scores are moved into each band of BANDS (outside the outermost threshold, so that min_k |v_k| is the band's), 2 % beyond
    |v| = 80, and the extremes +-50, +-1e4 and three scores exactly equal to each theta_k are added, in both classes.
    bce=True: the scores are folded into |s - theta_0| <= 7.99 instead (where float32 p does not saturate)."""
    rng = np.random.default_rng(1000 * K + B % 99991 + seed)
    s = (rng.standard_normal(B) * 2.5 - 1).astype(np.float32)
    t = (rng.random(B) < 0.15).astype(np.float32)
    th = np.array(THETA[:K], np.float32)
    if bce:
        far = np.abs(s - th[0]) > 7.99
        s[far] = th[0] + rng.uniform(-7.99, 7.99, int(far.sum())).astype(np.float32)
    elif B >= 64:
        idx = rng.permutation(B)
        n, o = max(B * 8 // 100, 1), 0
        for lo, hi in BANDS + ((80, 120),):
            m = n if lo < 80 else max(n // 4, 1)
            sel = idx[o:o + m]
            o += m
            av = rng.uniform(lo + 0.01 * (hi - lo), hi - 0.01 * (hi - lo), m) / ALPHA
            up = rng.random(m) < 0.5
            s[sel] = np.where(up, th.max() + av, th.min() - av).astype(np.float32)
        ext = idx[o:o + 8 + 6 * K]
        s[ext[:8]] = [50, -50, 1e4, -1e4, 50, -50, 1e4, -1e4]
        t[ext[:8]] = [1, 1, 1, 1, 0, 0, 0, 0]
        for k in range(K):
            s[ext[8 + 6 * k:14 + 6 * k]] = th[k]
            t[ext[8 + 6 * k:14 + 6 * k]] = [1, 0, 1, 0, 1, 0]
    if B >= 2:
        i, j = (0, 1) if bce or B < 64 else (idx[-1], idx[-2])
        t[i], t[j] = 1, 0
    return s, t
