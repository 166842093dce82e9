"""Dense reference of the all-pairs loss (csrc/nplda_allpairs.hip) in numpy — a plain helper of the all-pairs tests.

    T     = {(i, j): i < j, grp[i] == grp[j]},  target iff spk[i] == spk[j]
    s_ij  = q_i + q_j + 2 sum_d P_d z_id z_jd,  q_i = sum_d Q_d z_id^2,  P = P_sqrt^2
    sums, loss, dtheta, g_ij  from tests/loss_ref.py on the scores of T (fp64 sums of the per-trial terms)
    G     symmetric, G_ij = G_ji = g_ij on T, 0 elsewhere;  r = G 1,  A = G z
    dz    = 2 r (Q o z) + 2 P o A,   dQ = sum_i r_i z_i^2,   dP_sqrt = 2 P_sqrt sum_i z_i o A_i

`dtype=np.float64` is the oracle, `dtype=np.float32` the same formulas with every array in float32 (the unit of
tests/fp32_units.py); every sum over features or rows is a plain left-to-right sum in `dtype` (`_sum_over`);
`reverse=True` evaluates on the rows in reversed order (another summation order of every sum over rows) and returns the
results in the caller's order.

Rounding bound of the sums (`sum_bound`): loss_ref.softcdet_sum_bound / bce_sum_bound on the oracle's scores covers the
per-trial terms given the score; the device's score itself is a float32 computation, and its error enters every term through
|d term / ds| <= alpha / 4 (SoftCdet: sigma' <= 1/4 for the miss / false-alarm terms, |sigma''| < 0.1 for the derivative
terms) or <= 1 (BCE: |p - t| <= 1, p (1 - p) <= 1/4).  Count of the roundings of s_ij = fma(2, X_ij, q_i + q_j):
    P = P_sqrt^2, P o z_i                           one each                                          2
    X_ij: the MFMA chain over the features          one per fma; padded features add exact zeros      D2
    q_i: Q_d z_id (1), a chain of <= 12 fma per lane and four levels of the 16-lane sum               <= 17
    q_i + q_j, and the final fma                    one each, relative to the partial sums themselves
so every product of the three sums passes at most D2 + 2 roundings before the final fma: |ds_ij| <= gamma_{D2 + 2}
(|Q| z_i^2 + |Q| z_j^2 + 2 sum_d |P_d z_id z_jd|), first order in 2^-24 with 0.1 % on top — the dot-product bound of length
D2 + 2 this test is specified with.  (The final fma rounds s_ij itself once more; that rounding is not in the length.)  A count, not a
measurement.
"""
import contextlib
from collections import namedtuple

import numpy as np

from tests import loss_ref as lr
from tests import synth

Result = namedtuple("Result", "S trial target Nt Nn sums loss dtheta G dz dP_sqrt dQ pairs s_pairs t_pairs")

U = 2.0 ** -24
THETA, BETA, ALPHA = lr.THETA, lr.BETA, lr.ALPHA


def masks(spk, grp=None):
    """(trial, target): boolean (N, N), upper triangle only."""
    spk = np.asarray(spk)
    N = spk.shape[0]
    trial = np.triu(np.ones((N, N), dtype=bool), 1)
    if grp is not None:
        grp = np.asarray(grp)
        trial &= grp[:, None] == grp[None, :]
    return trial, trial & (spk[:, None] == spk[None, :])


def allpairs(z, spk, P_sqrt, Q, theta, beta, alpha, kind, grp=None, dtype=np.float64, reverse=False):
    """kind: "softcdet" (theta, beta: K values) or "bce" (theta: one value).  -> Result."""
    z = np.asarray(z, np.float32)
    spk = np.asarray(spk)
    if reverse:
        r = allpairs(z[::-1], spk[::-1], P_sqrt, Q, theta, beta, alpha, kind, None if grp is None else np.asarray(grp)[::-1],
                     dtype)
        return r._replace(dz=r.dz[::-1], S=None, G=None, trial=None, target=None, pairs=None, s_pairs=None, t_pairs=None)
    z = z.astype(dtype)
    ps, Qv = np.asarray(P_sqrt, np.float32).astype(dtype), np.asarray(Q, np.float32).astype(dtype)
    P = ps * ps
    q, X = _sum_over(lambda d: (Qv[d] * z[:, d]) * z[:, d], z.shape[1], dtype), \
        _sum_over(lambda d: (z[:, d] * P[d])[:, None] * z[None, :, d], z.shape[1], dtype)
    S = (q[:, None] + q[None, :]) + dtype(2) * X
    trial, target = masks(spk, grp)
    ii, jj = np.nonzero(trial)
    s_p = S[ii, jj].astype(dtype)
    t_p = target[ii, jj].astype(np.float32)
    if kind == "bce":
        L = _bce(s_p, t_p, theta[0], dtype)
    else:
        L = _softcdet(s_p, t_p, theta, beta, alpha, dtype)
    N = z.shape[0]
    G = np.zeros((N, N), dtype)
    if ii.size:
        G[ii, jj] = L.g
        G[jj, ii] = L.g
    rs = _sum_over(lambda j: G[:, j], N, dtype)
    A = _sum_over(lambda j: G[:, j, None] * z[j][None, :], N, dtype)
    dz = dtype(2) * (rs[:, None] * (Qv * z)) + dtype(2) * (P * A)
    dQ = _sum_over(lambda i: (rs[i] * z[i]) * z[i], N, dtype)
    dP = dtype(2) * ps * _sum_over(lambda i: z[i] * A[i], N, dtype)
    return Result(S, trial, target, float(L.sums[0]), float(L.sums[1]), L.sums, L.loss, L.dtheta, G, dz, dP, dQ,
                  (ii, jj), s_p, t_p)


def _sum_over(term, n, dtype):
    """sum_{k < n} term(k), left to right, every partial sum rounded to `dtype`: THE float32 sum, whatever the machine.  (A
    BLAS product or numpy's pairwise sum would do in float64; in float32 their blocked orders are up to four times more
    accurate than a plain sum at these lengths and differ between shapes and CPUs, which is not a property of the format
    and would make the unit of tests/fp32_units.py depend on where the test runs.)"""
    acc = None
    for k in range(n):
        v = term(k)
        acc = v.astype(dtype) if acc is None else (acc + v).astype(dtype)
    return acc


@contextlib.contextmanager
def _scores_as_given():
    """loss_ref rounds the scores it is given to float32 first (its callers hand it the float32 scores of a kernel).  The
    oracle's float64 scores must not be rounded — that alone is an error of one float32 unit — so its entry conversion is
    replaced for the duration of a call."""
    keep = lr._prep

    def prep(s, t, dtype):
        t = np.asarray(t, np.float32).astype(dtype)
        return np.asarray(s).astype(dtype), t, dtype(1) - t

    lr._prep = prep
    try:
        yield
    finally:
        lr._prep = keep


def _softcdet(s, t, theta, beta, alpha, dtype):
    with _scores_as_given():
        return lr.softcdet(s, t, theta, beta, alpha, dtype)


def _bce(s, t, theta, dtype):
    with _scores_as_given():
        return lr.bce(s, t, theta, dtype)


def score_error_bound(z, P_sqrt, Q, pairs):
    """|ds_ij| of the device's float32 score for the trials `pairs` (see the module docstring)."""
    z = np.asarray(z, np.float32).astype(np.float64)
    ps, Qv = np.asarray(P_sqrt, np.float32).astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
    n = z.shape[1] + 2
    gamma = 1.001 * n * U / (1 - n * U)
    qa = (np.abs(Qv) * z * z).sum(axis=1)
    X = (np.abs(z) * (ps * ps)) @ np.abs(z).T
    ii, jj = pairs
    return gamma * (qa[ii] + qa[jj] + 2 * X[ii, jj])


def sum_bound(ref64, z, P_sqrt, Q, theta, alpha, kind):
    """Per entry of `sums`: the bound of the per-trial terms at the oracle's scores plus the score's own error."""
    ds = score_error_bound(z, P_sqrt, Q, ref64.pairs).sum()
    s32 = ref64.s_pairs  # (loss_ref's bounds evaluate at float64(float32(s)): 2^-24 |s| off, far inside the score term)
    if kind == "bce":
        b = lr.bce_sum_bound(s32, ref64.t_pairs, theta[0])
        b[2:] += ds
    else:
        b = lr.softcdet_sum_bound(s32, ref64.t_pairs, theta, alpha)
        b[2:] += float(np.float32(alpha)) / 4 * ds
    return b


# ---- the inputs the CPU and GPU tests share ---------------------------------------------------------------------------------

TILE = 64  # the kernel's row tile (ops.ALLPAIRS_TILE; the GPU test asserts they agree)

# (N, D2, kind, K, label mode): N in {2, 3, T - 1, T, T + 1, 2 T + 17, 3 T + 17 (four row tiles and seven column tiles, both ragged)}
CASES = [
    (2, 150, "bce", 1, "mixed"), (2, 150, "softcdet", 2, "mixed"),
    (3, 150, "softcdet", 1, "mixed"), (3, 170, "bce", 1, "mixed"),
    (TILE - 1, 150, "softcdet", 2, "mixed"), (TILE, 160, "softcdet", 4, "mixed"), (TILE + 1, 170, "softcdet", 1, "mixed"),
    (TILE + 1, 150, "bce", 1, "mixed"),
    (2 * TILE + 17, 150, "softcdet", 4, "groups"), (2 * TILE + 17, 170, "softcdet", 2, "mixed"),
    (2 * TILE + 17, 160, "bce", 1, "groups"),
    (3 * TILE + 17, 150, "softcdet", 2, "mixed"), (3 * TILE + 17, 160, "softcdet", 1, "one"),
    (3 * TILE + 17, 170, "softcdet", 4, "groups"), (3 * TILE + 17, 150, "bce", 1, "one"),
]


def labels(N, mode, seed=0):
    """(spk, grp or None) for N rows.
    "mixed":  speakers of 1 - 9 utterances in row order (singletons present); one speaker holds rows TILE - 2 .. TILE + 1
    "groups": the same speakers, two groups of unequal size (about 1/3 and 2/3 of the speakers)
    "one":    every row one speaker but the last
    """
    rng = np.random.default_rng(100 + seed)
    if mode == "one":
        spk = np.zeros(N, np.int64)
        if N > 1:
            spk[-1] = 1
        return spk, None
    sizes = []
    while sum(sizes) < N:
        sizes.append(int(rng.integers(1, 10)) if len(sizes) % 5 else 1)
    spk = np.repeat(np.arange(len(sizes)), sizes)[:N]
    if N >= 4:
        spk[:2] = 0
        spk[2] = 1  # a target and a non-target at any size
    if N > TILE + 1:
        spk[TILE - 2:TILE + 2] = spk[TILE - 2]  # straddles the first tile edge
    grp = None
    if mode == "groups":
        grp = np.where(spk % 3 == 0, 7, -2).astype(np.int64)  # arbitrary label values, unequal sizes
    return spk.astype(np.int64), grp


def embeddings(N, D2, seed=0, span=55.0, K=4, alpha=ALPHA):
    """(z (N, D2) float32, P_sqrt, Q) from tests/synth.py: speaker-structured 512-d x-vectors through a random
    512 -> D1 -> D2 model (float64), scaled so that alpha |theta_k - s_ij| < span for every pair and k < K."""
    rng = np.random.default_rng(seed)
    D0, D1 = 512, D2
    W1 = rng.standard_normal((D1, D0)) / np.sqrt(D0)
    b1 = 0.1 * rng.standard_normal(D1)
    T = np.linalg.qr(rng.standard_normal((D1, D1)))[0]
    psi = 4.0 / (1 + np.arange(D1))
    x, _ = synth.speaker_structured_xvectors(W1, b1, T, np.zeros(D1), psi, (N + 8) // 9 + 1, 9, seed=seed + 7)
    x = x[:N].astype(np.float64)
    u = x @ W1.T + b1
    y = u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-12)
    W2 = rng.standard_normal((D2, D1)) / np.sqrt(D1)
    z = y @ W2.T + 0.05 * rng.standard_normal(D2)
    ps = rng.uniform(0.3, 1.0, D2).astype(np.float32)
    Q = (-rng.uniform(0.1, 0.6, D2)).astype(np.float32)
    P = ps.astype(np.float64) ** 2
    q = (Q * z * z).sum(axis=1)
    S = q[:, None] + q[None, :] + 2 * (z * P) @ z.T
    np.fill_diagonal(S, 0.0)
    th = np.abs(np.array(THETA[:K])).max()
    c2 = (0.9 * span / alpha - th) / max(np.abs(S).max(), 1e-30)
    return (z * np.sqrt(c2)).astype(np.float32), ps, Q


_cases = {}


def case(N, D2, kind, K, mode="mixed", seed=0):
    """Everything a test needs for one shape, computed once: inputs, the float64 and float32 references, the sum bound."""
    key = (N, D2, kind, K, mode, seed)
    if key not in _cases:
        z, ps, Q = embeddings(N, D2, seed=seed)
        spk, grp = labels(N, mode, seed)
        theta, beta = (THETA[:1], []) if kind == "bce" else (THETA[:K], BETA[:K])
        r64 = allpairs(z, spk, ps, Q, theta, beta, ALPHA, kind, grp, np.float64)
        r32 = allpairs(z, spk, ps, Q, theta, beta, ALPHA, kind, grp, np.float32)
        bound = sum_bound(r64, z, ps, Q, theta, ALPHA, kind)
        for a in (z, ps, Q, spk):
            a.setflags(write=False)
        _cases[key] = dict(z=z, P_sqrt=ps, Q=Q, spk=spk, grp=grp, theta=theta, beta=beta, alpha=ALPHA, kind=kind, K=len(theta),
                           r64=r64, r32=r32, bound=bound)
    return _cases[key]


def span_of(c):
    """max over trials and k of alpha |theta_k - s_ij| on the float64 reference."""
    s = c["r64"].s_pairs
    if s.size == 0:
        return 0.0
    th = np.array([float(np.float32(x)) for x in c["theta"]])
    return float(np.abs(float(np.float32(c["alpha"])) * (th[:, None] - s[None, :])).max())
