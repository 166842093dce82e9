"""Numpy oracle and case generators of the top-k search (csrc/nplda_topk.hip; a plain helper of tests/test_topk_*.py).

The score is s_rj = q_r + q_j + 2 sum_d P_d z_rd z_jd with P = P_sqrt^2; z, q (float32) are the kernel's INPUTS, as embed()
hands them over.  ref64 evaluates it in float64 from those float32 inputs, ref32 in float32 by plain left-to-right sums (the
unit of tests/fp32_units.py).  Eligibility is applied, then a stable sort gives the order: ties by ascending column.

Exact cases: every product and sum is exact in float32 in any order (all terms are multiples of 2^-8 and every partial
sum stays below 2^14), so the kernel must match numpy bit for bit, ties included.  The table of such a case is a base set
laid down three times at distant positions, one copy permuted, labels and groups with it: every score occurs at least three
times per row, and the ties straddle rank k and the chunk boundaries."""
import functools

import numpy as np

TILE = 64            # rows one block of topk_main owns
U = 2.0 ** -24


def padded_dim(D2):
    nb = (D2 + 15) // 16
    for n in (2, 4, 8, 10, 11, 12):
        if nb <= n:
            return 16 * n
    raise ValueError(D2)


def qvec(z, Q, dtype, order=None):
    """q_i = sum_d Q_d z_id^2 in `dtype`, left to right over `order`."""
    z, Q = z.astype(dtype), Q.astype(dtype)
    q = np.zeros(z.shape[0], dtype)
    for d in (range(Q.size) if order is None else order):
        q = q + (Q[d] * z[:, d]) * z[:, d]
    return q


def scores(zr, qr, zt, qt, P_sqrt, dtype, order=None):
    """S (R, M) in `dtype` from float32 inputs: left-to-right sum of P_d z_rd z_jd over `order`, then q_r + q_j + 2 sum."""
    D2 = P_sqrt.size
    P = (P_sqrt.astype(np.float32) * P_sqrt.astype(np.float32)).astype(dtype)  # the image holds fp32 P_sqrt^2
    zr, zt = zr[:, :D2].astype(dtype), zt[:, :D2].astype(dtype)
    acc = np.zeros((zr.shape[0], zt.shape[0]), dtype)
    for d in (range(D2) if order is None else order):
        acc = acc + (P[d] * zr[:, d])[:, None] * zt[:, d][None, :]
    return (qr.astype(dtype)[:, None] + qt.astype(dtype)[None, :]) + dtype(2) * acc


def magnitude(zr, qr, zt, qt, P_sqrt):
    """A_rj = |q_r| + |q_j| + 2 sum_d P_d |z_rd z_jd| (float64): what a rounding bound of the score scales with."""
    D2 = P_sqrt.size
    P = (P_sqrt.astype(np.float32) ** 2).astype(np.float64)
    return (np.abs(qr.astype(np.float64))[:, None] + np.abs(qt.astype(np.float64))[None, :]
            + 2.0 * (np.abs(zr[:, :D2].astype(np.float64)) * P) @ np.abs(zt[:, :D2].astype(np.float64)).T)


def tolerance(D2, A):
    """(D2 + 8) 2^-24 A: the a-priori bound of a float32 sum of D2 products and the few terms around it, in any order."""
    return (D2 + 8) * U * A


def eligible(R, M, mask=None, lab_r=None, lab_t=None, grp_r=None, grp_t=None, self_rows=None):
    e = np.ones((R, M), bool)
    if grp_r is not None:
        e &= np.asarray(grp_r)[:, None] == np.asarray(grp_t)[None, :]
    if self_rows is not None:
        e &= np.asarray(self_rows)[:, None] != np.arange(M)[None, :]
    if mask == "different":
        e &= np.asarray(lab_r)[:, None] != np.asarray(lab_t)[None, :]
    elif mask == "same":
        e &= np.asarray(lab_r)[:, None] == np.asarray(lab_t)[None, :]
    else:
        assert mask is None
    return e


def topk(S, elig, k, largest):
    """(vals (R, k) of S's dtype, idx (R, k) int64): stable sort of every row's eligible scores, short rows padded."""
    R, M = S.shape
    S = S + S.dtype.type(0)                        # -0.0 counts as +0.0
    key = np.where(elig, -S if largest else S, np.inf).astype(np.float64)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    if M < k:
        order = np.concatenate([order, np.zeros((R, k - M), np.int64)], axis=1)
    have = np.arange(k)[None, :] < elig.sum(1)[:, None]
    fill = S.dtype.type(-np.inf if largest else np.inf)
    if M == 0:
        return np.full((R, k), fill, S.dtype), np.full((R, k), -1, np.int64)
    vals = np.where(have, np.take_along_axis(S, order, 1), fill).astype(S.dtype)
    return vals, np.where(have, order, -1).astype(np.int64)


def tie_across_rank_k(S, elig, k, largest):
    """Does some row's k-th best eligible score equal its (k + 1)-th?"""
    v, _ = topk(S, elig, min(k + 1, max(S.shape[1], 1)), largest)
    return bool(v.shape[1] > k and np.any((v[:, k - 1] == v[:, k]) & np.isfinite(v[:, k])))


def selection_violations(vals, idx, S64, elig, tol, largest):
    """For every row, every eligible column NOT returned must score no better than the last returned value, to within
    tol[r, j].  Returns (number of violations, worst (S64 - vals_last) / tol with the sign turned so that > 1 violates)."""
    R, k = idx.shape
    bad, worst = 0, -np.inf
    for r in range(R):
        got = idx[r][idx[r] >= 0]
        rest = elig[r].copy()
        rest[got] = False
        if not rest.any():
            continue
        assert got.size == k, "a row with eligible columns left over returned fewer than k"
        d = S64[r, rest] - float(vals[r, k - 1])
        ratio = (d if largest else -d) / tol[r, rest]
        bad += int((ratio > 1.0).sum())
        worst = max(worst, float(ratio.max()))
    return bad, worst


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def exact_params(D2, rng):
    return rng.choice([0.5, 1.0, 1.5, 2.0], D2).astype(np.float32), (-0.25 * rng.integers(0, 9, D2)).astype(np.float32)


def exact_rows(n, D2, rng):
    """z (n, ldz): multiples of 1/8 in [-2, 2], zero pad columns."""
    z = np.zeros((n, padded_dim(D2)), np.float32)
    z[:, :D2] = rng.integers(-16, 17, (n, D2)) / 8.0
    return z


def tripled(base_n, M, rng):
    """Source row of each of M table rows: the base set three times, the middle copy permuted, cut to M."""
    src = np.concatenate([np.arange(base_n), rng.permutation(base_n), np.arange(base_n)])
    assert src.size >= M
    return src[:M]


def labels_for(n, n_lab, rng):
    return rng.integers(0, n_lab, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def exact_case(D2, k, R, M, mask, groups, seed=0):
    """Inputs and oracle of one exact case; `mask` None / "different" / "same" ("same" searches the table against its own
    rows: self_rows is given).  The oracle holds both directions."""
    rng = np.random.default_rng([seed, D2, k, R, M, {None: 0, "different": 1, "same": 2}[mask], int(groups)])
    P_sqrt, Q = exact_params(D2, rng)
    base_n = max(1, -(-M // 3))
    src = tripled(base_n, M, rng)
    zt = exact_rows(base_n, D2, rng)[src]
    lab_base, grp_base = labels_for(base_n, max(2, base_n // 40), rng), labels_for(base_n, 2, rng)
    lab_t, grp_t = lab_base[src], grp_base[src]
    self_rows = None
    if mask == "same":
        self_rows = np.sort(rng.choice(M, R, replace=R > M)).astype(np.int64)
        zr, lab_r, grp_r = zt[self_rows].copy(), lab_t[self_rows], grp_t[self_rows]
    else:
        zr, lab_r, grp_r = exact_rows(R, D2, rng), labels_for(R, max(2, base_n // 40), rng), labels_for(R, 2, rng)
    qr, qt = qvec(zr, Q, np.float32), qvec(zt, Q, np.float32)
    c = dict(D2=D2, k=k, R=R, M=M, mask=mask, P_sqrt=P_sqrt, Q=Q, zr=zr, zt=zt, qr=qr, qt=qt, self_rows=self_rows,
             lab_r=lab_r if mask else None, lab_t=lab_t if mask else None,
             grp_r=grp_r if groups else None, grp_t=grp_t if groups else None)
    c["S"] = scores(zr, qr, zt, qt, P_sqrt, np.float32)
    c["elig"] = eligible(R, M, mask, c["lab_r"], c["lab_t"], c["grp_r"], c["grp_t"], self_rows)
    c["ref"] = {lg: topk(c["S"], c["elig"], k, lg) for lg in (True, False)}
    if (c["elig"].sum(1) > k).any():   # (a case with no more than k eligible columns anywhere has no rank-k boundary)
        # a self-search row's own two copies score highest and stand alone in front of the triples: with k = 2 (mod 3), as
        # 5, 32 and 128 are, rank k of the LARGEST then falls between two triples; the smallest (what mining asks for) tie
        dirs = (False,) if mask == "same" and k % 3 == 2 else (True, False)
        assert all(tie_across_rank_k(c["S"], c["elig"], k, lg) for lg in dirs), (D2, k, R, M)
    return c


# (D2, k, R, M, mask, groups): every value of every axis at least once, and the corners (R = 1, M = 3000, k = 128) and
# (R = tile + 1, M = k - 1)
EXACT_CASES = [
    (32, 1, 1, 1, None, False),
    (150, 5, 17, 4, None, False),
    (170, 5, TILE + 1, 5, "different", False),
    (150, 32, 17, 63, None, True),
    (170, 32, 1, 64, "same", False),
    (32, 5, TILE + 1, 65, "different", True),
    (32, 128, 17, 128, None, False),
    (150, 128, 1, 3000, None, False),
    (170, 128, TILE + 1, 127, "same", True),
    (150, 32, 17, 3000, "same", True),
    (170, 1, TILE + 1, 3000, "different", False),
    (150, 1, 17, 3000, "same", False),   # k = 1: the self-search ties across rank k in BOTH directions (the row's own two copies)
]


@functools.lru_cache(maxsize=None)
def float_case(D2, k, seed=1, R=TILE + 1, M=3000):
    """Seeded normal z (scale 0.1, as embeddings of unit-normalised inputs are), P_sqrt, Q ~ U; mask "different" with groups."""
    rng = np.random.default_rng([seed, D2, k])
    P_sqrt, Q = rng.uniform(0.2, 1.5, D2).astype(np.float32), (-rng.uniform(0.0, 1.0, D2)).astype(np.float32)
    ld = padded_dim(D2)
    zr, zt = np.zeros((R, ld), np.float32), np.zeros((M, ld), np.float32)
    zr[:, :D2] = 0.1 * rng.standard_normal((R, D2))
    zt[:, :D2] = 0.1 * rng.standard_normal((M, D2))
    qr, qt = qvec(zr, Q, np.float32), qvec(zt, Q, np.float32)
    lab_r, lab_t = labels_for(R, 40, rng), labels_for(M, 40, rng)
    grp_r, grp_t = labels_for(R, 2, rng), labels_for(M, 2, rng)
    c = dict(D2=D2, k=k, R=R, M=M, mask="different", P_sqrt=P_sqrt, Q=Q, zr=zr, zt=zt, qr=qr, qt=qt, self_rows=None,
             lab_r=lab_r, lab_t=lab_t, grp_r=grp_r, grp_t=grp_t)
    c["S64"] = scores(zr, qr, zt, qt, P_sqrt, np.float64)
    c["S32"] = scores(zr, qr, zt, qt, P_sqrt, np.float32)
    c["tol"] = tolerance(D2, magnitude(zr, qr, zt, qt, P_sqrt))
    c["elig"] = eligible(R, M, "different", lab_r, lab_t, grp_r, grp_t)
    return c


FLOAT_CASES = [(150, 10), (150, 128), (170, 10), (170, 128)]


def check_float_result(vals, idx, c, largest, what):
    """The float-case checks of a (vals, idx) result against case c; returns the worst selection ratio."""
    from tests import fp32_units as fu
    R, M, k = c["R"], c["M"], idx.shape[1]
    assert vals.shape == idx.shape == (R, k)
    rows = np.arange(R)[:, None]
    have = idx >= 0
    assert (have.sum(1) == np.minimum(c["elig"].sum(1), k)).all(), what
    assert (idx[have] < M).all() and c["elig"][np.broadcast_to(rows, idx.shape)[have], idx[have]].all(), what
    for r in range(R):
        assert np.unique(idx[r][have[r]]).size == have[r].sum(), (what, r)
    safe = np.where(have, idx, 0)
    r = fu.assert_fp32_level(vals[have], c["S64"][rows, safe][have], c["S32"][rows, safe][have], what)
    print(f"{what}: values at {r['all'][0]:.2f} rms / {r['all'][1]:.2f} max float32 units")
    a, b = vals[:, :-1], vals[:, 1:]
    both = have[:, 1:]
    assert ((a >= b) if largest else (a <= b))[both].all(), what
    assert (idx[:, :-1] < idx[:, 1:])[both & (a == b)].all(), what
    bad, worst = selection_violations(vals, idx, c["S64"], c["elig"], c["tol"], largest)
    print(f"{what}: selection violations {bad}, worst (S64 - vals[k-1]) / tol = {worst:.4f}")
    assert bad == 0, (what, bad, worst)
    return worst


# ---- hard-trial mining ---------------------------------------------------------------------------------------------------------

def mined_pairs(S, spk, grp, rows, n_neg, n_pos):
    """The oracle's trial list for the table rows `rows` (table-row numbering): per row the n_neg highest-scoring rows of other
    speakers and the n_pos lowest-scoring of the same speaker (itself excluded), inside its group; unordered pairs, canonical,
    deduplicated, sorted by (rows1, rows2)."""
    pairs = set()
    sub_spk, sub_grp = spk[rows], None if grp is None else grp[rows]
    me = np.arange(rows.size)
    for mask, k, lg, tgt in (("different", n_neg, True, 0.0), ("same", n_pos, False, 1.0)):
        if k == 0:
            continue
        e = eligible(rows.size, rows.size, mask, sub_spk, sub_spk, sub_grp, sub_grp, me)
        _, idx = topk(S, e, k, lg)
        for r in range(rows.size):
            for j in idx[r][idx[r] >= 0]:
                a, b = int(rows[r]), int(rows[j])
                pairs.add((min(a, b), max(a, b), tgt))
    out = sorted(pairs)
    return (np.array([p[0] for p in out], np.int64), np.array([p[1] for p in out], np.int64),
            np.array([p[2] for p in out], np.float32))
