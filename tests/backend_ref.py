"""float64 numpy restatement of the back-end estimators (neuralplda_amd/backend.py): the class statistics, Kaldi's
ivector-compute-lda and ivector-compute-plda with unit weights — literal, with per-class loops, no grouping and no shared
code with the library.  `dtype=np.float32` accumulates the ROW statistics (sum, scatter, class sums: one row at a time, in
order) in float32 and leaves everything after them in float64: the `ref32` of tests/fp32_units.ratios."""
import numpy as np


def class_stats(x, offs, rows=None, pivot=None, dtype=np.float64):
    """(sum (n,), scatter (n, n), class_sum (S, n)) of x[rows] - pivot as float64 arrays, accumulated in `dtype`."""
    x = np.asarray(x)
    offs = np.asarray(offs, dtype=np.int64)
    S, N = len(offs) - 1, int(offs[-1])
    xs = x[:N] if rows is None else x[np.asarray(rows, dtype=np.int64)]
    xs = xs.astype(dtype)
    if pivot is not None:
        xs = xs - np.asarray(pivot).astype(dtype)  # the subtraction in the accumulation type, as the kernel does it
    n = xs.shape[1]
    cs = np.zeros((S, n), dtype=dtype)
    if dtype == np.float64:
        sc = xs.T @ xs
        for s in range(S):
            cs[s] = xs[offs[s]:offs[s + 1]].sum(0)
        sm = xs.sum(0)
    else:
        sc = np.zeros((n, n), dtype=dtype)
        sm = np.zeros(n, dtype=dtype)
        for s in range(S):
            for k in range(offs[s], offs[s + 1]):
                cs[s] += xs[k]
        for k in range(N):
            sm += xs[k]
            sc += np.outer(xs[k], xs[k])
    return sm.astype(np.float64), sc.astype(np.float64), cs.astype(np.float64)


def lda_covariances(x, offs, rows=None, pivot=None, dtype=np.float64):
    """(mean, T, W): with the rows centred by their mean, T = sum x x^T / N, W = (sum x x^T - sum_s sum_s sum_s^T / n_s) / N.
    The row statistics are taken about `pivot` in `dtype` and re-centred in float64."""
    offs = np.asarray(offs, dtype=np.int64)
    sm, sc, cs = class_stats(x, offs, rows, pivot, dtype)
    N = float(offs[-1])
    p = np.zeros_like(sm) if pivot is None else np.asarray(pivot, dtype=np.float64)
    delta = sm / N
    tot = sc - N * np.outer(delta, delta)
    between = np.zeros_like(tot)
    for s in range(len(offs) - 1):
        ns = float(offs[s + 1] - offs[s])
        if ns > 0:
            c = cs[s] - ns * delta
            between += np.outer(c, c) / ns
    return p + delta, tot / N, (tot - between) / N


def lda_transform(T, W, lda_dim, f=0.0, covariance_floor=1e-6):
    """-> (A (lda_dim, D), all D eigenvalues of P B P^T descending)."""
    M = f * T + (1.0 - f) * W
    e, U = np.linalg.eigh(0.5 * (M + M.T))
    e = np.maximum(e, e.max() * covariance_floor)
    P = np.diag(e ** -0.5) @ U.T
    G = P @ (T - W) @ P.T
    s, V = np.linalg.eigh(0.5 * (G + G.T))
    order = np.argsort(-s)
    s, V = s[order], V[:, order]
    A = V[:, :lda_dim].T @ P
    for i in range(lda_dim):
        if A[i, np.abs(A[i]).argmax()] < 0:
            A[i] = -A[i]
    return A, s


def fit_lda(x, offs, lda_dim, rows=None, pivot=None, dtype=np.float64, f=0.0, covariance_floor=1e-6):
    """[A | -A mean] (lda_dim, D + 1)."""
    mean, T, W = lda_covariances(x, offs, rows, pivot, dtype)
    A, _ = lda_transform(T, W, lda_dim, f, covariance_floor)
    return np.concatenate([A, -(A @ mean)[:, None]], axis=1)


def plda_stats(y, offs, rows=None, pivot=None, dtype=np.float64):
    """PldaStats with unit weights: (class means (S, D), counts (S,), offset_scatter), empty classes dropped."""
    offs = np.asarray(offs, dtype=np.int64)
    _, sc, cs = class_stats(y, offs, rows, pivot, dtype)
    p = np.zeros(sc.shape[0]) if pivot is None else np.asarray(pivot, dtype=np.float64)
    means, counts = [], []
    off = sc.copy()
    for s in range(len(offs) - 1):
        ns = float(offs[s + 1] - offs[s])
        if ns > 0:
            m = cs[s] / ns
            off -= ns * np.outer(m, m)
            means.append(m + p)
            counts.append(ns)
    return np.array(means), np.array(counts), off


def plda_loglike(W, B, mu, means, counts, offset_scatter):
    """Data log-likelihood of the model x_sk = mu + h_s + e_sk, h ~ N(0, B), e ~ N(0, W), from the statistics: per class the
    mean m_s ~ N(mu, B + W / n_s), and the residuals about it contribute -(1/2) [(n_s - 1) log|2 pi W| + tr(W^-1 S_s)]
    (+ a constant from the change of variables that does not depend on the parameters)."""
    D = len(mu)
    Winv = np.linalg.inv(W)
    _, ldW = np.linalg.slogdet(W)
    ll = -0.5 * np.trace(Winv @ offset_scatter)
    for m, n in zip(means, counts):
        C = B + W / n
        _, ld = np.linalg.slogdet(C)
        d = m - mu
        ll += -0.5 * (ld + d @ np.linalg.solve(C, d) + D * np.log(2 * np.pi))
        ll += -0.5 * (n - 1) * (ldW + D * np.log(2 * np.pi))
    return ll


def plda_em(means, counts, offset_scatter, num_em_iters=10, trace=None, init_scale=1.0):
    """The literal per-class loop of PldaEstimator (unit weights) from W = B = init_scale * I (Kaldi: I) -> (W, B, mu); `trace` (a list) receives the
    data log-likelihood before every iteration and after the last."""
    S, D = means.shape
    N = counts.sum()
    mu = means.sum(0) / S
    W, B = init_scale * np.eye(D), init_scale * np.eye(D)
    for _ in range(num_em_iters):
        if trace is not None:
            trace.append(plda_loglike(W, B, mu, means, counts, offset_scatter))
        within_stats, within_count = offset_scatter.copy(), N - S
        between_stats, between_count = np.zeros((D, D)), 0.0
        Binv, Winv = np.linalg.inv(B), np.linalg.inv(W)
        for m, n in zip(means, counts):
            d = m - mu
            V = np.linalg.inv(Binv + n * Winv)
            w = V @ (n * (Winv @ d))
            between_stats += V + np.outer(w, w)
            between_count += 1
            r = d - w
            within_stats += n * V + n * np.outer(r, r)
            within_count += 1
        W = within_stats / within_count
        B = between_stats / between_count
    if trace is not None:
        trace.append(plda_loglike(W, B, mu, means, counts, offset_scatter))
    return W, B, mu


def plda_output(W, B, mu):
    """(mean, transform, psi): W = C C^T, T1 = C^-1, T1 B T1^T = U diag(psi) U^T, psi floored at 0, descending."""
    C = np.linalg.cholesky(0.5 * (W + W.T))
    T1 = np.linalg.inv(C)
    G = T1 @ B @ T1.T
    psi, U = np.linalg.eigh(0.5 * (G + G.T))
    order = np.argsort(-psi)
    psi, U = np.maximum(psi[order], 0.0), U[:, order]
    return mu.copy(), U.T @ T1, psi


def fit_plda(y, offs, num_em_iters=10, rows=None, pivot=None, dtype=np.float64, length_scale=1.0):
    means, counts, off = plda_stats(y, offs, rows, pivot, dtype)
    W, B, mu = plda_em(means * length_scale, counts, off * length_scale ** 2, num_em_iters, init_scale=length_scale ** 2)
    return plda_output(W, B, mu)


def normalise(u):
    return u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-12)


def fit_backend(x, offs, lda_dim, plda_dim=None, rows=None, length_norm="unit", center=None, dtype=np.float64,
                pivot=None, y_pivot=None, num_em_iters=10):
    """The arrays of backend.fit_backend as a dict (mean_vec, transform_mat, plda_mean, plda_transform, psi) plus W, B (the
    LDA's covariances of the centred rows) and lda_eigs.  `dtype` is the accumulation type of the row statistics of BOTH
    passes; the projection y = normalise(A (x - mean)) is float64 on float32-rounded A and bias, as the model holds them."""
    plda_dim = lda_dim if plda_dim is None else plda_dim
    mean, T, W = lda_covariances(x, offs, rows, pivot, dtype)
    A, eigs = lda_transform(T, W, lda_dim)
    tm = np.concatenate([A, np.zeros((lda_dim, 1))], axis=1)
    mean_vec = mean if center is None else np.asarray(center, dtype=np.float64).mean(0)
    A32 = A.astype(np.float32).astype(np.float64)
    b32 = (-(A @ mean)).astype(np.float32).astype(np.float64)
    if dtype == np.float64:
        y = normalise(np.asarray(x, dtype=np.float64) @ A32.T + b32)
    else:  # the projection and the normalisation in float32 arithmetic too
        u = np.asarray(x, dtype=np.float32) @ A32.astype(np.float32).T + b32.astype(np.float32)
        y = u / np.maximum(np.sqrt((u * u).sum(1, dtype=np.float32, keepdims=True)), np.float32(1e-12))
    c = 1.0 if length_norm == "unit" else np.sqrt(lda_dim)
    pm, pt, psi = fit_plda(y, offs, num_em_iters, rows, y_pivot, dtype, c)
    return {"mean_vec": mean_vec, "transform_mat": tm, "plda_mean": pm, "plda_transform": pt[:plda_dim],
            "psi": psi[:plda_dim], "W": W, "B": T - W, "lda_eigs": eigs}


def synth(seed, D0=512, rank=24, S=96, max_utts=60, within_max=0.3, cond=100.0, mean_scale=1.0):
    """Seeded x-vectors of a model with between-class covariance of rank exactly `rank` (variances log-spaced 9 .. 1) and a
    full-rank within-class covariance (eigenvalues log-spaced within_max .. within_max / cond) about a non-zero mean.
    -> dict: table (R, D0) float32 with the rows in shuffled order, ids (R utterance names in table order), spk2utt
    [(spk, [utt ...])], rows / offs (the class layout of spk2utt over the table)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, max_utts + 1, S)
    N = int(counts.sum())
    Vb = np.linalg.qr(rng.standard_normal((D0, rank)))[0]
    sb = np.sqrt(np.logspace(np.log10(9.0), 0.0, rank))
    Qw = np.linalg.qr(rng.standard_normal((D0, D0)))[0]
    sw = np.sqrt(within_max * np.logspace(0.0, -np.log10(cond), D0))
    m0 = mean_scale * rng.standard_normal(D0)
    spk = np.repeat(np.arange(S), counts)
    h = (rng.standard_normal((S, rank)) * sb) @ Vb.T
    x = m0 + h[spk] + (rng.standard_normal((N, D0)) * sw) @ Qw.T
    perm = rng.permutation(N)           # table row of utterance k (in speaker order) is perm[k]
    table = np.empty((N, D0), dtype=np.float32)
    table[perm] = x.astype(np.float32)
    ids = [None] * N
    spk2utt, k = [], 0
    for s in range(S):
        utts = []
        for j in range(counts[s]):
            u = f"spk{s:03d}-utt{j:02d}"
            ids[perm[k]] = u
            utts.append(u)
            k += 1
        spk2utt.append((f"spk{s:03d}", utts))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return {"table": table, "ids": ids, "spk2utt": spk2utt, "rows": perm.astype(np.int64), "offs": offs}
