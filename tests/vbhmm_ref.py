"""Numpy twins of the VB-HMM resegmentation (csrc/nplda_vbhmm.hip, design/k22_vbhmm.md), a plain helper of the tests.

vbhmm(): the published log-domain form (Landini et al., "Bayesian HMM clustering of x-vector sequences", 2022): a dense S x S
transition matrix and logsumexp recursions, in float64 or longdouble.  vbhmm_scaled(): a second float64 formulation with the
recursions normalised at every step, the O(S) step of a diagonal-plus-rank-one transition, and sums in another order.
One problem is one recording: x (T, D) rows in time order in the space where the within-class covariance is I and the
between-class covariance diag(psi).

The accuracy yardstick is the project's own (tests/fp32_units.py) one precision up: the error of `got` against the longdouble
twin in units of the float64 twin's own error, floored at 2^-53 of the reference."""
import numpy as np

from tests import fp32_units

TINY = 2.0 ** -53
RMS_MAX, MAX_MAX = fp32_units.RMS_MAX, fp32_units.MAX_MAX
LN2PI = "1.837877066409345483560659472811235279722794947275566825634"


def _lse(a, axis):
    """logsumexp in the dtype of a; an all -inf slice gives -inf."""
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def gamma_from_labels(labels, S, smooth=5.0, dtype=np.float64):
    """softmax_s(smooth [s = label_t]); a label outside 0 .. S - 1 gives the uniform row."""
    labels = np.asarray(labels)
    v = np.zeros((labels.size, S), dtype)
    ok = (labels >= 0) & (labels < S)
    v[np.flatnonzero(ok), labels[ok]] = smooth
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def hard_labels(gamma):
    """(labels, n_speakers): argmax_s with the lowest s among equal values, renumbered to the dense rank of the speakers that
    own a row, in order of s."""
    T, S = gamma.shape
    if T == 0:
        return np.zeros(0, np.int32), 0
    best = np.argmax(gamma, axis=1)
    owns = np.zeros(S, bool)
    owns[best] = True
    rank = np.cumsum(owns) - 1
    return rank[best].astype(np.int32), int(owns.sum())


class Result:
    def __init__(self, gamma, pi, elbo, n_iters):
        self.gamma, self.pi, self.elbo, self.n_iters = gamma, pi, elbo, n_iters
        self.labels, self.n_speakers = hard_labels(gamma)


def _models(x, rho, psi, gamma, Fa, Fb, G, dt):
    r = dt(Fa) / dt(Fb)
    N = gamma.sum(axis=0)
    invL = 1 / (1 + r * N[:, None] * psi[None, :])
    alpha = r * invL * (gamma.T @ rho)
    ll = dt(Fa) * (rho @ alpha.T - (((invL + alpha * alpha) * psi[None, :]).sum(axis=1) / 2)[None, :] + G[:, None])
    kl = dt(Fb) / 2 * np.sum(np.log(invL) - invL - alpha * alpha + 1)
    return ll, kl


def _prepare(x, psi, dt):
    x, psi = np.asarray(x).astype(dt), np.asarray(psi).astype(dt)
    rho = x * np.sqrt(psi)[None, :]
    G = -(np.sum(x * x, axis=1) + x.shape[1] * dt(LN2PI)) / 2
    return x, psi, rho, G


def vbhmm(x, psi, gamma0, pi0=None, Fa=0.3, Fb=17.0, loop=0.99, eps=1e-4, max_iters=40, dtype=np.float64):
    """The log-domain twin -> Result.  elbo has max_iters entries, NaN where not executed."""
    dt = np.dtype(dtype).type
    x, psi, rho, G = _prepare(x, psi, dt)
    T, D = x.shape
    gamma = np.asarray(gamma0).astype(dt)
    S = gamma.shape[1]
    pi = np.full(S, dt(1) / dt(S), dt) if pi0 is None else np.asarray(pi0).astype(dt)
    elbo = np.full(max_iters, np.nan, dt)
    if T == 0:
        return Result(gamma, pi, elbo, 0)
    loop = dt(loop)
    n = 0
    for it in range(max_iters):
        ll, kl = _models(x, rho, psi, gamma, Fa, Fb, G, dt)
        tr = np.eye(S, dtype=dt) * loop + (1 - loop) * pi[None, :]
        with np.errstate(divide="ignore"):
            ltr, lpi = np.log(tr), np.log(pi)
        lf = np.empty((T, S), dt)
        lb = np.zeros((T, S), dt)
        lf[0] = ll[0] + lpi
        for t in range(1, T):
            lf[t] = ll[t] + _lse(lf[t - 1][:, None] + ltr, axis=0)
        for t in range(T - 2, -1, -1):
            lb[t] = _lse(ltr + (ll[t + 1] + lb[t + 1])[None, :], axis=1)
        tll = _lse(lf[T - 1], axis=0)
        gamma = np.exp(lf + lb - tll)
        elbo[it] = tll + kl
        pi = gamma[0] + (1 - loop) * pi * np.sum(np.exp(_lse(lf[:-1], axis=1)[:, None] + ll[1:] + lb[1:] - tll), axis=0)
        pi = pi / pi.sum()
        n = it + 1
        if it >= 1 and elbo[it] - elbo[it - 1] < eps:
            break
    return Result(gamma, pi, elbo, n)


def vbhmm_scaled(x, psi, gamma0, pi0=None, Fa=0.3, Fb=17.0, loop=0.99, eps=1e-4, max_iters=40):
    """The second float64 formulation: per-step normalisation, the O(S) step, sums in another order (reversed, or einsum)."""
    dt = np.float64
    x, psi, rho, G = _prepare(x, psi, dt)
    T, D = x.shape
    gamma = np.asarray(gamma0, dt).copy()
    S = gamma.shape[1]
    pi = np.full(S, 1.0 / S) if pi0 is None else np.asarray(pi0, dt).copy()
    elbo = np.full(max_iters, np.nan)
    if T == 0:
        return Result(gamma, pi, elbo, 0)
    r = Fa / Fb
    n = 0
    for it in range(max_iters):
        N = gamma[::-1].sum(axis=0)
        invL = 1.0 / (1.0 + r * N[:, None] * psi[None, :])
        alpha = r * invL * np.einsum("ts,td->sd", gamma[::-1], rho[::-1])
        K = 0.5 * np.einsum("sd,d->s", invL + alpha * alpha, psi)
        ll = Fa * (np.einsum("td,sd->ts", rho[:, ::-1], alpha[:, ::-1]) - K[None, :] + G[:, None])
        live = pi > 0
        m = np.max(np.where(live[None, :], ll, -np.inf), axis=1)
        with np.errstate(over="ignore"):
            p = np.where(live[None, :], np.exp(ll - m[:, None]), 0.0)
        f, b, c = np.empty((T, S)), np.empty((T, S)), np.empty(T)
        a = pi * p[0]
        c[0] = a.sum()
        f[0] = a / c[0]
        for t in range(1, T):
            a = (loop * f[t - 1] + (1.0 - loop) * pi) * p[t]
            c[t] = a.sum()
            f[t] = a / c[t]
        b[T - 1] = 1.0
        for t in range(T - 2, -1, -1):
            q = p[t + 1] * b[t + 1]
            u = float(pi @ q)
            bt = loop * q + (1.0 - loop) * u
            b[t] = bt / bt.sum()
        g = (f * b).sum(axis=1)
        gamma = f * b / g[:, None]
        elbo[it] = float(np.sum((np.log(c) + m)[::-1])) + 0.5 * Fb * float(np.sum(np.log(invL) - invL - alpha * alpha + 1.0))
        pi = gamma[0] + (1.0 - loop) * pi * np.sum((p[1:] * b[1:] / (c[1:] * g[1:])[:, None])[::-1], axis=0)
        pi = pi / pi.sum()
        n = it + 1
        if it >= 1 and elbo[it] - elbo[it - 1] < eps:
            break
    return Result(gamma, pi, elbo, n)


def make_problem(seed, T, S, D=128, sep=0.25, K=None, stay=0.9, corrupt=0.1):
    """(x float32 (T, D), psi float64 (D,), labels int32 (T,) in 0 .. S - 1, truth (T,)): K true speakers with means ~ N(0, psi),
    psi_d = sep 0.97^d, a sticky speaker sequence, unit within-class noise; the initial labels over-cluster (speaker k owns
    the slots s = k mod K) and a share `corrupt` of them is drawn afresh."""
    rng = np.random.default_rng(seed)
    K = max(1, min(S, (S + 1) // 2)) if K is None else K
    psi = sep * 0.97 ** np.arange(D)
    means = rng.standard_normal((K, D)) * np.sqrt(psi)[None, :]
    truth = np.empty(T, np.int64)
    cur = int(rng.integers(K))
    for t in range(T):
        if t and rng.random() >= stay:
            cur = int(rng.integers(K))
        truth[t] = cur
    x = (means[truth] + rng.standard_normal((T, D))).astype(np.float32)
    slots = [np.flatnonzero(np.arange(S) % K == k) for k in range(K)]
    labels = np.array([rng.choice(slots[k]) for k in truth], np.int64).reshape(T)
    bad = rng.random(T) < corrupt
    labels[bad] = rng.integers(S, size=int(bad.sum()))
    return x, psi, labels.astype(np.int32), truth


def units(got, ref_ld, ref_64):
    """(rms_ratio, max_ratio) of got - ref_ld in units of ref_64 - ref_ld, floored at 2^-53 of the reference's rms / max."""
    got, ld, r64 = (np.asarray(v, np.longdouble).ravel() for v in (got, ref_ld, ref_64))
    assert got.shape == ld.shape == r64.shape, (got.shape, ld.shape, r64.shape)
    if got.size == 0:
        return 0.0, 0.0
    if not np.all(np.isfinite(got)):
        return float("inf"), float("inf")
    e, e64 = got - ld, r64 - ld
    rms = lambda v: float(np.sqrt(np.mean(v * v)))  # noqa: E731
    den_r, den_m = max(rms(e64), TINY * rms(ld)), max(float(np.abs(e64).max()), TINY * float(np.abs(ld).max()))
    num_r, num_m = rms(e), float(np.abs(e).max())
    return (num_r / den_r if num_r else 0.0), (num_m / den_m if num_m else 0.0)


def assert_fp64_level(got, ref_ld, ref_64, what):
    r = units(got, ref_ld, ref_64)
    assert r[0] <= RMS_MAX and r[1] <= MAX_MAX, f"{what}: {r} float64 units, above {RMS_MAX} (rms) / {MAX_MAX} (max)"
    return r


def check_result(got, ld, r64, what, executed=None):
    """gamma, pi and the executed part of the ELBO trace of `got` (anything with those attributes) within the gates ->
    {name: (rms_ratio, max_ratio)}."""
    n = ld.n_iters if executed is None else executed
    out = {"gamma": assert_fp64_level(got.gamma, ld.gamma, r64.gamma, what + " gamma"),
           "pi": assert_fp64_level(got.pi, ld.pi, r64.pi, what + " pi"),
           "elbo": assert_fp64_level(np.asarray(got.elbo)[:n], ld.elbo[:n], r64.elbo[:n], what + " elbo")}
    return out


def pick_epsilon(elbo, floor=1e-4):
    """A stop threshold that no rounding can move: the geometric mean of two consecutive ELBO gains of a never-stopping
    trace that differ by at least 4x, both at least `floor` (far above the ELBO's rounding error), the LAST such pair for
    which EVERY gain of the trace lies outside [eps / 2, 2 eps] -> (eps, number of iterations a run with it executes) or
    None."""
    gains = np.diff(np.asarray(elbo, np.float64))
    for i in range(gains.size - 2, -1, -1):
        a, b = gains[i], gains[i + 1]
        if b >= floor and a >= 4 * b:
            eps = float(np.sqrt(a * b))
            if not ((gains >= eps / 2) & (gains <= 2 * eps)).any():
                return eps, int(np.flatnonzero(gains < eps)[0]) + 2
    return None


def top_two_margin(gamma):
    """The smallest difference between a row's two largest posteriors (1 for a single speaker)."""
    if gamma.shape[1] < 2:
        return 1.0
    s = np.sort(np.asarray(gamma, np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())
