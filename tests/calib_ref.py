"""fp64 numpy reference of the calibration kernels (csrc/nplda_calib.hip): the prior-weighted logistic objective with its
gradient and Hessian, the damped Newton iteration, Cllr and the error counts, and the Gaussian model through
scipy.stats.norm (the authority utils/score_calibration.py itself uses).  Written from the formulas of
design/k16_calibration.md, independently of the device code: softplus through np.logaddexp, sigma in its two-branch form.
"""
import numpy as np
import scipy.stats

MAX_HALVINGS = 20
EPS = np.finfo(np.float64).eps


def recipe(N, K, seed=None):
    """The test inputs: every eighth trial a target, K correlated systems of growing scale, noise and offset; X in fp32."""
    rg = np.random.default_rng(1000 * K + N % 997 if seed is None else seed)
    t = (np.arange(N) % 8 == 3).astype(np.float64)
    base = 4.0 * t - 2.0 + 1.5 * rg.standard_normal(N)
    X = np.empty((N, K), dtype=np.float64)
    for k in range(K):
        X[:, k] = base * (1.0 + 0.25 * k) + k * rg.standard_normal(N) + 0.5 * k
    return X.astype(np.float32), t.astype(np.float32)


def sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    return np.logaddexp(0.0, np.asarray(z, dtype=np.float64))


def triu_pack(M):
    return M[np.triu_indices(M.shape[0])]


def triu_unpack(h, n):
    M = np.zeros((n, n))
    M[np.triu_indices(n)] = h
    return M + np.triu(M, 1).T


def logreg_pass(X, t, theta, p_target=0.5, l2=0.0):
    """-> dict: n_tgt, n_non, J, g (K + 1), H ((K + 1, K + 1)), and J_abs / g_abs / H_abs = the sums of the absolute values
    of the terms each is made of (what a relative error bound of a sum refers to)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    t = np.asarray(t, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    N, K = X.shape
    tg, ng = t > 0.5, t < 0.5
    nt, nn = int(tg.sum()), int(ng.sum())
    keep = tg | ng
    Xk, tk = X[keep], tg[keep]
    w = np.where(tk, p_target / max(nt, 1), (1.0 - p_target) / max(nn, 1))
    tau = np.log(p_target) - np.log1p(-p_target)
    A = np.concatenate([Xk, np.ones((Xk.shape[0], 1))], axis=1)
    z = A @ theta + tau
    sp = np.where(tk, softplus(-z), softplus(z))
    r = np.where(tk, -sigmoid(-z), sigmoid(z))  # sigma - t without cancellation
    s1 = sigmoid(z) * sigmoid(-z)
    a = theta[:K]
    ridge_g = np.append(l2 * a, 0.0)
    ridge_H = l2 * np.diag(np.append(np.ones(K), 0.0))
    return {
        "n_tgt": nt, "n_non": nn,
        "J": float(np.sum(w * sp) + 0.5 * l2 * np.sum(a * a)),
        "g": A.T @ (w * r) + ridge_g,
        "H": (A * (w * s1)[:, None]).T @ A + ridge_H,
        "J_abs": float(np.sum(w * sp) + 0.5 * l2 * np.sum(a * a)),
        "g_abs": np.abs(A).T @ (w * np.abs(r)) + np.abs(ridge_g),
        "H_abs": (np.abs(A) * (w * s1)[:, None]).T @ np.abs(A) + ridge_H,
    }


def newton(X, t, p_target=0.5, l2=0.0, max_passes=64, tol=1e-10, init=None):
    """The damped Newton iteration of the step kernel: solve H d = g by Cholesky, accept theta - alpha d if J did not
    increase (beyond 8 ulp of J: the rounding of the sum), else halve alpha, at most 20 times in a row.
    -> (theta, info) with info = objective, grad_inf, iterations, passes, converged, not_finite, stalled."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    K = X.shape[1]
    acc = np.append(np.full(K, 1.0 / K), 0.0) if init is None else np.asarray(init, dtype=np.float64).copy()
    trial = acc.copy()
    info = dict(objective=np.nan, grad_inf=np.nan, iterations=0, passes=0, converged=False, not_finite=False,
                stalled=False)
    have, alpha, halvings, d = False, 1.0, 0, None
    while info["passes"] < max_passes:
        r = logreg_pass(X, t, trial, p_target, l2)
        info["passes"] += 1
        if not (r["n_tgt"] and r["n_non"] and np.isfinite(r["J"]) and np.isfinite(r["g"]).all() and np.isfinite(r["H"]).all()):
            info["not_finite"] = True
            break
        if not have or r["J"] <= info["objective"] + 8.0 * EPS * abs(info["objective"]):
            acc, have = trial.copy(), True
            info["objective"], info["grad_inf"] = r["J"], float(np.abs(r["g"]).max())
            if info["grad_inf"] <= tol:
                info["converged"] = True
                break
            try:
                L = np.linalg.cholesky(r["H"])
            except np.linalg.LinAlgError:
                info["not_finite"] = True
                break
            d = np.linalg.solve(L.T, np.linalg.solve(L, r["g"]))
            alpha, halvings = 1.0, 0
            info["iterations"] += 1
        else:
            if halvings >= MAX_HALVINGS:
                info["stalled"] = True
                break
            halvings += 1
            alpha *= 0.5
        trial = acc - alpha * d
    return acc, info


def cllr_sums(llr, t):
    """(sum_tgt log2(1 + exp(-llr)), sum_non log2(1 + exp(llr)), N_tgt, N_non)."""
    llr, t = np.asarray(llr, dtype=np.float64), np.asarray(t)
    tg, ng = t > 0.5, t < 0.5
    return (float(np.sum(softplus(-llr[tg]))) / np.log(2.0), float(np.sum(softplus(llr[ng]))) / np.log(2.0), int(tg.sum()),
            int(ng.sum()))


def cllr(llr, t):
    st, sn, nt, nn = cllr_sums(llr, t)
    return 0.5 * (st / nt + sn / nn)


def counts(llr, t, thresholds):
    """(misses, false alarms) per threshold: llr < th on targets, llr >= th on non-targets."""
    llr, t = np.asarray(llr, dtype=np.float64), np.asarray(t)
    tg, ng = t > 0.5, t < 0.5
    return ([int(np.sum(llr[tg] < th)) for th in thresholds], [int(np.sum(llr[ng] >= th)) for th in thresholds])


def gauss_train(scores, t):
    """The reference's model: {'tgt': norm(mean, std), 'imp': norm(mean, std)}, population standard deviations."""
    s, t = np.asarray(scores, dtype=np.float64), np.asarray(t)
    return {"tgt": scipy.stats.norm(np.mean(s[t > 0.5]), np.std(s[t > 0.5])),
            "imp": scipy.stats.norm(np.mean(s[t < 0.5]), np.std(s[t < 0.5]))}


def gauss_apply(scores, mdl):
    s = np.asarray(scores, dtype=np.float64)
    return mdl["tgt"].logpdf(s) - mdl["imp"].logpdf(s)
