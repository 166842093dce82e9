"""Score calibration and fusion — counterpart of utils/score_calibration.py.

The reference file is a module-level script with hard-coded paths (:30-34) around two functions: `calibrate_train` fits
one Gaussian per class on a development score list, `calibrate_apply` turns scores into the difference of the two log
densities.  Here:

* `calibrate_train(train_scores, train_labels)` / `calibrate_apply(scores, calib_mdl)` — the reference's names, argument
  order and semantics (labels 'target' / 'tgt' and 'nontarget' / 'imp', anything else ignored; population standard
  deviation), on the kernels nplda_calib_gauss_fit_* / nplda_calib_apply_gauss_*.
* `fit_linear(scores, target, ...)` -> `LinearCalibration` — what the field uses instead: prior-weighted linear logistic
  regression, `llr = sum_k a_k s_k + b`, over one system (calibration) or up to eight (fusion + calibration), a damped
  Newton iteration whose every pass is one fused reduction kernel (nplda_calib_logreg_fit_*, design/k16_calibration.md).
* `fit_pav(scores, target, laplace=True)` -> `PavCalibration` — the non-parametric alternative: isotonic regression of the
  labels on the scores (PAV), as the lower convex hull of the cumulative counts (nplda_pav_fit_*, design/k18_pav_rocch.md).
* `calibrate_scorefile(dev_score_file, dev_key_file, score_file, ...)` — the script body as a file-in / file-out function.

CPU tensors / arrays are moved to the HIP device and results come back where the inputs were; there is no CPU
implementation.  Metrics for the result: neuralplda_amd.metrics.cllr / act_cost / act_dcf.
"""
import os
import warnings

import numpy as np
import torch

from . import _lib, ops

__all__ = ["GaussianCalibration", "LinearCalibration", "PavCalibration", "calibrate_train", "calibrate_apply", "fit_linear",
           "fit_pav", "calibrate_scorefile", "labels_to_target"]

TARGET_LABELS = ("target", "tgt")        # utils/score_calibration.py:15
NONTARGET_LABELS = ("nontarget", "imp")  # :16


def _device(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise _lib.NpldaHipError("score calibration needs a HIP device (there is no CPU implementation)")
    return torch.device("cuda", torch.cuda.current_device())


def _scores_to(x, dev):
    """float32 / float64 device tensor of the scores (other dtypes -> float64)."""
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.to(dev)


def _back(out, like):
    """Result where (and as what) the input was: numpy for numpy, CPU tensor for CPU tensor."""
    if isinstance(like, torch.Tensor):
        return out if like.device == out.device else out.to(like.device)
    return out.cpu().numpy()


def labels_to_target(labels, dev=None):
    """0/1 arrays or tensors as they are; label strings -> 1.0 for 'target' / 'tgt', 0.0 for 'nontarget' / 'imp' and 0.5
    (neither class: the kernels ignore the trial) for anything else, as the reference's masks do.  float32 tensor."""
    if isinstance(labels, torch.Tensor):
        t = labels.detach().reshape(-1).to(torch.float32)
    else:
        arr = np.asarray(labels).reshape(-1)
        if arr.dtype.kind in "USO":
            arr = arr.astype(str)
            num = np.full(arr.shape, 0.5, dtype=np.float32)
            num[np.isin(arr, TARGET_LABELS)] = 1.0
            num[np.isin(arr, NONTARGET_LABELS)] = 0.0
            arr = num
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return t if dev is None else t.to(dev)


class _Normal:
    """What the reference's dict holds per class (a frozen scipy.stats.norm), as far as its callers use it."""
    __slots__ = ("mu", "sigma")

    def __init__(self, mu, sigma):
        self.mu, self.sigma = float(mu), float(sigma)

    def mean(self):
        return self.mu

    def std(self):
        return self.sigma

    def logpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        return -0.5 * np.log(2 * np.pi) - np.log(self.sigma) - (x - self.mu) ** 2 / (2 * self.sigma ** 2)


class GaussianCalibration:
    """One Gaussian per class: mu_tgt, std_tgt, mu_imp, std_imp (+ the class counts).  model['tgt'] / model['imp'] index it
    like the reference's dict."""
    __slots__ = ("mu_tgt", "std_tgt", "mu_imp", "std_imp", "n_tgt", "n_imp")

    def __init__(self, mu_tgt, std_tgt, mu_imp, std_imp, n_tgt=0, n_imp=0):
        self.mu_tgt, self.std_tgt, self.mu_imp, self.std_imp = float(mu_tgt), float(std_tgt), float(mu_imp), float(std_imp)
        self.n_tgt, self.n_imp = int(n_tgt), int(n_imp)

    def __getitem__(self, key):
        if key == "tgt":
            return _Normal(self.mu_tgt, self.std_tgt)
        if key == "imp":
            return _Normal(self.mu_imp, self.std_imp)
        raise KeyError(key)

    def apply(self, scores):
        return calibrate_apply(scores, self)

    def __repr__(self):
        return (f"GaussianCalibration(mu_tgt={self.mu_tgt!r}, std_tgt={self.std_tgt!r}, mu_imp={self.mu_imp!r}, "
                f"std_imp={self.std_imp!r})")


def calibrate_train(train_scores, train_labels):
    """utils/score_calibration.py:14-24.  ValueError on an empty class or a zero standard deviation (the reference returns
    nan there)."""
    dev = _device(train_scores, train_labels)
    s = _scores_to(train_scores, dev).reshape(-1)
    t = labels_to_target(train_labels, dev)
    if s.numel() != t.numel():
        raise ValueError("one label per score")
    if s.numel() < 2:
        raise ValueError("calibration needs scores of both classes")
    nt, mt, st, nn, mn, sn = ops.calib_gauss_fit(s, t).tolist()
    if nt < 1 or nn < 1:
        raise ValueError(f"calibration needs scores of both classes (got {int(nt)} targets, {int(nn)} non-targets)")
    if not (st > 0.0 and sn > 0.0 and np.isfinite([mt, st, mn, sn]).all()):
        raise ValueError(f"degenerate class statistics (std_tgt = {st}, std_imp = {sn})")
    return GaussianCalibration(mt, st, mn, sn, nt, nn)


def calibrate_apply(scores, calib_mdl):
    """utils/score_calibration.py:26-28: log N(s; tgt) - log N(s; imp), float64, shaped and placed like `scores`."""
    if isinstance(calib_mdl, GaussianCalibration):
        m = calib_mdl
    else:  # the reference's dict of frozen distributions
        m = GaussianCalibration(calib_mdl["tgt"].mean(), calib_mdl["tgt"].std(), calib_mdl["imp"].mean(), calib_mdl["imp"].std())
    dev = _device(scores)
    s = _scores_to(scores, dev)
    if s.numel() == 0:
        return _back(torch.empty(s.shape, dtype=torch.float64, device=dev), scores)
    try:
        out = ops.calib_apply_gauss(s, m.mu_tgt, m.std_tgt, m.mu_imp, m.std_imp)
    except _lib.NpldaHipError as e:
        if not (m.std_tgt > 0 and m.std_imp > 0):
            raise ValueError("the model's standard deviations must be positive") from e
        raise
    return _back(out, scores)


class LinearCalibration:
    """llr = sum_k a[k] * scores[:, k] + b.  a (K,) and b are Python floats / a numpy array; objective, grad_inf,
    iterations, passes and converged describe the fit that produced them."""
    __slots__ = ("a", "b", "p_target", "l2", "objective", "grad_inf", "iterations", "passes", "converged")

    def __init__(self, a, b, p_target=0.5, l2=0.0, objective=float("nan"), grad_inf=float("nan"), iterations=0, passes=0,
                 converged=True):
        self.a = np.atleast_1d(np.asarray(a, dtype=np.float64))
        self.b = float(b)
        self.p_target, self.l2 = float(p_target), float(l2)
        self.objective, self.grad_inf = float(objective), float(grad_inf)
        self.iterations, self.passes, self.converged = int(iterations), int(passes), bool(converged)

    def apply(self, scores, out_dtype=torch.float64):
        dev = _device(scores)
        s = _scores_to(scores, dev)
        K = 1 if s.dim() == 1 else s.shape[-1]
        if K != self.a.size:
            raise ValueError(f"this calibration fuses {self.a.size} systems, got {K}")
        if s.shape[0] == 0:
            return _back(torch.empty(0, dtype=out_dtype, device=dev), scores)
        theta = torch.from_numpy(np.append(self.a, self.b)).to(dev)
        return _back(ops.calib_apply_linear(s, theta, out_dtype=out_dtype), scores)

    def __repr__(self):
        return (f"LinearCalibration(a={self.a.tolist()!r}, b={self.b!r}, objective={self.objective!r}, "
                f"grad_inf={self.grad_inf!r}, passes={self.passes}, converged={self.converged})")


def fit_linear(scores, target, p_target=0.5, l2=0.0, max_passes=64, tol=1e-10, init=None):
    """Prior-weighted linear logistic regression: minimise
        J = p_target / N_tgt * sum_tgt softplus(-z) + (1 - p_target) / N_non * sum_non softplus(z) + l2 / 2 * |a|^2,
        z = a . s + b + logit(p_target),
    by damped Newton on the device from a = 1 / K, b = 0 (or `init` = K + 1 numbers).  scores (N,) or (N, K <= 8).
    Raises ValueError without both classes and NpldaHipError when the objective is not finite (a NaN score);
    warns and returns converged=False when max_passes ran out first (separable data with l2 = 0 can do that)."""
    dev = _device(scores, target)
    s = _scores_to(scores, dev)
    t = labels_to_target(target, dev)
    K = 1 if s.dim() == 1 else s.shape[-1]
    if s.dim() not in (1, 2) or s.shape[0] != t.numel():
        raise ValueError("scores must be (N,) or (N, K) with one target per row")
    if not 0.0 < p_target < 1.0:
        raise ValueError("p_target must lie strictly between 0 and 1")
    if l2 < 0.0:
        raise ValueError("l2 must not be negative")
    if s.shape[0] < 2:
        raise ValueError("calibration needs trials of both classes")
    if init is None:
        start = np.append(np.full(K, 1.0 / K), 0.0)
    else:
        start = np.asarray(init, dtype=np.float64).reshape(-1)
        if start.size != K + 1:
            raise ValueError(f"init must hold K + 1 = {K + 1} numbers")
    theta = torch.from_numpy(start.copy()).to(dev)
    rep = dict(zip(ops.CALIB_REPORT, ops.calib_logreg_fit(s, t, theta, p_target=p_target, l2=l2, max_passes=max_passes,
                                                          tol=tol).tolist()))
    if rep["n_tgt"] < 1 or rep["n_non"] < 1:
        raise ValueError(f"calibration needs trials of both classes (got {int(rep['n_tgt'])} targets, "
                         f"{int(rep['n_non'])} non-targets)")
    if rep["not_finite"]:
        raise _lib.NpldaHipError("the calibration objective, its gradient or its Hessian is not finite (NaN / inf scores?) "
                                 "or the Hessian is not positive definite; theta was left at its last accepted value")
    th = theta.cpu().numpy()
    conv = bool(rep["converged"])
    if not conv:
        warnings.warn(f"fit_linear stopped after {int(rep['passes'])} passes without convergence "
                      f"(max |g| = {rep['grad_inf']:.3e} > tol = {tol:.1e}"
                      f"{'; the line search stalled' if rep['stalled'] else ''})", RuntimeWarning, stacklevel=2)
    return LinearCalibration(th[:K], th[K], p_target, l2, rep["objective"], rep["grad_inf"], rep["iterations"], rep["passes"],
                             conv)


class PavCalibration:
    """The block table of a PAV fit: block b covers the scores lo[b] .. hi[b] (n[b] trials, t[b] targets, the two dummy
    trials of the Laplace rule included) and maps them to llr[b]; between blocks the map is linear in the score.  numpy
    arrays; n_tgt, n_non are the class counts of the trials the fit kept."""
    __slots__ = ("lo", "hi", "llr", "n", "t", "laplace", "n_tgt", "n_non", "bins")

    def __init__(self, lo, hi, llr, n, t, laplace=True, n_tgt=0, n_non=0, bins=0):
        self.lo, self.hi, self.llr = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (lo, hi, llr))
        self.n, self.t = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (n, t))
        if not (self.lo.size == self.hi.size == self.llr.size == self.n.size == self.t.size >= 1):
            raise ValueError("lo, hi, llr, n and t must hold one entry per block, at least one")
        self.laplace, self.n_tgt, self.n_non, self.bins = bool(laplace), int(n_tgt), int(n_non), int(bins)

    def apply(self, scores, out_dtype=torch.float64):
        dev = _device(scores)
        s = _scores_to(scores, dev)
        if s.numel() == 0:
            return _back(torch.empty(s.shape, dtype=out_dtype, device=dev), scores)
        lo, hi, llr = (torch.from_numpy(x).to(dev) for x in (self.lo, self.hi, self.llr))
        return _back(ops.pav_apply(s, lo, hi, llr, out_dtype=out_dtype), scores)

    def __repr__(self):
        return (f"PavCalibration({self.llr.size} blocks over {self.bins} bins, laplace={self.laplace}, "
                f"llr {self.llr[0]:.4f} .. {self.llr[-1]:.4f})")


def fit_pav(scores, target, laplace=True):
    """Isotonic (PAV) calibration: the monotone map of the scores to log-likelihood ratios that minimises Cllr on the
    data.  laplace=True adds one target and one non-target at each of -inf and +inf, which keeps the end blocks finite.
    Trials with a NaN score or a label that is neither class are ignored.  Raises ValueError without both classes."""
    dev = _device(scores, target)
    s = _scores_to(scores, dev).reshape(-1)
    t = labels_to_target(target, dev)
    if s.numel() != t.numel():
        raise ValueError("one label per score")
    if s.numel() < 2:
        raise ValueError("calibration needs trials of both classes")
    cap = None
    for _ in range(2):
        lo, hi, n, tt, llr, summary = ops.pav_fit(s, t, laplace=laplace, cap=cap)
        rep = dict(zip(ops.PAV_SUMMARY, summary.tolist()))
        if rep["n_tgt"] < 1 or rep["n_non"] < 1:
            raise ValueError(f"calibration needs trials of both classes (got {int(rep['n_tgt'])} targets, "
                             f"{int(rep['n_non'])} non-targets)")
        if not rep["overflow"]:
            break
        cap = int(rep["blocks"])  # always the true number of blocks: the second call fits
    nb = int(rep["blocks"])
    return PavCalibration(*(x[:nb].cpu().numpy() for x in (lo, hi, llr, n, tt)), laplace=laplace, n_tgt=rep["n_tgt"],
                          n_non=rep["n_non"], bins=rep["bins"])


def calibrate_scorefile(dev_score_file, dev_key_file, score_file, method="gaussian", label_col=3, dev_skip_header=1,
                        skip_header=1, out=None, **fit_kw):
    """The reference's script body (:39-51): scores from the last column of `dev_score_file`, labels from column
    `label_col` of `dev_key_file` (row for row), a model trained on them, and `score_file` rewritten with its last column
    calibrated and formatted '{:f}'; every other byte of a data row and the header lines are kept.  The output path
    defaults to `score_file` with '_calibrated' in front of the extension.  method: "gaussian" (calibrate_train /
    calibrate_apply), "linear" (fit_linear, fit_kw = its keywords) or "pav" (fit_pav, fit_kw = laplace).  Returns (output
    path, model)."""
    from . import textio
    if method not in ("gaussian", "linear", "pav"):
        raise ValueError('method must be "gaussian", "linear" or "pav"')

    def body(path, skip):
        with open(path, "rb") as fh:
            head = [fh.readline() for _ in range(skip)]  # skip_header counts LINES, before any blank-line handling
            return head, fh.read()

    _, dev_text = body(dev_score_file, dev_skip_header)
    _, key_text = body(dev_key_file, dev_skip_header)
    n_dev, _ = textio.scan(dev_text)
    n_key, key_cols = textio.scan(key_text)
    if n_dev != n_key:
        raise ValueError(f"{n_dev} development scores but {n_key} key rows")
    if not -key_cols <= label_col < key_cols:
        raise ValueError(f"the key file has {key_cols} columns, label_col = {label_col}")
    dev_scores = textio.column_f64(dev_text, -1, n_dev)
    labels = np.array(textio.column_tokens(key_text, label_col, n_key))
    if method == "gaussian":
        model = calibrate_train(dev_scores, labels)
    elif method == "pav":
        model = fit_pav(dev_scores, labels, **fit_kw)
    else:
        model = fit_linear(dev_scores, labels, **fit_kw)
    head, text = body(score_file, skip_header)
    n, _ = textio.scan(text)
    scores = textio.column_f64(text, -1, n)
    cal = np.asarray(model.apply(scores), dtype=np.float64)
    if out is None:
        root, ext = os.path.splitext(score_file)
        out = root + "_calibrated" + ext
    # textio writes shortest round-trip floats; the reference wants '{:f}' (six decimals), so this one column is
    # formatted here and spliced in front of each row's line ending
    lines = text.split(b"\n")
    k = 0
    for j, line in enumerate(lines):
        data = line.split(b"#", 1)[0]  # a row ends at a comment, as in textio.scan
        if not data.split():
            continue
        row = data.rstrip()
        cut = len(row)
        while cut > 0 and not row[cut - 1:cut].isspace():
            cut -= 1
        lines[j] = row[:cut] + "{:f}".format(cal[k]).encode() + line[len(row):]
        k += 1
    if k != n:
        raise ValueError("the score file changed shape while it was rewritten")
    with open(out, "wb") as fh:
        fh.write(b"".join(head) + b"\n".join(lines))
    return out, model
