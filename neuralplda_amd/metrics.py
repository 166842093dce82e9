"""Detection-cost metrics of the validation loop (utils/models.py:406-436).

The reference's `minc` is an O(N_tgt * N) Python loop with a `.cpu().item()` per element; here it is one call of
nplda_detcost_sweep_f32 (device radix sort of (score, label) + prefix scan + one sweep kernel, csrc/nplda_detcost.hip).
CPU tensors are moved to the HIP device first — like the rest of the package there is no CPU implementation.  Two modes:

* reference_semantics=True (default): bit-compatible with the reference INCLUDING its quirks
  (utils/models.py:23-27 `arr2val`): the "count" is the last index of torch.where (= count - 1) and
  1.0 when the set is empty; thresholds are swept over the target scores only; the classes are target > 0.5 and
  target < 0.5, but the two rates are divided by target.sum() and (1 - target).sum() over ALL labels, so a label
  outside {0, 1} is in neither class and still in both normalisers.
* reference_semantics=False: the exact minimum of P_miss + beta * P_fa over all thresholds, the rates divided by the
  class counts.

Trials whose score is NaN are ignored by minc, minc_exact and eer: they are in neither class and change no other
trial's counts (in reference mode their labels still enter the two sums, which the reference forms over all labels).

Calibration-sensitive metrics (no reference counterpart; kernel nplda_calib_costs_*, csrc/nplda_calib.hip) take
log-likelihood ratios instead of arbitrary scores:

* cllr(llr, target): the cost of the LLRs as soft decisions, in bits (0 = perfect, 1 = as good as no system).
* act_cost(llr, target, betas): P_miss + beta * P_fa at the Bayes threshold log(beta) — the cost, beta convention
  (NpldaConf's `beta`) and normalisation of minc_exact, whose minimum over thresholds it can only exceed.
* act_dcf(llr, target, p_target, c_miss, c_fa): the same counts in NIST's normalisation.

Calibration-insensitive counterparts on the ROC convex hull (kernels nplda_pav_*, csrc/nplda_pav.hip,
design/k18_pav_rocch.md), for arbitrary scores:

* min_cllr(scores, target): the Cllr of the best monotone map of the scores (PAV); cllr - min_cllr is the calibration loss.
* rocch_eer(scores, target): the equal error rate on the ROC convex hull; rocch(scores, target): the hull's vertices.

Confidence intervals (kernels nplda_bootstrap_*, csrc/nplda_bootstrap.hip, design/k20_bootstrap.md):

* bootstrap(scores, target, groups1, groups2): EER, min cost (and with llr=True actual cost and Cllr) of n_boot
  resamplings of the groups of both trial sides; bootstrap_ci: percentile intervals; bootstrap_diff: the paired
  comparison of two systems on the same trials under the same resamplings.

Diarization (kernels of csrc/nplda_der.hip, design/k24_der.md; the host side is neuralplda_amd/derscore.py):

* der(ref, hyp, ...): the diarization error rate of NIST md-eval on a frame grid, with the optimal speaker mapping, a
  collar, optional exclusion of overlapped speech and UEM regions -> DerResult (exact integer counts per recording).
"""
import math

import torch

from . import _lib, ops
from .derscore import DerResult, der

__all__ = ["minc", "eer", "minc_exact", "cllr", "act_cost", "act_dcf", "min_cllr", "rocch_eer", "rocch", "bootstrap",
           "bootstrap_ci", "bootstrap_diff", "BootstrapResult", "der", "DerResult"]


def _on_device(output, target):
    dev = None
    for t in (output, target):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            dev = t.device
            break
    if dev is None:
        if not torch.cuda.is_available():
            raise _lib.NpldaHipError("detection-cost metrics need a HIP device (there is no CPU implementation)")
        dev = torch.device("cuda", torch.cuda.current_device())
    s = output.detach().reshape(-1).to(dev, torch.float32)
    t = target.detach().reshape(-1).to(dev, torch.float32)
    return s, t


def _sweep(output, target, betas, exact, want_eer=False):
    s, t = _on_device(output, target)
    mc, th, avg, e = ops.detcost_sweep(s, t, betas, exact=exact, want_eer=want_eer)
    odev = output.device
    back = (lambda x: x if x is None or x.device == odev else x.to(odev))
    return back(mc), back(th), back(avg), back(e)


def minc(output, target, betas, reference_semantics=True):
    """Returns (minc_avg: 0-d float32 tensor, {beta: 0-d threshold tensor}).  Trials whose score is NaN are ignored."""
    _, th, avg, _ = _sweep(output, target, list(betas), exact=not reference_semantics)
    return avg.reshape(()), {beta: th[k] for k, beta in enumerate(betas)}


def minc_exact(output, target, betas):
    """True minimum detection cost: decide 'target' iff s >= th, th swept over every score and +inf.  Trials whose score
    is NaN are ignored."""
    return minc(output, target, betas, reference_semantics=False)


def eer(output, target):
    """Equal error rate (linear interpolation at the P_miss / P_fa crossing).  Trials whose score is NaN are ignored."""
    _, _, _, e = _sweep(output, target, [1.0], exact=True, want_eer=True)
    return float(e.item())


def _llr_on_device(llr, target):
    dev = None
    for t in (llr, target):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            dev = t.device
            break
    if dev is None:
        if not torch.cuda.is_available():
            raise _lib.NpldaHipError("calibration metrics need a HIP device (there is no CPU implementation)")
        dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.as_tensor(llr).detach().reshape(-1)
    if s.dtype not in (torch.float32, torch.float64):
        s = s.to(torch.float64)
    t = torch.as_tensor(target).detach().reshape(-1).to(torch.float32)
    return s.to(dev), t.to(dev)


def _rates(llr, target, thresholds):
    """Host numbers of one nplda_calib_costs_* call: (N_tgt, N_non, misses [..], false alarms [..], Cllr sums (2))."""
    s, t = _llr_on_device(llr, target)
    cnt, miss, fa, sums = ops.calib_costs(s, t, thresholds)
    nt, nn = cnt.tolist()
    if nt < 1 or nn < 1:
        raise ValueError(f"the metric needs trials of both classes (got {nt} targets, {nn} non-targets)")
    return nt, nn, miss.tolist(), fa.tolist(), sums.tolist()


def cllr(llr, target):
    """Cllr = (mean_tgt log2(1 + exp(-llr)) + mean_non log2(1 + exp(llr))) / 2, a float."""
    nt, nn, _, _, sums = _rates(llr, target, ())
    return 0.5 * (sums[0] / nt + sums[1] / nn)


def act_cost(llr, target, betas):
    """-> (average over betas, {beta: P_miss + beta * P_fa}) with the decision 'target' iff llr >= log(beta): minc_exact's
    cost at the threshold a calibrated system would use instead of at the best one."""
    betas = list(betas)
    if not betas:
        raise ValueError("at least one beta")
    nt, nn, miss, fa, _ = _rates(llr, target, [math.log(b) for b in betas])
    costs = [miss[k] / nt + b * (fa[k] / nn) for k, b in enumerate(betas)]
    return sum(costs) / len(costs), dict(zip(betas, costs))  # the average counts a repeated beta as often as it is given


def act_dcf(llr, target, p_target, c_miss=1.0, c_fa=1.0):
    """NIST's normalised actual DCF: (c_miss p_target P_miss + c_fa (1 - p_target) P_fa) / min(c_miss p_target,
    c_fa (1 - p_target)) at the threshold log(c_fa (1 - p_target) / (c_miss p_target))."""
    if not 0.0 < p_target < 1.0 or c_miss <= 0.0 or c_fa <= 0.0:
        raise ValueError("p_target must lie strictly between 0 and 1, the costs must be positive")
    wm, wf = c_miss * p_target, c_fa * (1.0 - p_target)
    nt, nn, miss, fa, _ = _rates(llr, target, [math.log(wf / wm)])
    return (wm * miss[0] / nt + wf * fa[0] / nn) / min(wm, wf)


def _hull(scores, target):
    """One nplda_pav_fit_* call without the Laplace rule -> (n, t) of the blocks (device int64) and the summary as a dict."""
    s, t = _llr_on_device(scores, target)
    if s.numel() < 2:
        raise ValueError("the metric needs trials of both classes")
    cap = None
    for _ in range(2):
        _, _, n, tt, _, summary = ops.pav_fit(s, t, laplace=False, cap=cap)
        rep = dict(zip(ops.PAV_SUMMARY, summary.tolist()))
        if rep["n_tgt"] < 1 or rep["n_non"] < 1:
            raise ValueError(f"the metric needs trials of both classes (got {int(rep['n_tgt'])} targets, "
                             f"{int(rep['n_non'])} non-targets)")
        if not rep["overflow"]:
            break
        cap = int(rep["blocks"])  # the true number is always reported: the second call fits
    nb = int(rep["blocks"])
    return n[:nb], tt[:nb], rep


def min_cllr(scores, target):
    """Cllr, in bits, after the optimal monotone (PAV) map of the scores: a float.  Trials whose score is NaN are ignored."""
    s, t = _llr_on_device(scores, target)
    if s.numel() < 2:
        raise ValueError("the metric needs trials of both classes")
    rep = dict(zip(ops.PAV_SUMMARY, ops.pav_fit(s, t, laplace=False, cap=1)[5].tolist()))  # the table is not wanted
    if rep["n_tgt"] < 1 or rep["n_non"] < 1:
        raise ValueError(f"the metric needs trials of both classes (got {int(rep['n_tgt'])} targets, "
                         f"{int(rep['n_non'])} non-targets)")
    return rep["min_cllr"]


def rocch_eer(scores, target):
    """Equal error rate on the ROC convex hull (P_miss = P_fa on the hull's edge that crosses the diagonal): a float."""
    s, t = _llr_on_device(scores, target)
    if s.numel() < 2:
        raise ValueError("the metric needs trials of both classes")
    rep = dict(zip(ops.PAV_SUMMARY, ops.pav_fit(s, t, laplace=False, cap=1)[5].tolist()))
    if rep["n_tgt"] < 1 or rep["n_non"] < 1:
        raise ValueError(f"the metric needs trials of both classes (got {int(rep['n_tgt'])} targets, "
                         f"{int(rep['n_non'])} non-targets)")
    return rep["rocch_eer"]


def rocch(scores, target):
    """-> (P_fa, P_miss): float64 numpy arrays over the vertices of the ROC convex hull, from (1, 0) (accept everything)
    to (0, 1), for a DET / ROC plot."""
    n, t, rep = _hull(scores, target)
    n, t = n.cpu().numpy(), t.cpu().numpy()
    import numpy as np
    T = np.concatenate(([0], np.cumsum(t))).astype(np.float64)
    F = np.concatenate(([0], np.cumsum(n - t))).astype(np.float64)
    return 1.0 - F / rep["n_non"], T / rep["n_tgt"]


class BootstrapResult:
    """Replicates of one bootstrap call.  columns: {name: (n_boot + 1,) float64 array}, row 0 the point estimate, the
    row of a degenerate replicate (a class left empty by the draw) NaN; names are "min_cost_<beta>" and "eer", then with
    llr "act_cost_<beta>" and "cllr".  totals: (n_boot + 1, 2) int64, the weighted numbers of targets and non-targets."""

    def __init__(self, columns, totals, betas=(), seed=0):
        import numpy as np
        self.columns = {k: np.asarray(v, dtype=np.float64) for k, v in columns.items()}
        self.totals = np.asarray(totals, dtype=np.int64)
        self.betas = tuple(betas)
        self.seed = seed
        n = {v.shape for v in self.columns.values()}
        if len(n) != 1 or len(next(iter(n))) != 1 or self.totals.shape != (next(iter(n))[0], 2):
            raise ValueError("columns must be equally long vectors with one row of totals each")

    @property
    def n_boot(self):
        return self.totals.shape[0] - 1

    @property
    def degenerate(self):
        """Which replicates (of rows 1 .. n_boot) are degenerate: a boolean array."""
        import numpy as np
        bad = np.zeros(self.n_boot, dtype=bool)
        for v in self.columns.values():
            bad |= np.isnan(v[1:])
        return bad

    @property
    def n_degenerate(self):
        return int(self.degenerate.sum())

    def __getitem__(self, name):
        return self.columns[name]


def _group_ids(groups, N, dev, name):
    """-> (int32 device tensor of ids in [0, G), G).  Integer tensors / arrays are ids as given (G = max + 1); anything
    else (strings) is mapped with np.unique; None is one group per trial."""
    import numpy as np
    if groups is None:
        return torch.arange(N, dtype=torch.int32, device=dev), N
    if isinstance(groups, torch.Tensor):
        if groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise TypeError(f"{name} must hold integer ids or strings")
        g = groups.detach().reshape(-1)
        if g.numel() != N:
            raise ValueError(f"{name} must hold one id per trial")
        if N and int(g.min()) < 0:
            raise ValueError(f"{name} holds a negative id")
        return g.to(dev, torch.int32), (int(g.max()) + 1 if N else 0)
    a = np.asarray(groups).reshape(-1)
    if a.size != N:
        raise ValueError(f"{name} must hold one id per trial")
    if a.dtype.kind in "iu":
        if N and int(a.min()) < 0:
            raise ValueError(f"{name} holds a negative id")
        return torch.from_numpy(a.astype(np.int32)).to(dev), (int(a.max()) + 1 if N else 0)
    u, inv = np.unique(a, return_inverse=True)
    return torch.from_numpy(inv.reshape(-1).astype(np.int32)).to(dev), int(u.size)


def _column_names(betas, llr):
    names = [f"min_cost_{b:g}" for b in betas] + ["eer"]
    if llr:
        names += [f"act_cost_{b:g}" for b in betas] + ["cllr"]
    return names


def bootstrap(scores, target, groups1, groups2=None, n_boot=1000, seed=0, betas=(99.0, 199.0), llr=False):
    """Group bootstrap of the detection metrics -> BootstrapResult.  groups1 / groups2: the group (speaker) of each
    trial's two sides, as integer ids or as arrays of names; every replicate redraws the groups of each side with
    replacement and weighs a trial by the product of the draw counts of its two groups.  groups2=None resamples side 1
    alone, groups1=None resamples trials (one group per trial, within the kernel's group limit)."""
    betas = [float(b) for b in betas]
    if len(set(_column_names(betas, llr))) != len(_column_names(betas, llr)):
        raise ValueError("betas must be distinct")
    s, t = _on_device(torch.as_tensor(scores), torch.as_tensor(target))
    N = s.numel()
    g1, G1 = _group_ids(groups1, N, s.device, "groups1")
    g2, G2 = (None, 0) if groups2 is None else _group_ids(groups2, N, s.device, "groups2")
    out, totals, flags = ops.bootstrap_metrics(s, t, g1, G1, g2, G2, n_boot=n_boot, seed=seed, betas=betas, llr=llr)
    bad, sat = flags.tolist()
    if bad:
        raise ValueError(f"{bad} trials have a group id outside the declared range")
    if sat:
        raise _lib.NpldaHipError(f"{sat} draw counts exceeded 255: the replicates are not usable")
    out = out.cpu().numpy()
    return BootstrapResult({n: out[:, j].copy() for j, n in enumerate(_column_names(betas, llr))}, totals.cpu().numpy(),
                           betas=betas, seed=seed)


def _interval(values, alpha):
    import numpy as np
    lo, hi = np.quantile(values, [alpha / 2, 1 - alpha / 2], method="linear")
    return float(lo), float(hi)


def bootstrap_ci(result, alpha=0.05, max_degenerate=0.05, **kwargs):
    """Percentile intervals -> {name: (point, lo, hi)} over the non-degenerate replicates of a BootstrapResult (or of
    bootstrap(*result, **kwargs) when `result` is a tuple of its arguments).  Raises when more than the share
    max_degenerate of the replicates is degenerate: an interval over the rest would be biased."""
    if not isinstance(result, BootstrapResult):
        result = bootstrap(*result, **kwargs)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie strictly between 0 and 1")
    bad = result.degenerate
    if result.n_boot < 1 or bad.sum() > max_degenerate * result.n_boot or bad.all():
        raise ValueError(f"{int(bad.sum())} of {result.n_boot} replicates are degenerate (a class left empty); "
                         f"the allowed share is {max_degenerate}")
    return {n: (float(v[0]),) + _interval(v[1:][~bad], alpha) for n, v in result.columns.items()}


def bootstrap_diff(scores_a, scores_b, target, groups1, groups2=None, n_boot=1000, seed=0, betas=(99.0, 199.0), llr=False,
                   alpha=0.05, max_degenerate=0.05):
    """Paired comparison of two systems on the same trials: two bootstrap calls with one seed, hence the same weights ->
    (diff: BootstrapResult of a - b per replicate, {name: (point, lo, hi, excludes_zero)})."""
    ra = bootstrap(scores_a, target, groups1, groups2, n_boot=n_boot, seed=seed, betas=betas, llr=llr)
    rb = bootstrap(scores_b, target, groups1, groups2, n_boot=n_boot, seed=seed, betas=betas, llr=llr)
    diff = BootstrapResult({n: ra.columns[n] - rb.columns[n] for n in ra.columns}, ra.totals, betas=ra.betas, seed=seed)
    ci = bootstrap_ci(diff, alpha=alpha, max_degenerate=max_degenerate)
    return diff, {n: (p, lo, hi, bool(lo > 0.0 or hi < 0.0)) for n, (p, lo, hi) in ci.items()}
