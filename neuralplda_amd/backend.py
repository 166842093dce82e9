"""Estimate the LDA and the PLDA initialisation of the models from x-vectors: what Kaldi's `ivector-mean`,
`ivector-compute-lda` and `ivector-compute-plda` write as `mean.vec`, `transform.mat` and `plda`
(design/k15_backend_estimation.md).

Where the work runs:
  * everything O(N) in the number of x-vectors is HIP: the class scatter (ops.class_scatter, csrc/nplda_scatter.hip:
    sum, sum of outer products and per-speaker sums in one call) and the LDA projection with unit-length normalisation
    (ops.embed_train, its `y` output);
  * everything O(speakers * D^2) — the between-class scatter from the speaker sums, the E-step of the PLDA — is torch
    float64 on the device the statistics live on;
  * everything O(D^3) on a single D x D matrix — the eigendecompositions and the Cholesky factor — is numpy float64 on the
    host (D <= 512: milliseconds), so the result does not depend on a device solver library.
"""
import collections
import math
import os
import sys
import warnings

import numpy as np
import torch

from . import kaldi_format

__all__ = ["read_spk2utt", "class_layout", "fit_lda", "fit_plda", "fit_backend", "Backend", "lda_from_stats", "plda_stats",
           "plda_em", "plda_output"]

PIVOT_SAMPLE = 4096  # rows averaged (float32, on the device) for the pivot the scatter kernel subtracts


# ---- speaker lists ------------------------------------------------------------------------------------------------

def read_spk2utt(path):
    """Kaldi `spk2utt` (`spk utt1 utt2 ...` per line) -> [(spk, [utt, ...]), ...] in file order."""
    out = []
    with open(path) as fh:
        for ln in fh:
            f = ln.split()
            if f:
                out.append((f[0], f[1:]))
    return out


def class_layout(table, spk2utt):
    """(rows, offs, speakers, missing) for an XvectorTable (anything with `row_of`) and a spk2utt (path, list of
    (spk, utts) or dict): `rows` int64 table rows grouped by speaker, `offs` int64 (S + 1) offsets into it, `speakers` the S
    names.  Utterances the table does not hold are skipped and returned in `missing` — the caller reports them — and a
    speaker left without any utterance is dropped."""
    if isinstance(spk2utt, (str, os.PathLike)):
        spk2utt = read_spk2utt(spk2utt)
    elif isinstance(spk2utt, dict):
        spk2utt = list(spk2utt.items())
    row_of = table.row_of
    rows, offs, speakers, missing = [], [0], [], []
    for spk, utts in spk2utt:
        n0 = len(rows)
        for u in utts:
            r = row_of.get(u)
            if r is None:
                missing.append(u)
            else:
                rows.append(r)
        if len(rows) > n0:
            speakers.append(spk)
            offs.append(len(rows))
    return np.asarray(rows, dtype=np.int64), np.asarray(offs, dtype=np.int64), speakers, missing


# ---- dense algebra (host, float64) --------------------------------------------------------------------------------

def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _sym(m):
    return 0.5 * (m + m.T)


def lda_from_stats(T, W, mean, lda_dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """Kaldi's ComputeLdaTransform on the total and within-class covariances (numpy float64, host):
    M = f T + (1 - f) W = U diag(e) U^T, e floored at max(e) * covariance_floor, P = diag(e^-1/2) U^T, the eigenvectors of
    P (T - W) P^T by descending eigenvalue, A = (first lda_dim)^T P, each row's largest-magnitude entry made positive.
    -> (transform (lda_dim, D + 1) = [A | -A mean], eigenvalues (D, descending), number of floored eigenvalues)."""
    T, W, mean = _sym(_np64(T)), _sym(_np64(W)), _np64(mean)
    D = T.shape[0]
    if not 0 < lda_dim <= D:
        raise ValueError(f"lda_dim must be in 1 .. {D}")
    f = float(total_covariance_factor)
    e, U = np.linalg.eigh(f * T + (1.0 - f) * W)
    floor = e.max() * covariance_floor
    nfloored = int((e < floor).sum())
    if nfloored:
        warnings.warn(f"LDA: floored {nfloored} of {D} eigenvalues of the within-class covariance at {floor:.3e}")
    P = U.T / np.sqrt(np.maximum(e, floor))[:, None]
    s, V = np.linalg.eigh(_sym(P @ (T - W) @ P.T))
    order = np.argsort(-s, kind="stable")
    s, V = s[order], V[:, order]
    A = V[:, :lda_dim].T @ P
    big = np.abs(A).argmax(axis=1)
    A = A * np.where(A[np.arange(lda_dim), big] < 0.0, -1.0, 1.0)[:, None]
    return np.concatenate([A, -(A @ mean)[:, None]], axis=1), s, nfloored


def plda_output(W, B, mu):
    """Kaldi's PldaEstimator::GetOutput (numpy float64, host): W = C C^T, T1 = C^-1, T1 B T1^T = U diag(psi) U^T, psi floored
    at 0 and sorted descending -> (mean, transform = U^T T1, psi)."""
    W, B = _sym(_np64(W)), _sym(_np64(B))
    T1 = np.linalg.inv(np.linalg.cholesky(W))
    psi, U = np.linalg.eigh(_sym(T1 @ B @ T1.T))
    order = np.argsort(-psi, kind="stable")
    psi, U = np.maximum(psi[order], 0.0), U[:, order]
    return _np64(mu).copy(), U.T @ T1, psi


# ---- PLDA (torch float64, on the device of its inputs) ------------------------------------------------------------

def plda_stats(scatter, class_sum, counts, pivot=None):
    """Kaldi's PldaStats with unit weights from the class scatter of the rows minus `pivot` (torch float64):
    -> (class means (S, D) [empty classes dropped], counts (S,), offset_scatter (D, D) = sum_s (sum_k y y^T - n_s m_s m_s^T))."""
    keep = counts > 0
    cs, n = class_sum[keep], counts[keep].to(torch.float64)
    half = cs / n.sqrt()[:, None]
    offset_scatter = scatter - half.T @ half
    means = cs / n[:, None]
    if pivot is not None:
        means = means + pivot.to(torch.float64)[None, :]
    return means, n, 0.5 * (offset_scatter + offset_scatter.T)


def plda_em(means, counts, offset_scatter, num_em_iters=10, init_scale=1.0):
    """Kaldi's PldaEstimator with unit weights (torch float64, any device) -> (W, B, mu), mu = the mean of the class means.
    From W = B = init_scale * I (Kaldi: I), per iteration and class with n rows and d = m - mu:
        V = (B^-1 + n W^-1)^-1,  w = V n W^-1 d,  between += V + w w^T,  within += n V + n (d - w)(d - w)^T
    on top of within = offset_scatter with count N - S; then W = within / N, B = between / S.
    Each iteration works in the basis Z that diagonalises W and B together (Z W Z^T = I, Z B Z^T = diag(psi): one Cholesky
    factor and one eigendecomposition of a D x D matrix, numpy on the host).  There V = diag(psi / (1 + n psi)) and
    V n W^-1 = diag(n psi / (1 + n psi)): no matrix is inverted per class (none at all: a zero psi is no special case), the
    E-step is elementwise on the S x D class means, and the two sums of outer products are two matrix products (torch, on
    the device of the inputs).  The result equals the literal per-class loop to float64 rounding."""
    means, counts = means.to(torch.float64), counts.to(torch.float64)
    dev = means.device
    S, D = means.shape
    N = counts.sum()
    mu = means.sum(0) / S
    d = means - mu
    n = counts[:, None]
    W = np.eye(D) * init_scale
    B = np.eye(D) * init_scale
    for _ in range(num_em_iters):
        T1 = np.linalg.inv(np.linalg.cholesky(_sym(W)))
        psi, U = np.linalg.eigh(_sym(T1 @ B @ T1.T))
        Z = torch.from_numpy(U.T @ T1).to(dev)
        Zinv = torch.from_numpy(np.linalg.inv(U.T @ T1)).to(dev)
        psi = torch.from_numpy(np.maximum(psi, 0.0)).to(dev)[None, :]
        dz = d @ Z.T
        v = psi / (1.0 + n * psi)          # diagonal of V per class (S, D)
        wz = dz * (n * v)
        rz = (dz - wz) * n.sqrt()
        between = torch.diag(v.sum(0)) + wz.T @ wz
        within = Z @ offset_scatter @ Z.T + torch.diag((n * v).sum(0)) + rz.T @ rz
        W = _sym(_np64(Zinv @ within @ Zinv.T / N))     # within_count = (N - S) + S
        B = _sym(_np64(Zinv @ between @ Zinv.T / S))
    return torch.from_numpy(W).to(dev), torch.from_numpy(B).to(dev), mu


# ---- estimators on device tables ----------------------------------------------------------------------------------

def _dev_i64(a, dev):
    if a is None:
        return None
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    return t.to(dev)


def _pivot_of(x, rows, N, n):
    """float32 mean of at most PIVOT_SAMPLE evenly spaced rows: an estimate of the mean for the kernel to subtract."""
    if N == 0:
        return None
    step = max(1, N // PIVOT_SAMPLE)
    pos = torch.arange(0, N, step, device=x.device)[:PIVOT_SAMPLE]
    idx = pos if rows is None else rows[pos]
    return x.index_select(0, idx)[:, :n].mean(0).contiguous()


def _scatter(x, rows, offs, n=None):
    """ops.class_scatter about a sampled pivot -> (pivot float64, sum, scatter, class_sum, counts) on x's device."""
    from . import ops
    dev = x.device
    rows, offs = _dev_i64(rows, dev), _dev_i64(offs, dev)
    n = x.shape[1] if n is None else n
    N = int(offs[-1])
    pivot = _pivot_of(x, rows, N, n)
    sm, sc, cs = ops.class_scatter(x, offs, rows=rows, pivot=pivot, n=n)
    counts = (offs[1:] - offs[:-1]).to(torch.float64)
    piv64 = torch.zeros(n, dtype=torch.float64, device=dev) if pivot is None else pivot.to(torch.float64)
    return piv64, sm, sc, cs, counts


def _lda_covariances(x, rows, offs):
    """(mean, T, W) of the rows, numpy float64: the kernel's pivoted statistics re-centred on the exact mean in float64
    (torch, device), the S x D -> D x D product of the class sums included."""
    piv, sm, sc, cs, counts = _scatter(x, rows, offs)
    N = float(counts.sum())
    if N <= 0:
        raise ValueError("no rows to estimate from")
    delta = sm / N
    tot = sc - N * torch.outer(delta, delta)
    keep = counts > 0
    half = (cs[keep] - counts[keep, None] * delta[None, :]) / counts[keep].sqrt()[:, None]
    between = half.T @ half
    return _np64(piv + delta), _np64(tot) / N, _np64(tot - between) / N


def fit_lda(x, rows, offs, lda_dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """Kaldi's ivector-compute-lda on the rows `x[rows]` (x: float32 device tensor (R, D0), D0 % 4 == 0, D0 <= 512; rows None:
    the first offs[-1] rows) with speaker s at positions offs[s] .. offs[s + 1].  With the rows centred by their mean,
    T = sum x x^T / N, W = (sum x x^T - sum_s sum_s sum_s^T / n_s) / N; see lda_from_stats.
    -> float64 numpy (lda_dim, D0 + 1) = [A | -A mean], the layout kaldi_format.fold_init consumes.
    The O(N) statistics are one HIP call; the re-centring is torch float64 on the device, the two eigendecompositions numpy
    on the host."""
    mean, T, W = _lda_covariances(x, rows, offs)
    return lda_from_stats(T, W, mean, lda_dim, total_covariance_factor, covariance_floor)[0]


def fit_plda(y, offs, num_em_iters=10, rows=None, dim=None, length_scale=1.0):
    """Kaldi's ivector-compute-plda (PldaStats + PldaEstimator, unit weights) on the rows of `y` (float32 device tensor; `dim`:
    the leading columns that count, default all; rows / offs as in fit_lda) -> (mean (D,), transform (D, D), psi (D,)) numpy
    float64.  length_scale c: the rows are taken as c * y by exact float64 rescaling of the statistics (means * c, scatter
    * c^2), and the EM then starts from W = B = c^2 I instead of I: every iterate is c^2 times the unit one, so the result is
    the unit estimate in the other geometry (transform / c, mean * c, the same psi) after any number of iterations, not only
    at the fixed point both starts share.
    The O(N) statistics are one HIP call, the EM torch float64 on the device, the output step numpy on the host."""
    D = y.shape[1] if dim is None else int(dim)
    n4 = (D + 3) // 4 * 4
    if n4 > y.shape[1]:
        raise ValueError(f"y needs {n4} columns (zero padding past {D})")
    piv, _, sc, cs, counts = _scatter(y, rows, offs, n4)
    means, n, off = plda_stats(sc[:D, :D], cs[:, :D], counts, piv[:D])
    c = float(length_scale)
    W, B, mu = plda_em(means * c, n, off * (c * c), num_em_iters, init_scale=c * c)
    return plda_output(W, B, mu)


# ---- the whole back end -------------------------------------------------------------------------------------------

class Backend(collections.namedtuple("Backend", "mean_vec transform_mat plda_mean plda_transform psi length_norm")):
    """What the Kaldi loaders of the models consume, as float64 numpy arrays: mean_vec (D0), transform_mat (lda_dim, D0 + 1),
    and — unless fitted with plda=False — plda_mean (lda_dim), plda_transform (plda_dim, lda_dim), psi (plda_dim)."""
    __slots__ = ()

    def save(self, out_dir):
        """mean.vec, transform.mat (float32, as Kaldi writes them) and plda (doubles) — readable by read_vector /
        read_matrix / read_plda and by Kaldi."""
        os.makedirs(out_dir, exist_ok=True)
        kaldi_format.write_vector_binary(os.path.join(out_dir, "mean.vec"), self.mean_vec)
        kaldi_format.write_matrix_binary(os.path.join(out_dir, "transform.mat"), self.transform_mat)
        if self.plda_transform is not None:
            kaldi_format.write_plda_binary(os.path.join(out_dir, "plda"), self.plda_mean, self.plda_transform, self.psi)
        return out_dir

    def model_plda(self):
        """(mean, transform, psi) in the geometry of the models, whose layer 2 sees UNIT-length rows: a "sqrt_dim" estimate is
        the unit one with transform / sqrt(D) and mean * sqrt(D), so it is scaled back (psi is the same)."""
        if self.plda_transform is None:
            return None
        if self.length_norm == "unit":
            return self.plda_mean, self.plda_transform, self.psi
        c = math.sqrt(self.transform_mat.shape[0])
        return self.plda_mean / c, self.plda_transform * c, self.psi

    def with_plda_dim(self, plda_dim):
        """The first plda_dim rows of the PLDA transform and entries of psi (the largest between-class variances)."""
        if not 0 < plda_dim <= self.plda_transform.shape[0]:
            raise ValueError(f"plda_dim must be in 1 .. {self.plda_transform.shape[0]}")
        return self._replace(plda_transform=self.plda_transform[:plda_dim], psi=self.psi[:plda_dim])

    def apply(self, model):
        """Fold the arrays into a model (NeuralPlda and subclasses: LDA + PLDA; DPlda / GaussianBackend: the LDA), through
        the code path of kaldi_format.fold_init.  mean_vec and transform_mat pass through float32, as the files do."""
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
        plda = self.model_plda() if hasattr(model, "centering_and_wccn_plda") else None
        if plda is None and hasattr(model, "centering_and_wccn_plda"):
            raise ValueError("this Backend was fitted without a PLDA")
        kaldi_format.fold_arrays(model, f32(self.mean_vec), f32(self.transform_mat), plda)
        return model


def _table_tensor(table, device):
    """Device matrix of an XvectorTable (`on()`), or of a plain tensor — which only `center` may be: the training table
    must also map utterance names to rows (`row_of`)."""
    if isinstance(table, torch.Tensor):
        return table if device is None else table.to(device)
    return table.on(device if device is not None else "cuda")


def _mean_of(x):
    """Mean of all rows of a device table through the scatter kernel (one class) -> numpy float64."""
    offs = torch.tensor([0, x.shape[0]], dtype=torch.int64)
    piv, sm, _, _, counts = _scatter(x, None, offs)
    return _np64(piv + sm / float(counts.sum()))


def fit_backend(table, spk2utt, lda_dim, plda_dim=None, length_norm="unit", center=None, plda=True,
                total_covariance_factor=0.0, covariance_floor=1e-6, num_em_iters=10, device=None):
    """mean.vec, transform.mat and plda from an XvectorTable (anything with `row_of` and `on(device)`) and a spk2utt (path,
    list or dict) -> Backend.

    As the Kaldi recipes do it: the LDA is estimated on the training rows minus their own mean, so transform_mat's offset
    column is -A times the mean of the CENTRED rows (zero up to rounding) whatever `center` is; the PLDA on
    y = normalise(A (x - training mean)).  mean_vec is the training mean, or with `center` (another XvectorTable or device
    tensor: in-domain data) the mean of that table.
    length_norm: "unit" (default) — rows of length 1, what the models' own F.normalize feeds layer 2, so a NeuralPlda
    initialised from the result scores the PLDA log-likelihood ratio of its own geometry; "sqrt_dim" — Kaldi's
    ivector-normalize-length (length sqrt(lda_dim)), by exact float64 rescaling of the unit statistics.
    plda_dim < lda_dim keeps the first plda_dim rows of the PLDA transform and entries of psi (the largest).
    plda=False stops after the LDA (DPlda, GaussianBackend).
    Utterances of spk2utt that the table lacks are listed on stderr.  Runs on `device` (default: the current HIP device); see
    the module docstring for what runs where."""
    from . import ops
    if length_norm not in ("unit", "sqrt_dim"):
        raise ValueError("length_norm must be 'unit' or 'sqrt_dim'")
    plda_dim = lda_dim if plda_dim is None else int(plda_dim)
    if not 0 < plda_dim <= lda_dim:
        raise ValueError("plda_dim must be in 1 .. lda_dim")
    rows, offs, speakers, missing = class_layout(table, spk2utt)
    if missing:
        print(f"fit_backend: {len(missing)} utterances of spk2utt are not in the table: {' '.join(missing[:20])}"
              f"{' ...' if len(missing) > 20 else ''}", file=sys.stderr)
    if len(speakers) == 0:
        raise ValueError("no speaker of spk2utt has an utterance in the table")
    x = _table_tensor(table, device)
    dev = x.device
    D0 = x.shape[1]
    rows_d, offs_d = _dev_i64(rows, dev), _dev_i64(offs, dev)
    mean, T, W = _lda_covariances(x, rows_d, offs_d)
    # the LDA of the rows minus `mean`: their mean is zero
    tm, _, _ = lda_from_stats(T, W, np.zeros(D0), lda_dim, total_covariance_factor, covariance_floor)
    tm[:, -1] = 0.0
    mean_vec = mean if center is None else _mean_of(_table_tensor(center, dev))
    if not plda:
        return Backend(mean_vec, tm, None, None, None, length_norm)
    # y = normalise(A (x - mean)) for every table row (HIP: layer 1 + unit-length normalisation of the scoring model; its
    # layer 2 is given an identity and ignored), then the class scatter of the speakers' rows of y
    A = torch.from_numpy(tm[:, :-1]).to(dev, torch.float32).contiguous()
    b = torch.from_numpy(-(tm[:, :-1] @ mean)).to(dev, torch.float32)
    zeros, ones = torch.zeros(lda_dim, device=dev), torch.ones(lda_dim, device=dev)
    packed = ops.pack_params(A, b, torch.eye(lda_dim, device=dev), zeros, ones, ones)
    _, (_, _, y, _) = ops.embed_train(x, packed)
    c = 1.0 if length_norm == "unit" else math.sqrt(lda_dim)
    pm, pt, psi = fit_plda(y, offs_d, num_em_iters, rows=rows_d, dim=lda_dim, length_scale=c)
    return Backend(mean_vec, tm, pm, pt, psi, length_norm).with_plda_dim(plda_dim)
