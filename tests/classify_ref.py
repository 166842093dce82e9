"""The numpy twin of the speaker-classification loss (csrc/nplda_classify.hip; include/nplda_hip.h has the definition) — a
plain helper of the classification tests.

    kind 0: u_ic = <x_i, w_c>;  kinds 1, 2: u_ic = <x^_i, w^_c>,  x^ = x / max(||x||, 1e-12)
    a_ic = s u_ic + b_c;  l_ic = a_ic (c != y_i),  l_iy = s phi(u_iy) + b_y
    phi: u (kind 0), u - m (kind 1); kind 2: v = clamp(u, -1, 1), sn = sqrt(max(1 - v^2, 2^-24)),
         v > -cos m: phi = v cos m - sn sin m, phi' = cos m + (v / sn) sin m; else phi = v - m sin m, phi' = 1
    V = {i: 0 <= y_i < C};  lse_i = log sum_c exp l_ic;  rowloss_i = lse_i - l_iy on V;  loss = sum_V rowloss / |V|
    pred_i = argmax_c a_ic (lowest index on ties);  counts = (|V|, #{i in V: pred_i = y_i}, #{y_i < -1 or y_i >= C})
    g = (softmax(l) - onehot(y)) / |V| on V, 0 elsewhere;  db = sum_i g_i;  h = s g, times phi' at the target
    kind 0: dX = H W, dW = H^T X;  kinds 1, 2: A = H W^, dX_i = (A_i - <x^_i, A_i> x^_i) / max(||x_i||, 1e-12), dW likewise

`dtype=np.float64` is the oracle, `dtype=np.float32` the same formulas with every array in float32 (the unit of
tests/fp32_units.py).  Every sum over features, classes or rows is a plain left-to-right sum in `dtype`, as
tests/allpairs_ref.py does and for its reason; `chunk=16` evaluates every such sum as left-to-right sums of 16 terms added
left to right (a second summation order, for the CPU test of the gates).  s, m, cos m, sin m and m sin m enter as the float32
values the device is handed."""
from collections import namedtuple

import numpy as np

from tests.allpairs_ref import _sum_over

Result = namedtuple("Result", "U a l lse rowloss loss pred counts dX dW db valid")

KINDS = {"softmax": 0, "am": 1, "aam": 2}
SCALE = {0: 0.05, 1: 30.0, 2: 30.0}
MARGIN = {0: 0.0, 1: 0.2, 2: 0.2}


def _sum(term, n, dtype, chunk=None):
    if chunk is None:
        return _sum_over(term, n, dtype)
    acc = None
    for k0 in range(0, n, chunk):
        part = _sum_over(lambda k: term(k0 + k), min(chunk, n - k0), dtype)  # noqa: B023
        acc = part if acc is None else (acc + part).astype(dtype)
    return acc


def consts(s, m, dtype):
    """(s, m, cos m, sin m, m sin m) as the float32 values of the C call, in `dtype`."""
    s32, m32 = np.float32(s), np.float32(m)
    md = np.float64(m32)
    return tuple(dtype(np.float32(v)) for v in (s32, m32, np.cos(md), np.sin(md), md * np.sin(md)))


def phi_of(u, kind, m, cm, sm, msm, dtype):
    """(phi, phi') of an array of target cosines / logits."""
    u = np.asarray(u, dtype)
    one = np.ones_like(u)
    if kind == 0:
        return u, one
    if kind == 1:
        return (u - m).astype(dtype), one
    v = np.clip(u, dtype(-1), dtype(1))
    sn = np.sqrt(np.maximum(dtype(1) - v * v, dtype(2.0 ** -24))).astype(dtype)
    inside = v > -cm
    phi = np.where(inside, v * cm - sn * sm, v - msm).astype(dtype)
    dphi = np.where(inside, cm + (v / sn) * sm, one).astype(dtype)
    return phi, dphi


def classify(X, y, W, b, kind, s, m, dtype=np.float64, chunk=None):
    """-> Result.  X (N, D), W (C, D), b (C) or None: float32 values; y (N) integers; kind 0 / 1 / 2."""
    X = np.asarray(X, np.float32).astype(dtype)
    W = np.asarray(W, np.float32).astype(dtype)
    y = np.asarray(y).astype(np.int64)
    N, D = X.shape
    C = W.shape[0]
    bv = np.zeros(C, dtype) if b is None else np.asarray(b, np.float32).astype(dtype)
    s, m, cm, sm, msm = consts(s, m, dtype)
    if kind == 0:
        Xh, Wh, nx, nw = X, W, np.ones(N, dtype), np.ones(C, dtype)
    else:
        nx = np.maximum(np.sqrt(_sum(lambda d: X[:, d] * X[:, d], D, dtype, chunk)), dtype(1e-12)).astype(dtype)
        nw = np.maximum(np.sqrt(_sum(lambda d: W[:, d] * W[:, d], D, dtype, chunk)), dtype(1e-12)).astype(dtype)
        Xh, Wh = (X / nx[:, None]).astype(dtype), (W / nw[:, None]).astype(dtype)
    U = _sum(lambda d: Xh[:, d, None] * Wh[None, :, d], D, dtype, chunk)
    a = (s * U + bv[None, :]).astype(dtype)
    valid = (y >= 0) & (y < C)
    rows = np.flatnonzero(valid)
    yv = y[rows]
    phi, dphi = phi_of(U[rows, yv], kind, m, cm, sm, msm, dtype)
    l = a.copy()
    l[rows, yv] = (s * phi + bv[yv]).astype(dtype)
    M = l.max(axis=1)
    lse = (M + np.log(_sum(lambda c: np.exp(l[:, c] - M), C, dtype, chunk))).astype(dtype)
    rowloss = np.zeros(N, dtype)
    rowloss[rows] = lse[rows] - l[rows, yv]
    V = rows.size
    loss = float(rowloss[rows].astype(np.float64).sum() / V) if V else float("nan")
    pred = a.argmax(axis=1)
    counts = np.array([V, int((pred[rows] == yv).sum()), int(((y < -1) | (y >= C)).sum())], np.int64)
    g = np.zeros((N, C), dtype)
    if V:
        p = np.exp(l[rows] - lse[rows, None]).astype(dtype)
        p[np.arange(V), yv] -= dtype(1)
        g[rows] = (p / dtype(V)).astype(dtype)
    db = _sum(lambda i: g[i], N, dtype, chunk)
    h = (s * g).astype(dtype)
    h[rows, yv] = (h[rows, yv] * dphi).astype(dtype)
    A = _sum(lambda c: h[:, c, None] * Wh[c][None, :], C, dtype, chunk)
    B = _sum(lambda i: h[i, :, None] * Xh[i][None, :], N, dtype, chunk)
    if kind == 0:
        dX, dW = A, B
    else:
        dX = ((A - _sum(lambda d: Xh[:, d] * A[:, d], D, dtype, chunk)[:, None] * Xh) / nx[:, None]).astype(dtype)
        dW = ((B - _sum(lambda d: Wh[:, d] * B[:, d], D, dtype, chunk)[:, None] * Wh) / nw[:, None]).astype(dtype)
    return Result(U, a, l, lse, rowloss, loss, pred, counts, dX, dW, db, valid)


def torch_loss(X, W, b, y, kind, s, m):
    """The literal composition on torch tensors (of any floating dtype, with autograd): F.normalize, F.linear, the margin
    on the target, F.cross_entropy(ignore_index=-1) -> (loss, u).  Labels are -1 or inside 0 .. C - 1."""
    import torch
    import torch.nn.functional as F
    s, m, cm, sm, msm = (float(v) for v in consts(s, m, np.float64))
    u = F.linear(F.normalize(X), F.normalize(W)) if kind else F.linear(X, W)
    rows = torch.nonzero(y >= 0).ravel()
    ut = u[rows, y[rows]]
    if kind == 1:
        phi = ut - m
    elif kind == 2:
        phi = torch.where(ut > -cm, ut * cm - torch.sqrt(1 - ut * ut) * sm, ut - msm)
    else:
        phi = ut
    logits = (s * u).index_put((rows, y[rows]), s * phi)
    if b is not None:
        logits = logits + b
    return F.cross_entropy(logits, y, ignore_index=-1), u


# ---- the inputs the CPU and GPU tests share ---------------------------------------------------------------------------------

# (N, C, D, class_chunks, row_chunks): the last one forces ragged last chunks at a small shape
SHAPES = [(1, 1, 150, 0, 0), (2, 3, 150, 0, 0), (65, 17, 150, 0, 0), (130, 257, 170, 0, 0), (100, 1000, 150, 0, 0),
          (257, 300, 192, 0, 0), (64, 64, 8, 0, 0), (70, 100, 150, 3, 2)]
GAP = 1e-4  # the float64 gap between the best and the second-best a_ic of every row, relative to max |a|


def draw(N, C, D, seed, bias=True, noise=1.5):
    """Class centroids plus noise: W ~ N(0, 1), x_i = w_{y_i} + noise N(0, 1) (target cosines about 0.55), small biases, one
    label of -1 where N > 4."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((C, D)).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int32)
    X = (W[y] + noise * rng.standard_normal((N, D))).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32) if bias else None
    if N > 4:
        y[N // 3] = -1
    return X, W, b, y


def gap_of(r):
    """min over rows of (best - second-best a_ic) / max |a| on a Result; inf with one class."""
    if r.a.shape[1] < 2:
        return float("inf")
    top = np.sort(r.a, axis=1)[:, -2:]
    return float((top[:, 1] - top[:, 0]).min() / np.abs(r.a).max())


_cases = {}


def case(N, C, D, kind, class_chunks=0, row_chunks=0):
    """Everything a test needs for one shape and kind, computed once: the inputs (the seed redrawn until the float64 twin's
    argmax is decided by more than GAP in every row) and the float64 and float32 twins."""
    key = (N, C, D, kind)
    if key not in _cases:
        s, m = SCALE[kind], MARGIN[kind]
        seed = 1000 * kind + N + C + D
        while True:
            X, W, b, y = draw(N, C, D, seed, bias=D != 8)
            r64 = classify(X, y, W, b, kind, s, m, np.float64)
            if gap_of(r64) > GAP:
                break
            seed += 7919
        r32 = classify(X, y, W, b, kind, s, m, np.float32)
        for arr in (X, W, y) + (() if b is None else (b,)):
            arr.setflags(write=False)
        _cases[key] = dict(X=X, W=W, b=b, y=y, kind=kind, s=s, m=m, r64=r64, r32=r32, seed=seed)
    return dict(_cases[key], class_chunks=class_chunks, row_chunks=row_chunks)


def cases():
    """(N, C, D, kind, class_chunks, row_chunks) of the GPU test: every shape under the three kinds."""
    for N, C, D, cc, rc in SHAPES:
        for kind in (0, 1, 2):
            yield (N, C, D, kind, cc, rc)


def rowloss_bound(r64):
    """Per row: 16 * 2^-24 * max(1, max_c |l_ic|), the absolute bound of rowloss for the cases with fewer than 64 rows."""
    return 16 * 2.0 ** -24 * np.maximum(1.0, np.abs(r64.l).max(axis=1))


def small_bounds(c):
    """Absolute bounds for a case with fewer than 64 rows, where a ratio of errors is a draw: (rowloss per row, {dX, dW, db}).
    A float32 logit carries an absolute error of a few 2^-24 max(1, max |l|) =: e, taken as 16 of them as for rowloss; that is
    the RELATIVE error of every softmax probability, so |dg_ic| <= e p_ic / |V| <= e / |V|.  Then
      db_c = sum_i g_ic:                      |V| terms                              e
      dX_id = s sum_c g_ic phi' w^_cd:        C terms                                e s max phi' C max |w^| / |V|
      dW_cd = s sum_i g_ic phi' x^_id:        |V| terms                              e s max phi' max |x^|
    and under kinds 1 and 2 the projection (A - <x^, A> x^) / ||x|| at most doubles a bound and divides it by the smallest norm.
    Bounds of the error's propagation, not measurements; the CPU test holds the float32 twin to a quarter of each."""
    r64, kind = c["r64"], c["kind"]
    X, W = c["X"].astype(np.float64), c["W"].astype(np.float64)
    nx, nw = np.linalg.norm(X, axis=1), np.linalg.norm(W, axis=1)
    xh = np.abs(X / nx[:, None]).max() if kind else np.abs(X).max()
    wh = np.abs(W / nw[:, None]).max() if kind else np.abs(W).max()
    s, m, cm, sm, msm = consts(c["s"], c["m"], np.float64)
    rows = np.flatnonzero(r64.valid)
    dphi = float(phi_of(r64.U[rows, c["y"][rows]], kind, m, cm, sm, msm, np.float64)[1].max()) if rows.size else 1.0
    e = 16 * 2.0 ** -24 * max(1.0, float(np.abs(r64.l).max()))
    V, C = max(rows.size, 1), W.shape[0]
    px, pw = (2.0 / nx.min(), 2.0 / nw.min()) if kind else (1.0, 1.0)
    return rowloss_bound(r64), {"db": e, "dX": e * s * dphi * C * wh / V * px, "dW": e * s * dphi * xh * pw}
