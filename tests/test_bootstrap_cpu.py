"""Group bootstrap without a GPU: the generator and the yardstick of the GPU tests (tests/bootstrap_ref.py) against the
existing exact metrics on np.repeat-expanded trial lists, the declared ABI, the workspace size, every status code of
nplda_bootstrap_f32 (returned before anything is enqueued: no valid call is made) and bootstrap_ci on a hand-made result."""
import ctypes
import os
import re

import numpy as np
import pytest

from neuralplda_amd import _lib
from oracle import nplda_oracle as orc

from tests import bootstrap_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENOSPC = -22, -95, -28
NAMES = ["nplda_bootstrap_workspace_bytes", "nplda_bootstrap_run", "nplda_bootstrap_tile", "nplda_bootstrap_f32"]


# ---- the generator ------------------------------------------------------------------------------------------------------
def test_splitmix64_known_answer():
    assert int(br.mix(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF  # first output of splitmix64 seeded 0
    assert int(br.mix(np.array([0], dtype=np.uint64))[0]) == 0


@pytest.mark.parametrize("G", [1, 2, 7, 2 ** 20])
def test_draws_lie_in_range_and_counts_sum_to_G(G):
    for seed, b, side in ((0, 1, 0), (0, 1, 1), (12345678901234567890, 77, 0), (2 ** 64 - 1, 1000, 1)):
        d = br.draws(seed, b, side, G)
        assert d.shape == (G,) and d.min() >= 0 and d.max() < G
        c = br.counts(seed, b, side, G)
        assert c.shape == (G,) and int(c.sum()) == G
    assert np.array_equal(br.counts(5, 0, 0, G), np.ones(G, dtype=np.int64))  # replicate 0: the point estimate
    if G >= 7:  # sides, replicates and seeds give different draws
        a = br.draws(0, 1, 0, G)
        assert not np.array_equal(a, br.draws(0, 1, 1, G)) and not np.array_equal(a, br.draws(0, 2, 0, G))
        assert not np.array_equal(a, br.draws(1, 1, 0, G))
    if G == 2 ** 20:  # a multinomial: about a share 1/e of the groups is not drawn
        assert abs((br.counts(3, 9, 0, G) == 0).mean() - np.exp(-1)) < 5e-3


# ---- the twin against the existing metrics on the expanded list ------------------------------------------------------------
def _expanded(scores, target, w):
    s, y = np.asarray(scores, dtype=np.float32), np.asarray(target, dtype=np.float32)
    w = np.where(np.isnan(s), 0, w)
    return np.repeat(s, w), np.repeat(y, w)


def _check_row(scores, target, w, betas):
    order, key, code, start = br.sort_trials(scores, target)
    row, Nt, Nn = br.sweep(key, code, start, np.asarray(w)[order], betas)
    se, ye = _expanded(scores, target, np.asarray(w))
    assert Nt == int((ye > 0.5).sum()) and Nn == int((ye < 0.5).sum())
    if Nt == 0 or Nn == 0:
        assert np.isnan(row).all()
        return False
    for k, b in enumerate(betas):
        assert row[k] == orc.minc_exact(se, ye, [b])[0], (k, b)
    assert row[len(betas)] == orc.eer(se, ye)
    return True


@pytest.mark.parametrize("seed", range(30))
def test_twin_equals_the_exact_metrics_on_the_expanded_list(seed):
    rg = np.random.default_rng(seed)
    N = int(rg.integers(2, 40))
    G1, G2 = int(rg.integers(1, 6)), int(rg.integers(1, 5))
    # heavy ties.  No +inf: the oracle merges the accept-nothing point with a score of +inf, the kernels (like
    # nplda_detcost_sweep_f32) keep it apart (design/k20_bootstrap.md)
    s = rg.choice(np.array([-2.0, -0.5, -0.0, 0.0, 1.0, 3.5, 1e30, -np.inf]), size=N)
    y = (rg.random(N) < 0.4).astype(np.float64)
    y[rg.random(N) < 0.1] = 0.5
    s[rg.random(N) < 0.1] = np.nan
    g1, g2 = rg.integers(0, G1, N), rg.integers(0, G2, N)
    betas = [1.0, 9.0, 0.25]
    live = 0
    for b in range(6):
        w = br.counts(seed, b, 0, G1)[g1] * (br.counts(seed, b, 1, G2)[g2] if seed % 3 else 1)
        live += _check_row(s, y, w, betas)
    out, totals = br.bootstrap(s, y, g1, G1, g2 if seed % 3 else None, G2 if seed % 3 else 0, n_boot=5, seed=seed, betas=betas)
    assert int(np.isfinite(out).all(axis=1).sum()) == live and out.shape == (6, 4) and totals.shape == (6, 2)


def test_twin_on_cases_done_by_hand():
    # a zero-weight position (score 2) between the crossing (score 3) and its predecessor (score 1)
    s = [0.0, 1.0, 2.0, 3.0, 4.0]
    y = [0, 1, 0, 0, 1]
    assert _check_row(s, y, [1, 1, 0, 1, 1], [1.0, 5.0])
    assert _check_row(s, y, [2, 1, 0, 3, 1], [1.0, 5.0])
    # zero-weight trials at both ends, a zero-weight start of a tie run, an excluded label as a threshold
    assert _check_row([0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 9.0], [1, 0, 1, 0.5, 0, 1, 0], [0, 0, 2, 1, 3, 1, 0], [1.0, 2.0])
    # no crossing in the expanded list; the zero-weight trial above it must not create one: EER (0 + 1) / 2
    order, key, code, start = br.sort_trials([0.0, 1.0, 1.0, 2.0], [0, 1, 0, 1])
    row, Nt, Nn = br.sweep(key, code, start, np.array([1, 1, 1, 0]), [1.0])
    assert (Nt, Nn) == (1, 2) and row[1] == 0.5
    assert _check_row([0.0, 1.0, 1.0, 2.0], [0, 1, 0, 1], [1, 1, 1, 0], [1.0])
    # a degenerate replicate
    assert not _check_row([0.0, 1.0], [0, 1], [3, 0], [1.0])
    # actual cost and Cllr of the twin against direct formulas
    s, y, w = np.array([-1.0, 0.5, 2.0, 3.0], dtype=np.float32), np.array([0, 1, 0, 1]), np.array([2, 1, 1, 3])
    order, key, code, start = br.sort_trials(s, y)
    row, Nt, Nn = br.sweep(key, code, start, w, [2.0], llr=True, sp=br.softplus_terms(key, code))
    th = np.log(2.0)
    assert row[2] == (1 * (0.5 < th)) / 4 + 2.0 * ((1 * (2.0 >= th)) / 3)
    want = 0.5 * ((np.log2(1 + np.exp(-0.5)) + 3 * np.log2(1 + np.exp(-3.0))) / 4 +
                  (2 * np.log2(1 + np.exp(-1.0)) + np.log2(1 + np.exp(2.0))) / 3)
    assert abs(row[3] - want) <= 1e-15


# ---- the library --------------------------------------------------------------------------------------------------------
def test_declared_names(hip_lib):
    assert hip_lib.nplda_abi_version() == 4
    with open(os.path.join(ROOT, "include", "nplda_hip.h")) as fh:
        hdr = fh.read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None, name
    from neuralplda_amd import metrics, ops
    for mod, fns in ((ops, ("bootstrap_metrics", "bootstrap_run", "bootstrap_tile")),
                     (metrics, ("bootstrap", "bootstrap_ci", "bootstrap_diff", "BootstrapResult"))):
        for fn in fns:
            assert callable(getattr(mod, fn)), fn
    assert hip_lib.nplda_bootstrap_run() >= 2 and hip_lib.nplda_bootstrap_tile() >= 2


def test_workspace_bytes(hip_lib):
    f = hip_lib.nplda_bootstrap_workspace_bytes
    R, T = hip_lib.nplda_bootstrap_run(), hip_lib.nplda_bootstrap_tile()
    ns = sorted({2, 3, R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 1 << 20, 10_000_000, 2 ** 31 - 1})
    sizes = [f(n, 50, 7, 100) for n in ns]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    for bad in ((1, 5, 5, 10), (0, 5, 5, 10), (-4, 5, 5, 10), (2 ** 31, 5, 5, 10), (100, 0, 5, 10), (100, 5, -1, 10),
                (100, 2 ** 20 + 1, 0, 10), (100, 5, 2 ** 20 + 1, 10), (100, 5, 5, 0), (100, 5, 5, 2 ** 20 + 1)):
        assert f(*bad) == 0, bad
    assert f(100, 5, 0, 10) > 0
    # the size the issue names is supported
    big = f(10_000_000, 10_000, 10_000, 1000)
    assert 0 < big < 2 ** 31
    # no N x B or G x B term: beyond one tile the replicates reuse the same tables and partials
    for n, g in ((100_000, 1000), (10_000_000, 10_000)):
        assert f(n, g, g, 4 * T) == f(n, g, g, 8 * T) == f(n, g, g, 1000 * T)
        assert f(n, g, g, 1) <= f(n, g, g, 4 * T)


def test_status_codes(hip_lib):
    buf = np.zeros(1 << 16, dtype=np.float64)
    a = buf.ctypes.data
    N, G1, G2, B = 100, 7, 5, 10
    ws = hip_lib.nplda_bootstrap_workspace_bytes(N, G1, G2, B)
    assert ws > 0
    good = (ctypes.c_double * 8)(*([2.0] * 8))
    as_betas = lambda *v: (ctypes.c_double * len(v))(*v)  # noqa: E731

    def call(s=a, t=a, g1=a, g2=a, N=N, G1=G1, G2=G2, B=B, seed=1, betas=good, K=2, llr=1, out=a, tot=a, w=a, wb=ws):
        return hip_lib.nplda_bootstrap_f32(s, t, g1, g2, N, G1, G2, B, seed, betas, K, llr, out, tot, w, wb, None)

    for name in ("s", "t", "g1", "g2", "betas", "out", "tot", "w"):
        assert call(**{name: None}) == EINVAL, name
    assert call(g2=None, G2=0, wb=0) == ENOSPC  # g2 may be absent when G2 is 0: the next check is reached
    assert call(G2=0) == EINVAL  # g2 given, G2 = 0
    assert call(N=1) == EINVAL and call(N=0) == EINVAL and call(N=-3) == EINVAL
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL and call(G1=0) == EINVAL and call(G2=-1) == EINVAL
    assert call(K=0) == EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(betas=as_betas(2.0, bad)) == EINVAL, bad
    for name in ("out", "tot"):
        assert call(**{name: a + 4}) == EINVAL, name  # not aligned to 8 bytes
    for name in ("s", "t", "g1", "g2"):
        assert call(**{name: a + 2}) == EINVAL, name
    assert call(w=a + 8) == EINVAL
    assert call(N=2 ** 31) == EUNSUPPORTED and call(G1=2 ** 20 + 1) == EUNSUPPORTED and call(G2=2 ** 20 + 1) == EUNSUPPORTED
    assert call(B=2 ** 20 + 1) == EUNSUPPORTED and call(K=9) == EUNSUPPORTED
    assert call(wb=ws - 1) == ENOSPC and call(wb=0) == ENOSPC


# ---- intervals ----------------------------------------------------------------------------------------------------------
def test_bootstrap_ci_on_a_hand_made_result():
    from neuralplda_amd import metrics
    rg = np.random.default_rng(0)
    B = 200
    eer = np.concatenate(([0.05], 0.05 + 0.01 * rg.standard_normal(B)))
    cost = np.concatenate(([0.4], 0.4 + 0.05 * rg.standard_normal(B)))
    totals = np.stack([np.full(B + 1, 10), np.full(B + 1, 90)], axis=1)
    res = metrics.BootstrapResult({"eer": eer, "min_cost_99": cost}, totals, betas=(99.0,))
    assert res.n_boot == B and res.n_degenerate == 0
    ci = metrics.bootstrap_ci(res, alpha=0.1)
    assert set(ci) == {"eer", "min_cost_99"}
    for name, v in (("eer", eer), ("min_cost_99", cost)):
        lo, hi = np.quantile(v[1:], [0.05, 0.95])
        assert ci[name] == (v[0], lo, hi)
    assert metrics.bootstrap_ci(res)["eer"][1:] == tuple(np.quantile(eer[1:], [0.025, 0.975]))
    # NaN rows are dropped, within the allowed share
    bad = [3, 17, 101]
    eer2, cost2 = eer.copy(), cost.copy()
    eer2[bad] = np.nan
    cost2[bad] = np.nan
    totals2 = totals.copy()
    totals2[bad, 0] = 0
    res2 = metrics.BootstrapResult({"eer": eer2, "min_cost_99": cost2}, totals2)
    assert res2.n_degenerate == 3 and np.flatnonzero(res2.degenerate).tolist() == [b - 1 for b in bad]
    keep = np.ones(B + 1, dtype=bool)
    keep[[0] + bad] = False
    ci2 = metrics.bootstrap_ci(res2)
    assert ci2["eer"] == (eer[0],) + tuple(np.quantile(eer[keep], [0.025, 0.975]))
    assert metrics.bootstrap_ci(res2, max_degenerate=0.02)["min_cost_99"] == ci2["min_cost_99"]
    with pytest.raises(ValueError):
        metrics.bootstrap_ci(res2, max_degenerate=0.01)  # 3 of 200 is more than 1 %
    with pytest.raises(ValueError):
        metrics.bootstrap_ci(res2, max_degenerate=0.0)
    with pytest.raises(ValueError):
        metrics.bootstrap_ci(res, alpha=0.0)
    with pytest.raises(ValueError):
        metrics.BootstrapResult({"eer": eer}, totals[:-1])
