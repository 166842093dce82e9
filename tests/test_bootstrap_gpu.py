"""Group bootstrap on the GPU (csrc/nplda_bootstrap.hip) against tests/bootstrap_ref.py, the numpy twin written from
design/k20_bootstrap.md, and row 0 against the existing point metrics.

Tolerances are derived, not measured.  Totals are integers: equal.  Cost, EER and act_cost columns: 1e-12 relative — the
kernel compares candidates on un-normalised integer products and divides once, a handful of fp64 roundings, while the
smallest real error, one unit of weight in a rate, is at least 1 / (65 025 * 20 000) = 8e-10 at these sizes.  Cllr:
2 N 2^-52 relative, the bound of any summation order of N positive terms.  Row 0 against metrics.*: 1e-6, the existing
entry points return float32 (values at most 1) or sum in another order.
Sizes straddle R = nplda_bootstrap_run() (through 64 R) and T = nplda_bootstrap_tile()."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bootstrap_ref as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def make(N, G1, G2, tied, seed=0):
    """(scores fp32, labels, g1, g2 or None) in a shuffled order.  Every (g1, g2) combination holds a target and a
    non-target (so that no replicate can be degenerate) when N >= 2 G1 max(G2, 1); a few labels are 0.5 and a few scores
    NaN among the other trials."""
    rg = np.random.default_rng(7919 * seed + N + 31 * G1 + G2)
    g2n = max(G2, 1)
    i = np.arange(N)
    fixed = 2 * G1 * g2n if N >= 2 * G1 * g2n else 0
    y = (rg.random(N) < 0.3).astype(np.float64)
    g1, g2 = rg.integers(0, G1, N), rg.integers(0, g2n, N)
    if G1 == N:
        g1 = rg.permutation(N)
    y[:fixed] = i[:fixed] % 2
    g1[:fixed] = (i[:fixed] // 2) % G1
    g2[:fixed] = (i[:fixed] // 2) // G1
    s = (rg.standard_normal(N) + 1.5 * y).astype(np.float32)
    if tied:
        s = np.round(s, 1).astype(np.float32)
    if N > fixed + 20:
        free = fixed + rg.permutation(N - fixed)
        y[free[:5]] = 0.5
        s[free[5:9]] = np.nan
        s[free[9]], y[free[9]] = -np.inf, 0.0  # on a non-target: its Cllr term is 0, not infinite
    p = rg.permutation(N)
    return s[p], y[p], g1[p].astype(np.int32), (g2[p].astype(np.int32) if G2 else None)


def run(s, y, g1, G1, g2, G2, B, seed, betas, llr):
    from neuralplda_amd import ops
    out, totals, flags = ops.bootstrap_metrics(_dev(s), _dev(y, torch.float32), _dev(g1), G1, None if g2 is None else _dev(g2),
                                               G2, n_boot=B, seed=seed, betas=betas, llr=llr)
    torch.cuda.synchronize()
    return out.cpu().numpy(), totals.cpu().numpy(), flags.tolist()


def compare(got, want, N, K, llr):
    """The columns of `got` against the twin's `want` at the tolerances of the module docstring."""
    assert got.shape == want.shape
    nc = 2 * K + 1 if llr else K + 1  # cost, EER and act_cost columns
    err = np.abs(got[:, :nc] - want[:, :nc])
    with np.errstate(invalid="ignore", divide="ignore"):
        print("max relative error of the cost / EER / act_cost columns:", float(np.nanmax(err / np.abs(want[:, :nc]))))
    assert (err <= 1e-12 * np.abs(want[:, :nc])).all()
    if llr:
        e = np.abs(got[:, -1] - want[:, -1]) / want[:, -1]
        print("max relative error of Cllr:", float(e.max()), "bound", 2 * N * 2.0 ** -52)
        assert (e <= 2 * N * 2.0 ** -52).all()


BETAS = {1: [99.0], 2: [99.0, 199.0], 8: [0.25, 1.0, 2.0, 9.0, 19.0, 99.0, 199.0, 999.0]}


def _cases():
    from neuralplda_amd import _lib
    lib = _lib.load()
    R, T = lib.nplda_bootstrap_run(), lib.nplda_bootstrap_tile()
    return [  # N, B, G1, G2, K, llr, tied
        (2, 1, 1, 1, 1, True, False),
        (R + 1, 1, 7, 5, 2, True, True),
        (64 * R - 1, T - 1, 7, 5, 2, True, False),
        (64 * R, T, 50, 0, 8, True, True),
        (64 * R + 1, T + 1, 64 * R + 1, 0, 1, False, False),
        (20000, 200, 7, 5, 2, True, True),
        (20011, 200, 50, 0, 8, False, False),
        (19999, T, 19999, 0, 2, True, True),
    ]


@pytest.mark.parametrize("case", range(8))
def test_replicates_against_the_twin(case):
    N, B, G1, G2, K, llr, tied = _cases()[case]
    if N == 2:
        s, y = np.array([0.25, -1.0], dtype=np.float32), np.array([1.0, 0.0])
        g1, g2 = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    else:
        s, y, g1, g2 = make(N, G1, G2, tied, seed=case)
    seed = 1000 + case
    want, wtot = br.bootstrap(s, y, g1, G1, g2, G2, n_boot=B, seed=seed, betas=BETAS[K], llr=llr)
    assert np.isfinite(want).all() and (wtot > 0).all()  # no degenerate replicate, by construction
    got, gtot, flags = run(s, y, g1, G1, g2, G2, B, seed, BETAS[K], llr)
    assert flags == [0, 0]
    assert np.array_equal(gtot, wtot)
    compare(got, want, N, K, llr)


@pytest.mark.parametrize("tied", [False, True])
def test_point_estimate_is_the_existing_metrics(tied):
    from neuralplda_amd import metrics
    s, y, g1, g2 = make(5000, 7, 5, tied, seed=3)
    betas = [99.0, 199.0, 1.0]
    res = metrics.bootstrap(s, y, g1, g2, n_boot=3, seed=5, betas=betas, llr=True)
    S, Y = _dev(s), _dev(y, torch.float32)
    keep = ~torch.isnan(S)  # metrics.minc_exact / eer / cllr have no NaN rule of their own
    S, Y = S[keep], Y[keep]
    for b in betas:
        assert abs(res[f"min_cost_{b:g}"][0] - float(metrics.minc_exact(S, Y, [b])[0])) <= 1e-6, b
    assert abs(res["eer"][0] - metrics.eer(S, Y)) <= 1e-6
    act = metrics.act_cost(S, Y, betas)[1]
    for b in betas:
        assert abs(res[f"act_cost_{b:g}"][0] - act[b]) <= 1e-6, b
    assert abs(res["cllr"][0] - metrics.cllr(S, Y)) <= 1e-6
    valid = ~np.isnan(s)
    assert res.totals[0].tolist() == [int(((y > 0.5) & valid).sum()), int(((y < 0.5) & valid).sum())]
    assert res.n_degenerate == 0


def test_degenerate_replicates():
    from neuralplda_amd import metrics
    rg = np.random.default_rng(11)
    N, B, seed = 400, 64, 21
    g1 = (np.arange(N) % 2).astype(np.int32)
    y = ((g1 == 0) & (rg.random(N) < 0.5)).astype(np.float64)  # every target sits in group 0
    s = (rg.standard_normal(N) + 1.5 * y).astype(np.float32)
    want, wtot = br.bootstrap(s, y, g1, 2, n_boot=B, seed=seed, betas=[9.0], llr=True)
    both_1 = np.array([b > 0 and br.counts(seed, b, 0, 2)[0] == 0 for b in range(B + 1)])
    assert np.array_equal(np.isnan(want).all(axis=1), both_1) and 5 < both_1.sum() < B - 5
    got, gtot, flags = run(s, y, g1, 2, None, 0, B, seed, [9.0], True)
    assert np.array_equal(np.isnan(got), np.isnan(want))  # the NaN rows are exactly the twin's, whole rows
    assert np.array_equal(gtot, wtot) and (gtot[both_1, 0] == 0).all() and (gtot[~both_1] > 0).all()
    compare(got[~both_1], want[~both_1], N, 1, True)
    res = metrics.bootstrap(s, y, g1, None, n_boot=B, seed=seed, betas=[9.0], llr=True)
    assert res.n_degenerate == int(both_1.sum())
    with pytest.raises(ValueError):
        metrics.bootstrap_ci(res, max_degenerate=0)
    ci = metrics.bootstrap_ci(res, alpha=0.1, max_degenerate=1.0)
    for j, name in enumerate(["min_cost_9", "eer", "act_cost_9", "cllr"]):
        lo, hi = np.quantile(want[1:][~both_1[1:], j], [0.05, 0.95])
        tol = 2 * N * 2.0 ** -52 if name == "cllr" else 1e-12
        assert abs(ci[name][0] - want[0, j]) <= tol * want[0, j]
        assert abs(ci[name][1] - lo) <= tol * lo and abs(ci[name][2] - hi) <= tol * hi, name


def test_determinism_and_order_independence():
    N, G1, G2, B, K = 20000, 7, 5, 70, 2
    s, y, g1, g2 = make(N, G1, G2, True, seed=9)
    a = run(s, y, g1, G1, g2, G2, B, 42, BETAS[K], True)
    b = run(s, y, g1, G1, g2, G2, B, 42, BETAS[K], True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = run(s, y, g1, G1, g2, G2, B, 43, BETAS[K], True)
    assert np.array_equal(c[0][0], a[0][0]) and not np.array_equal(c[0][1:], a[0][1:])  # row 0 has no draws
    p = np.random.default_rng(5).permutation(N)
    d = run(s[p], y[p], g1[p], G1, g2[p], G2, B, 42, BETAS[K], True)
    assert d[1].tobytes() == a[1].tobytes()
    assert d[0][:, :2 * K + 1].tobytes() == a[0][:, :2 * K + 1].tobytes()  # integer counts only
    assert (np.abs(d[0][:, -1] - a[0][:, -1]) <= 2 * N * 2.0 ** -52 * a[0][:, -1]).all()


def test_capturable():
    """A call captured in a graph (one stream, no branches) and replayed twice gives the eager bits."""
    from neuralplda_amd import ops
    N, G1, G2, B, K = 3000, 7, 5, 70, 2
    s, y, g1, g2 = make(N, G1, G2, False, seed=2)
    eager = run(s, y, g1, G1, g2, G2, B, 8, BETAS[K], True)
    S, Y, A, C = _dev(s), _dev(y, torch.float32), _dev(g1), _dev(g2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, totals, flags = ops.bootstrap_metrics(S, Y, A, G1, C, G2, n_boot=B, seed=8, betas=BETAS[K], llr=True)
    for _ in range(2):
        out.zero_()
        totals.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == eager[0].tobytes() and totals.cpu().numpy().tobytes() == eager[1].tobytes()
        assert flags.tolist() == [0, 0]


def test_group_ids_out_of_range_are_counted_not_used():
    from neuralplda_amd import metrics, ops
    s, y, g1, g2 = make(1000, 7, 5, False, seed=4)
    g1b, g2b = g1.copy(), g2.copy()
    g1b[[3, 500]] = [7, -1]
    g2b[[9]] = [1 << 30]
    got, gtot, flags = run(s, y, g1b, 7, g2b, 5, 5, 1, [9.0], False)
    assert flags == [3, 0]
    drop = np.zeros(1000, dtype=bool)
    drop[[3, 500, 9]] = True
    s2 = np.where(drop, np.float32(np.nan), s)  # an excluded trial: the twin's NaN rule
    want, wtot = br.bootstrap(s2, y, np.where(drop, 0, g1b), 7, np.where(drop, 0, g2b), 5, n_boot=5, seed=1, betas=[9.0])
    assert np.array_equal(gtot, wtot)
    compare(got, want, 1000, 1, False)
    with pytest.raises(ValueError):
        metrics.bootstrap(s, y, g1b, g2, n_boot=5)  # a negative id
    names = np.array(["spk%03d" % g for g in g1])
    r1 = metrics.bootstrap(s, y, names, g2, n_boot=5, seed=3, betas=[9.0])  # ids as strings: np.unique keeps the order
    r2 = metrics.bootstrap(s, y, g1, g2, n_boot=5, seed=3, betas=[9.0])
    assert r1["eer"].tobytes() == r2["eer"].tobytes() and np.array_equal(r1.totals, r2.totals)
    r3 = metrics.bootstrap(s, y, None, n_boot=5, seed=3, betas=[9.0])  # trial-level resampling
    want3, _ = br.bootstrap(s, y, np.arange(1000), 1000, n_boot=5, seed=3, betas=[9.0])
    assert np.isfinite(want3).all() and (np.abs(r3["eer"] - want3[:, 1]) <= 1e-12 * want3[:, 1]).all()
    assert ops.bootstrap_run() >= 2 and ops.bootstrap_tile() >= 2


def test_bootstrap_diff():
    from neuralplda_amd import metrics
    N, G1, G2, B = 5000, 7, 5, 40
    s, y, g1, g2 = make(N, G1, G2, False, seed=6)
    betas = [99.0, 9.0]
    diff, ci = metrics.bootstrap_diff(s, s.copy(), y, g1, g2, n_boot=B, seed=4, betas=betas, llr=True)
    for name, v in diff.columns.items():
        assert (v == 0.0).all(), name
        assert ci[name] == (0.0, 0.0, 0.0, False)
    s2 = s.copy()
    idx = np.flatnonzero(~np.isnan(s))[:200]
    s2[idx] += np.random.default_rng(1).standard_normal(200).astype(np.float32)
    diff, ci = metrics.bootstrap_diff(s, s2, y, g1, g2, n_boot=B, seed=4, betas=betas, llr=True)
    wa, _ = br.bootstrap(s, y, g1, G1, g2, G2, n_boot=B, seed=4, betas=betas, llr=True)
    wb, _ = br.bootstrap(s2, y, g1, G1, g2, G2, n_boot=B, seed=4, betas=betas, llr=True)
    assert np.isfinite(wa).all() and np.isfinite(wb).all()
    names = ["min_cost_99", "min_cost_9", "eer", "act_cost_99", "act_cost_9", "cllr"]
    assert list(diff.columns) == names
    for j, name in enumerate(names):  # each side within its own tolerance of the twin
        tol = 2 * N * 2.0 ** -52 if name == "cllr" else 1e-12
        assert (np.abs(diff[name] - (wa[:, j] - wb[:, j])) <= tol * (np.abs(wa[:, j]) + np.abs(wb[:, j]))).all(), name
        p, lo, hi, excl = ci[name]
        assert lo <= hi and excl == (lo > 0 or hi < 0)
    assert any(np.abs(v).max() > 0 for v in diff.columns.values())


def test_eval_scores_tool(tmp_path):
    rg = np.random.default_rng(3)
    N = 300
    enr = ["m%02d" % (i % 20) for i in range(N)]
    tst = ["u%03d" % (i % 60) for i in range(N)]
    y = (rg.random(N) < 0.4).astype(int)
    s = rg.standard_normal(N) + 2.0 * y
    with open(tmp_path / "key.txt", "w") as fh:
        fh.write("enrol test x label\n")
        for e, t, l in zip(enr, tst, y):
            fh.write(f"{e} {t} x {'target' if l else 'nontarget'}\n")
    for name, noise in (("a.txt", 0.0), ("b.txt", 0.7)):
        with open(tmp_path / name, "w") as fh:
            fh.write("enrol test score\n")
            for e, t, v in zip(enr, tst, s + noise * rg.standard_normal(N)):
                fh.write(f"{e} {t} {v:.6f}\n")
    with open(tmp_path / "m1.txt", "w") as fh:
        for i in range(20):
            fh.write(f"m{i:02d} spk{i % 10}\n")
    with open(tmp_path / "m2.txt", "w") as fh:
        for i in range(60):
            fh.write(f"u{i:03d} spk{i % 15}\n")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_scores.py"), str(tmp_path / "a.txt"), str(tmp_path / "key.txt"),
           "--side1-map", str(tmp_path / "m1.txt"), "--side2-map", str(tmp_path / "m2.txt"), "--n-boot", "100", "--seed", "2",
           "--betas", "9,19", "--llr", "--compare", str(tmp_path / "b.txt")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if len(f) >= 5 and f[0] in ("A", "B", "A-B"):
            rows[(f[0], f[1])] = tuple(float(x) for x in f[2:5])
    for sysname in ("A", "B"):
        for m in ("eer", "min_cost_9", "min_cost_19", "act_cost_9", "act_cost_19", "cllr"):
            p, lo, hi = rows[(sysname, m)]
            assert lo <= p <= hi, (sysname, m, p, lo, hi)
    assert ("A-B", "eer") in rows and rows[("A-B", "cllr")][1] <= rows[("A-B", "cllr")][2]
