"""PAV / ROC convex hull on the GPU (csrc/nplda_pav.hip) against tests/pav_ref.py.

The hull is integer work: the number of blocks and every (n_b, t_b, lo_b, hi_b) must be EQUAL to the reference's.
Floating-point tolerances are derived, not measured: the reference evaluates the same formulas in fp64, so
min Cllr (a sum of at most 2^31 positive fp64 terms, fixed order on both sides) is held to 1e-12 relative, the ROCCH EER
to 1e-12 absolute, and the block LLRs and the map to 4 ulp of fp64.  For llr_b = log(t / (n - t)) - log(N_t' / N_n') the
ulp is that of the larger of the two logarithms and the result: each logarithm is within 1 ulp OF ITSELF in either
library, and where the two nearly cancel no implementation of this formula can promise ulps of the (small) difference.
Where they do not cancel this is 4 ulp of llr_b itself.  The map is checked against the reference map of the DEVICE's
table, so that it is the map's own arithmetic that is held to 4 ulp.
Sizes straddle the level-0 chunk C = nplda_pav_chunk(): 2, 3, C - 1, C, C + 1, 2C, 2C + 1, 3C + 5, 7C + 3, 64C + 17, and
one case of 2^20 + 3."""
import os

import numpy as np
import pytest
import torch

from tests import pav_ref as pr

pytestmark = pytest.mark.gpu

FAMILIES = ["separated", "inverted", "tied", "alternating", "staircase", "reversed_staircase", "all_2_1", "left_anchor",
            "gauss", "gauss16", "specials", "excluded"]


def _sizes():
    from neuralplda_amd import ops
    C = ops.pav_chunk()
    return [2, 3, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 5, 7 * C + 3, 64 * C + 17]


def _from_bins(bins, N, rg, base=0.0):
    """Trials of the given (n, t) bins at scores base + 0.25 k, padded to N trials with excluded ones (label 0.5)."""
    s, y = [], []
    for k, (n, t) in enumerate(bins):
        s += [base + 0.25 * k] * n
        y += [1.0] * t + [0.0] * (n - t)
    pad = N - len(s)
    assert pad >= 0
    s += rg.standard_normal(pad).tolist()
    y += [0.5] * pad
    return np.array(s), np.array(y)


def _stairs(N):
    m = 1
    while (m + 1) * (m + 2) <= N:
        m += 1
    return m


def make(family, N, seed=0):
    """(scores fp64, labels) of N trials in a shuffled order."""
    rg = np.random.default_rng(1000 * seed + N)
    i = np.arange(N)
    if family == "separated":
        s, y = i.astype(np.float64), (i >= N // 2).astype(np.float64)
    elif family == "inverted":
        s, y = i.astype(np.float64), (i < N // 2).astype(np.float64)
    elif family == "tied":
        s, y = np.full(N, 1.5), (i % 3 == 0).astype(np.float64)
    elif family == "alternating":
        s, y = i.astype(np.float64) - 7.0, (i & 1).astype(np.float64)
    elif family == "staircase":
        m = _stairs(N)
        s, y = _from_bins([(m + 1, k) for k in range(1, m + 1)] if N >= 2 else [], N, rg)
    elif family == "reversed_staircase":
        m = _stairs(N)
        s, y = _from_bins([(m + 1, k) for k in range(m, 0, -1)], N, rg)
    elif family == "all_2_1":
        s, y = _from_bins([(2, 1)] * (N // 2), N, rg)
    elif family == "left_anchor":
        h = N // 2
        m = _stairs(N - h) if N - h >= 2 else 0
        s, y = _from_bins([(h, h)] + [(m + 1, k) for k in range(1, m + 1)], N, rg, base=-100.0)
    else:
        y = (rg.random(N) < 0.1).astype(np.float64)
        s = rg.standard_normal(N) + 2.0 * y
        if family in ("gauss16", "specials"):
            s = np.clip(np.round(s * 3.0), -7, 8) / 4.0  # 16 values
        if family == "specials":
            k = rg.integers(0, 6, size=N)
            s = np.where(k == 0, -np.inf, np.where(k == 1, np.inf, np.where(k == 2, -0.0, np.where(k == 3, 0.0, s))))
        if family == "excluded":
            y = np.where(rg.random(N) < 0.2, 0.5, y)
            s = np.where(rg.random(N) < 0.2, np.nan, s)
            y = np.where(rg.random(N) < 0.05, np.nan, y)
    p = rg.permutation(N)
    return s[p], y[p]


def _fit_dev(s, y, dtype, laplace, cap=None):
    from neuralplda_amd import ops
    S = torch.from_numpy(np.asarray(s, dtype=dtype)).cuda()
    T = torch.from_numpy(np.asarray(y, dtype=np.float32)).cuda()
    lo, hi, n, t, llr, summary = ops.pav_fit(S, T, laplace=laplace, cap=cap)
    rep = dict(zip(ops.PAV_SUMMARY, summary.tolist()))
    nb = min(int(rep["blocks"]), lo.numel())
    return dict(lo=lo[:nb].cpu().numpy(), hi=hi[:nb].cpu().numpy(), n=n[:nb].cpu().numpy(), t=t[:nb].cpu().numpy(),
                llr=llr[:nb].cpu().numpy(), rep=rep, dev=(lo[:nb], hi[:nb], llr[:nb]))


def _check(got, ref, laplace, tag):
    rep = got["rep"]
    print(f"{tag}: nb = {rep['blocks']:.0f} (ref {ref['nb']}), M = {rep['bins']:.0f}, min_cllr = {rep['min_cllr']!r} "
          f"(ref {ref['min_cllr']!r}), eer = {rep['rocch_eer']!r} (ref {ref['rocch_eer']!r})")
    assert (rep["n_tgt"], rep["n_non"], rep["bins"], rep["blocks"]) == (ref["N_t"], ref["N_n"], ref["M"], ref["nb"]), tag
    assert rep["overflow"] == 0.0 and rep["reserved"] == 0.0
    assert np.array_equal(got["n"], ref["n"]) and np.array_equal(got["t"], ref["t"]), tag
    assert np.array_equal(got["lo"], ref["lo"]) and np.array_equal(got["hi"], ref["hi"]), tag
    if ref["N_t"] == 0 or ref["N_n"] == 0:
        assert np.isnan(rep["min_cllr"]) and np.isnan(rep["rocch_eer"])
        return
    assert abs(rep["min_cllr"] - ref["min_cllr"]) <= 1e-12 * abs(ref["min_cllr"]), tag
    assert abs(rep["rocch_eer"] - ref["rocch_eer"]) <= 1e-12, tag
    off = 2 if laplace else 0
    with np.errstate(divide="ignore"):
        la = np.log(ref["t"].astype(np.float64) / (ref["n"] - ref["t"]).astype(np.float64))
    lb = np.log(np.float64(ref["N_t"] + off) / np.float64(ref["N_n"] + off))
    fin = np.isfinite(ref["llr"])
    assert np.array_equal(got["llr"][~fin], ref["llr"][~fin]), tag
    scale = np.maximum(np.maximum(np.abs(la[fin]), abs(lb)), np.abs(ref["llr"][fin]))
    err = np.abs(got["llr"][fin] - ref["llr"][fin]) / np.spacing(scale)
    print(f"{tag}: llr max error {err.max() if err.size else 0.0:.2f} ulp")
    assert (err <= 4.0).all(), tag
    assert (np.diff(got["llr"]) > 0).all()  # p_b strictly increasing


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", FAMILIES)
def test_block_table_equals_the_reference(hip_lib, family, dtype):
    for N in _sizes():
        s, y = make(family, N)
        s = s.astype(dtype)
        for laplace in (False, True):
            ref = pr.fit(s, y, laplace=laplace)
            _check(_fit_dev(s, y, dtype, laplace), ref, laplace, f"{family} N={N} laplace={laplace}")


def test_block_table_at_a_million_scores(hip_lib):
    N = 2 ** 20 + 3
    s, y = make("gauss", N)
    s = s.astype(np.float32)
    _check(_fit_dev(s, y, np.float32, False), pr.fit(s, y, laplace=False), False, "gauss N=2^20+3")


@pytest.mark.parametrize("family,N", [("staircase", 2 ** 20), ("left_anchor", 2 ** 20), ("alternating", 40000),
                                      ("all_2_1", 40000)])
def test_deep_trees_of_many_vertices(hip_lib, family, N):
    """Families whose points survive the candidate filter, at sizes that take the tree several levels past level 0: about
    a thousand vertices that all survive (staircases), and 20 000 collinear points that all go."""
    s, y = make(family, N)
    _check(_fit_dev(s, y, np.float64, True), pr.fit(s, y, laplace=True), True, f"{family} N={N}")


def _probes(lo, hi):
    fin = np.concatenate((lo[np.isfinite(lo)], hi[np.isfinite(hi)]))
    pts = [lo, hi, np.array([np.nan, -np.inf, np.inf, -0.0, 0.0])]
    if fin.size:
        pts += [np.array([fin.min() - 1.0, fin.max() + 1.0, fin.min() - 1e30, fin.max() + 1e30])]
    if lo.size > 1:
        a, b = hi[:-1], lo[1:]
        ok = np.isfinite(a) & np.isfinite(b)
        pts += [0.5 * (a[ok] + b[ok]), a[ok] + 0.25 * (b[ok] - a[ok]), np.nextafter(a[ok], np.inf), np.nextafter(b[ok], -np.inf)]
        pts += [np.where(np.isfinite(a), a, b)[~ok] + 1.0, np.where(np.isfinite(a), a, b)[~ok] - 1.0]
    return np.concatenate(pts)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["gauss", "gauss16", "specials", "staircase", "separated", "excluded"])
def test_apply_against_the_reference_map(hip_lib, family, dtype):
    from neuralplda_amd import ops
    C = ops.pav_chunk()
    for N in (3, 3 * C + 5, 64 * C + 17):
        s, y = make(family, N)
        s = s.astype(dtype)
        for laplace in (False, True):
            got = _fit_dev(s, y, dtype, laplace)
            if got["rep"]["n_tgt"] == 0 or got["rep"]["n_non"] == 0:
                continue  # no map without both classes (fit_pav raises)
            q = _probes(got["lo"], got["hi"]).astype(dtype)
            want = pr.apply(got["lo"], got["hi"], got["llr"], q.astype(np.float64))
            lo, hi, llr = got["dev"]
            out = ops.pav_apply(torch.from_numpy(q).cuda(), lo, hi, llr).cpu().numpy()
            assert out.dtype == np.float64
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(out), nan) and np.isnan(q[nan]).all()
            inf = np.isinf(want)
            assert np.array_equal(out[inf], want[inf])
            ok = ~nan & ~inf
            err = np.abs(out[ok] - want[ok]) / np.spacing(np.abs(want[ok]))
            print(f"{family} N={N} laplace={laplace}: {q.size} probes, max error {err.max() if err.size else 0:.2f} ulp")
            assert (err <= 4.0).all()
            out32 = ops.pav_apply(torch.from_numpy(q).cuda(), lo, hi, llr, out_dtype=torch.float32).cpu().numpy()
            assert out32.dtype == np.float32 and np.array_equal(out32[~nan], out[~nan].astype(np.float32))
            # non-decreasing over sorted scores
            qs = np.sort(q[~np.isnan(q)])
            o = ops.pav_apply(torch.from_numpy(qs).cuda(), lo, hi, llr).cpu().numpy()
            assert (o[1:] >= o[:-1]).all()


def test_apply_against_the_reference_table(hip_lib):
    """End to end: device fit + device map against reference fit + reference map; the LLR error of the table carries over."""
    s, y = make("gauss", 2065)
    got = _fit_dev(s, y, np.float64, True)
    ref = pr.fit(s, y, laplace=True)
    q = np.sort(np.concatenate((s, _probes(ref["lo"], ref["hi"]))))
    q = q[~np.isnan(q)]
    from neuralplda_amd import ops
    lo, hi, llr = got["dev"]
    out = ops.pav_apply(torch.from_numpy(q).cuda(), lo, hi, llr).cpu().numpy()
    want = pr.apply(ref["lo"], ref["hi"], ref["llr"], q)
    lb = abs(np.log((ref["N_t"] + 2) / (ref["N_n"] + 2)))
    assert (np.abs(out - want) <= 8.0 * np.spacing(np.maximum(np.abs(want), lb) + lb)).all()
    assert (out[1:] >= out[:-1]).all()


def test_two_calls_are_bitwise_identical(hip_lib):
    s, y = make("gauss", 64 * 32 + 17)
    a, b = _fit_dev(s, y, np.float32, True), _fit_dev(s, y, np.float32, True)
    for k in ("lo", "hi", "n", "t", "llr"):
        assert a[k].tobytes() == b[k].tobytes()
    assert np.array(list(a["rep"].values())).tobytes() == np.array(list(b["rep"].values())).tobytes()


@pytest.mark.parametrize("family", ["gauss", "gauss16"])
def test_min_cllr_is_invariant_under_an_increasing_map(hip_lib, family):
    from neuralplda_amd import metrics
    s, y = make(family, 7 * 32 + 3)
    s = s.astype(np.float32).astype(np.float64)
    a = metrics.min_cllr(s, y.astype(np.float32))
    b = metrics.min_cllr(2.0 * s + 1.0, y.astype(np.float32))  # exact in fp64: order and ties are kept
    assert a == b and isinstance(a, float)
    assert metrics.rocch_eer(s, y.astype(np.float32)) == metrics.rocch_eer(2.0 * s + 1.0, y.astype(np.float32))


def test_min_cllr_bounds_linear_calibration_and_rocch_eer_bounds_eer(hip_lib):
    from neuralplda_amd import metrics, score_calibration as sc
    s, y = make("gauss", 64 * 32 + 17)
    S, T = torch.from_numpy(s).cuda(), torch.from_numpy(y.astype(np.float32)).cuda()
    mc = metrics.min_cllr(S, T)
    cal = sc.fit_linear(S, T)
    lin = metrics.cllr(cal.apply(S), T)
    e, he = metrics.eer(S.float(), T), metrics.rocch_eer(S.float(), T)
    print(f"min_cllr = {mc:.6f} <= cllr(linear) = {lin:.6f}; rocch_eer = {he:.6f} <= eer = {e:.6f}")
    assert 0.0 < mc <= lin and 0.0 < he <= e + 1e-6
    ref = pr.fit(s, y, laplace=False)
    assert abs(mc - ref["min_cllr"]) <= 1e-12 * ref["min_cllr"]
    # the PAV map without the Laplace rule attains min Cllr on its own training data (to the rounding of cllr's sums)
    pav = sc.fit_pav(S, T, laplace=False)
    assert abs(metrics.cllr(pav.apply(S), T) - mc) <= 1e-9
    pfa, pmiss = metrics.rocch(S, T)
    rfa, rmiss = pr.rocch(ref["n"], ref["t"])
    assert np.array_equal(pfa, rfa) and np.array_equal(pmiss, rmiss) and pfa[0] == 1.0 and pmiss[-1] == 1.0


def test_overflow_flag_and_true_block_count(hip_lib):
    s, y = make("staircase", 64 * 32 + 17)
    ref = pr.fit(s, y, laplace=True)
    assert ref["nb"] > 4
    got = _fit_dev(s, y, np.float64, True, cap=1)
    assert got["rep"]["overflow"] == 1.0 and got["rep"]["blocks"] == ref["nb"]
    assert got["n"].tolist() == ref["n"][:1].tolist() and got["lo"].tolist() == ref["lo"][:1].tolist()
    assert abs(got["rep"]["min_cllr"] - ref["min_cllr"]) <= 1e-12 * ref["min_cllr"]
    got = _fit_dev(s, y, np.float64, True, cap=ref["nb"])
    assert got["rep"]["overflow"] == 0.0 and np.array_equal(got["n"], ref["n"])


def test_empty_class_raises(hip_lib):
    from neuralplda_amd import metrics, score_calibration as sc
    s = np.arange(10.0)
    for y in (np.ones(10, dtype=np.float32), np.zeros(10, dtype=np.float32)):
        for fn in (metrics.min_cllr, metrics.rocch_eer, metrics.rocch, sc.fit_pav):
            with pytest.raises(ValueError):
                fn(s, y)


def test_results_come_back_where_the_inputs_were(hip_lib):
    from neuralplda_amd import score_calibration as sc
    s, y = make("gauss16", 500)
    ref = pr.fit(s, y, laplace=True)
    want = pr.apply(ref["lo"], ref["hi"], ref["llr"], s)
    for S, Y in ((s, y), (torch.from_numpy(s), torch.from_numpy(y)), (torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())):
        m = sc.fit_pav(S, Y)
        assert np.array_equal(m.n, ref["n"]) and np.array_equal(m.t, ref["t"]) and np.array_equal(m.lo, ref["lo"])
        out = m.apply(S)
        assert type(out) is type(S) and (not isinstance(S, torch.Tensor) or out.device == S.device)
        o = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
        assert o.dtype == np.float64 and np.abs(o - want).max() <= 1e-13 * (1.0 + np.abs(want).max())
        o32 = m.apply(S, out_dtype=torch.float32)
        assert (o32.cpu().numpy() if isinstance(o32, torch.Tensor) else o32).dtype == np.float32
    assert "PavCalibration" in repr(m)


def _write_fixtures(tmp_path):
    rg = np.random.default_rng(11)
    n_dev, n_eval = 40, 25
    is_t = np.arange(n_dev) % 3 == 0
    dev = np.round(np.where(is_t, 1.5, -1.5) + 1.5 * rg.standard_normal(n_dev), 1)  # one decimal: some ties
    labels = [("target" if k % 2 else "tgt") if is_t[k] else ("nontarget" if k % 2 else "imp") for k in range(n_dev)]
    labels[7] = "unknown"
    dev_path, key_path, eval_path = (str(tmp_path / n) for n in ("dev_scores.tsv", "dev_key.tsv", "eval_scores.tsv"))
    with open(dev_path, "w") as fh:
        fh.write("modelid\tsegmentid\tside\tLLR\n")
        for k in range(n_dev):
            fh.write(f"m{k:03d}\tseg{k:03d}.sph\ta\t{float(dev[k])!r}\n")
    with open(key_path, "w") as fh:
        fh.write("modelid\tsegmentid\tside\ttargettype\n")
        for k in range(n_dev):
            fh.write(f"m{k:03d}\tseg{k:03d}.sph\ta\t{labels[k]}\n")
    ev = 3.0 * rg.standard_normal(n_eval)
    with open(eval_path, "w") as fh:
        fh.write("modelid\tsegmentid\tside\tLLR\n")
        for k in range(n_eval):
            fh.write(f"e{k:03d}\tutt{k:03d}.sph\tb\t{ev[k]:.7f}\n")
    t = np.array([1.0 if lab in ("target", "tgt") else (0.0 if lab in ("nontarget", "imp") else 0.5) for lab in labels])
    return dev_path, key_path, eval_path, dev, t, np.array([float(f"{v:.7f}") for v in ev])


def test_calibrate_scorefile_with_pav(hip_lib, tmp_path, capsys):
    from neuralplda_amd import score_calibration as sc
    dev_path, key_path, eval_path, dev, t, ev = _write_fixtures(tmp_path)
    out, model = sc.calibrate_scorefile(dev_path, key_path, eval_path, method="pav")
    assert out == str(tmp_path / "eval_scores_calibrated.tsv") and isinstance(model, sc.PavCalibration)
    direct = sc.fit_pav(dev, t)
    assert np.array_equal(model.llr, direct.llr) and np.array_equal(model.lo, direct.lo) and model.n_tgt + model.n_non == 39
    ref = pr.fit(dev, t, laplace=True)
    want = pr.apply(ref["lo"], ref["hi"], ref["llr"], ev)
    assert np.array_equal(direct.apply(ev), model.apply(ev))
    src, dst = open(eval_path).read().split("\n"), open(out).read().split("\n")
    assert len(src) == len(dst) == 27 and dst[0] == src[0]
    for k in range(25):
        a, b = src[k + 1].rsplit("\t", 1), dst[k + 1].rsplit("\t", 1)
        assert a[0] == b[0] and abs(float(b[1]) - want[k]) <= 1.5e-6
    # the command-line tool: --method pav, and min_Cllr at the END of the before / after lines
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("calibrate_scores_tool_pav", os.path.join(root, "tools", "calibrate_scores.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main([dev_path, key_path, dev_path, "--method", "pav", "--key", key_path, "--out", str(tmp_path / "dev_cal.tsv")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.lstrip().startswith(("before", "after"))]
    assert len(lines) == 2
    mcs = [float(ln.rsplit("min_Cllr = ", 1)[1]) for ln in lines]
    assert all(ln.rstrip().endswith(f"min_Cllr = {m:.6f}") for ln, m in zip(lines, mcs))
    want_mc = pr.fit(dev, t, laplace=False)["min_cllr"]
    assert abs(mcs[0] - want_mc) <= 1e-6 and mcs[1] >= mcs[0] - 1e-6  # a monotone map cannot lower min Cllr
    assert all(float(ln.split("Cllr = ")[1].split()[0]) >= m - 1e-6 for ln, m in zip(lines, mcs))
