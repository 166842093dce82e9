"""Calibration on the device (csrc/nplda_calib.hip, neuralplda_amd/score_calibration.py, metrics.cllr / act_cost / act_dcf)
against the fp64 numpy reference tests/calib_ref.py.

The bound on every sum q = sum_i term_i is |q_gpu - q_ref| <= 1e-12 * sum_i |term_i|: a tree reduction over <= 2^21 fp64
terms adds at most ~21 * 2^-53 relative to that, the evaluation of a term a few ulp, which leaves about two orders of
magnitude.  Counts are exact."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from tests import calib_ref as cr

pytestmark = pytest.mark.gpu
REL = 1e-12


@functools.lru_cache(maxsize=None)
def _recipe(N, K):
    X, t = cr.recipe(N, K)
    if N < 4:  # the recipe's first target is trial 3: give the two-trial case both classes
        t = t.copy()
        t[0] = 1.0
    X.setflags(write=False)
    t.setflags(write=False)
    return X, t


@functools.lru_cache(maxsize=None)
def _ref_fit(N, K, p_target, l2):
    X, t = _recipe(N, K)
    return cr.newton(X, t, p_target, l2)


def _sweep_rows():
    from neuralplda_amd import _lib
    return int(_lib.load().nplda_calib_sweep_rows())


def _dev(a, dtype=None):
    x = torch.tensor(np.ascontiguousarray(a))  # a copy: the cached recipe arrays are read-only
    return (x if dtype is None else x.to(dtype)).cuda()


def _strided(X, ldx, dtype):
    """(N, K) device view of an (N, ldx) buffer whose padding is NaN: an over-read shows."""
    N, K = X.shape
    buf = torch.full((N, ldx), float("nan"), dtype=dtype, device="cuda")
    buf[:, :K] = _dev(X, dtype)
    return buf[:, :K]


def _check_pass(out, ref, K, what):
    cnt, J, g, H = (o.cpu().numpy() for o in out)
    assert cnt.tolist() == [ref["n_tgt"], ref["n_non"]], what
    assert np.isfinite(J).all() and np.isfinite(g).all() and np.isfinite(H).all(), what
    assert abs(J[0] - ref["J"]) <= REL * ref["J_abs"], (what, J[0], ref["J"])
    assert np.all(np.abs(g - ref["g"]) <= REL * ref["g_abs"]), (what, g, ref["g"])
    assert np.all(np.abs(H - cr.triu_pack(ref["H"])) <= REL * cr.triu_pack(ref["H_abs"])), (what, H)


# 1. one pass against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 257, 4099, "sweep+1"])
def test_pass_against_reference(hip_lib, N, K):
    from neuralplda_amd import ops
    if N == "sweep+1":  # one trial more than a full sweep of the grid: the first lane sums two
        N = _sweep_rows() + 1
        assert N <= 1 << 21
    X, t = _recipe(N, K)
    T = _dev(t)
    rg = np.random.default_rng(7 * N + K)
    thetas = [np.append(np.full(K, 1.0 / K), 0.0), rg.standard_normal(K + 1)]
    for dtype in (torch.float32, torch.float64):
        for ldx in (K, K + 3):
            Xd = _strided(X, ldx, dtype)
            for p_target in (0.5, 0.005):
                for theta in thetas:
                    for l2 in ((0.0, 1e-3) if ldx == K else (0.0,)):
                        out = ops.calib_logreg_pass(Xd, T, _dev(theta), p_target=p_target, l2=l2)
                        _check_pass(out, cr.logreg_pass(X, t, theta, p_target, l2), K, (N, K, dtype, ldx, p_target, l2))


# 2. extremes -----------------------------------------------------------------------------------------------------------
def test_pass_extremes(hip_lib):
    from neuralplda_amd import ops
    col = np.array([1e4, -1e4, 0.0, 1e4, -1e4, 0.0, 3.0, -3.0], dtype=np.float32)
    t = np.array([1, 1, 1, 0, 0, 0, 1, 0], dtype=np.float32)
    for K in (1, 2):
        X = np.stack([col, col[::-1]][:K], axis=1)
        for theta in (np.append(np.full(K, 50.0), 0.0), np.append(np.full(K, 1.0), 0.0), np.append(np.full(K, -50.0), 3.0)):
            for dtype in (torch.float32, torch.float64):
                out = ops.calib_logreg_pass(_dev(X, dtype), _dev(t), _dev(theta), p_target=0.5)
                ref = cr.logreg_pass(X, t, theta, 0.5, 0.0)
                assert np.isfinite(ref["J"]) and ref["J"] > 1e3  # a target at -1e4 costs 1e4 |a| times its weight, not inf
                _check_pass(out, ref, K, (K, theta, dtype))
    # a single trial at z = +-1e4: softplus gives 1e4 or 0
    X1 = np.array([[1e4], [1e4]], dtype=np.float32)
    _, J, _, _ = ops.calib_logreg_pass(_dev(X1), _dev(np.array([1, 0], dtype=np.float32)), _dev(np.array([1.0, 0.0])))
    assert J.item() == 0.5 * 1e4
    _, J, _, _ = ops.calib_logreg_pass(_dev(X1), _dev(np.array([0, 1], dtype=np.float32)), _dev(np.array([1.0, 0.0])))
    assert J.item() == 0.5 * 1e4


# 3. the fit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", [0.0, 1e-3])
@pytest.mark.parametrize("p_target", [0.5, 0.005])
@pytest.mark.parametrize("N,K", [(65, 1), (257, 2), (257, 3), (257, 8), (4099, 8), (131073, 1)])
def test_fit_against_reference(hip_lib, N, K, p_target, l2):
    from neuralplda_amd import metrics, score_calibration as sc
    X, t = _recipe(N, K)
    tol = 1e-10
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = sc.fit_linear(_dev(X), _dev(t), p_target=p_target, l2=l2, tol=tol)
    assert m.converged and m.passes <= 64 and m.iterations <= m.passes
    th_gpu = np.append(m.a, m.b)
    th_ref, info = _ref_fit(N, K, p_target, l2)
    assert info["converged"]
    at_gpu = cr.logreg_pass(X, t, th_gpu, p_target, l2)
    at_ref = cr.logreg_pass(X, t, th_ref, p_target, l2)
    print(f"N={N} K={K} p={p_target} l2={l2}: passes {m.passes} (ref {info['passes']}), |g(theta_gpu)| = "
          f"{np.abs(at_gpu['g']).max():.3e}, J_gpu - J_ref = {at_gpu['J'] - at_ref['J']:.3e}, "
          f"|dtheta| = {np.abs(th_gpu - th_ref).max():.3e}")
    assert np.all(np.abs(at_gpu["g"]) <= tol + REL * at_gpu["g_abs"])
    assert at_gpu["J"] <= at_ref["J"] + 1e-12
    assert abs(m.objective - at_gpu["J"]) <= REL * at_gpu["J_abs"]
    hinv = np.abs(np.linalg.inv(at_ref["H"])).sum(axis=1).max()
    assert np.abs(th_gpu - th_ref).max() <= 2.0 * hinv * (np.abs(at_gpu["g"]).max() + np.abs(at_ref["g"]).max())
    if K == 1 and p_target == 0.5:
        # calibrating at p_target = 0.5 minimises Cllr itself (l2 = 0); with the ridge the optimum's slope stays above 1 on
        # this recipe (the class means are 4 apart at a standard deviation of 1.5), which keeps the inequality
        before = metrics.cllr(_dev(X[:, 0]), _dev(t))
        after = metrics.cllr(m.apply(_dev(X)), _dev(t))
        assert after <= before + 1e-12
        assert abs(after * np.log(2.0) - (at_gpu["J"] - 0.5 * l2 * m.a[0] ** 2)) <= 1e-12


# 4. separable data and the ridge -----------------------------------------------------------------------------------------
def test_two_point_problem(hip_lib):
    from neuralplda_amd import score_calibration as sc
    X, t = np.array([[1.0], [-1.0]]), np.array([1.0, 0.0], dtype=np.float32)
    m = sc.fit_linear(_dev(X), _dev(t), p_target=0.5, l2=1e-3)
    ref, info = cr.newton(X, t, 0.5, 1e-3)
    assert m.converged and m.iterations == info["iterations"] == 8
    assert abs(m.a[0] - ref[0]) <= 1e-12 and abs(m.a[0] - 5.245185654) < 5e-9 and abs(m.b) <= 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # running out of budget is allowed here, raising is not
        m0 = sc.fit_linear(_dev(X), _dev(t), p_target=0.5, l2=0.0)
    assert np.isfinite(m0.a).all() and np.isfinite(m0.b) and m0.passes <= 64
    X16, t16 = _recipe(16, 1)  # separable: a runs to ~36 before the gradient is below the tolerance
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m16 = sc.fit_linear(_dev(X16), _dev(t16))
    assert np.isfinite(m16.a).all() and np.isfinite(m16.b) and m16.passes <= 64


# 5. degenerate input ---------------------------------------------------------------------------------------------------
def test_degenerate_input(hip_lib):
    from neuralplda_amd import _lib, ops, score_calibration as sc
    X, t = _recipe(257, 2)
    for const in (0.0, 1.0):
        with pytest.raises(ValueError):
            sc.fit_linear(_dev(X), _dev(np.full(257, const, dtype=np.float32)))
        with pytest.raises(ValueError):
            sc.calibrate_train(_dev(X[:, 0]), _dev(np.full(257, const, dtype=np.float32)))
    Xn = X.copy()
    Xn[100, 1] = np.nan
    with pytest.raises(_lib.NpldaHipError):
        sc.fit_linear(_dev(Xn), _dev(t))
    start = np.array([0.3, -0.2, 0.1])
    theta = _dev(start)
    rep = dict(zip(ops.CALIB_REPORT, ops.calib_logreg_fit(_dev(Xn), _dev(t), theta).tolist()))
    assert rep["not_finite"] == 1.0 and rep["converged"] == 0.0 and rep["passes"] == 1.0
    assert theta.cpu().numpy().tolist() == start.tolist()
    with pytest.raises(_lib.NpldaHipError):
        sc.fit_linear(_dev(np.zeros((64, 9), dtype=np.float32)), _dev(t[:64]))
    with pytest.raises(_lib.NpldaHipError):
        ops.calib_apply_linear(_dev(np.zeros((64, 9), dtype=np.float32)), _dev(np.zeros(10)))
    with pytest.raises(ValueError):
        sc.calibrate_train(_dev(np.full(64, 2.5, dtype=np.float32)), _dev(t[:64]))  # zero standard deviation


# 6. the Gaussian model -------------------------------------------------------------------------------------------------
def _check_gauss(m, s, t):
    s = np.asarray(s, dtype=np.float64)
    for got, want in ((m.mu_tgt, np.mean(s[t > 0.5])), (m.std_tgt, np.std(s[t > 0.5])), (m.mu_imp, np.mean(s[t < 0.5])),
                      (m.std_imp, np.std(s[t < 0.5]))):
        assert abs(got - want) <= REL * abs(want), (got, want)
    assert (m.n_tgt, m.n_imp) == (int((t > 0.5).sum()), int((t < 0.5).sum()))


@pytest.mark.parametrize("N", [65, 4099, "sweep+1"])
def test_gaussian_fit(hip_lib, N):
    from neuralplda_amd import score_calibration as sc
    N = _sweep_rows() + 1 if N == "sweep+1" else N
    X, t = _recipe(N, 1)
    _check_gauss(sc.calibrate_train(_dev(X[:, 0]), _dev(t)), X[:, 0], t)
    _check_gauss(sc.calibrate_train(_dev(X[:, 0].astype(np.float64)), _dev(t)), X[:, 0], t)
    # mean 1e4, standard deviation 1e-2: sum s^2 - (sum s)^2 / n is wrong in the fourth digit here
    s = 1e4 + 1e-2 * np.random.default_rng(N).standard_normal(N)
    _check_gauss(sc.calibrate_train(_dev(s), _dev(t)), s, t)


def test_gaussian_apply_and_labels(hip_lib):
    from neuralplda_amd import score_calibration as sc
    X, t = _recipe(4099, 1)
    s = X[:, 0].astype(np.float64)
    ref_mdl = cr.gauss_train(s, t)
    mt, st, mn, sn = ref_mdl["tgt"].mean(), ref_mdl["tgt"].std(), ref_mdl["imp"].mean(), ref_mdl["imp"].std()
    want = cr.gauss_apply(s, ref_mdl)
    terms = abs(np.log(sn)) + abs(np.log(st)) + (s - mt) ** 2 / (2 * st * st) + (s - mn) ** 2 / (2 * sn * sn)
    for mdl in (sc.GaussianCalibration(mt, st, mn, sn), ref_mdl):  # the package's model and the reference's dict
        for dtype in (torch.float32, torch.float64):
            got = sc.calibrate_apply(_dev(s, dtype), mdl)
            assert got.dtype == torch.float64 and got.shape == (4099,)
            assert np.all(np.abs(got.cpu().numpy() - want) <= REL * terms)
    # label strings, one of them ignored (last, so that every other trial keeps its place in the reduction)
    n = 100
    lab = np.where(t[:n] > 0.5, "target", "nontarget").astype(object)
    lab[1::4] = np.where(t[1:n:4] > 0.5, "tgt", "imp")
    lab[n - 1] = "unknown"
    a = sc.calibrate_train(_dev(X[:n, 0]), np.array(lab))
    b = sc.calibrate_train(_dev(X[:n - 1, 0]), _dev(t[:n - 1]))
    assert (a.mu_tgt, a.std_tgt, a.mu_imp, a.std_imp, a.n_tgt, a.n_imp) == (b.mu_tgt, b.std_tgt, b.mu_imp, b.std_imp,
                                                                           b.n_tgt, b.n_imp)
    assert a["tgt"].mean() == a.mu_tgt and a["imp"].std() == a.std_imp


# 7. apply, linear ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8])
def test_apply_linear(hip_lib, K):
    from neuralplda_amd import ops
    X, _ = _recipe(4099, K)
    theta = np.random.default_rng(K).standard_normal(K + 1)
    exact = (X.astype(np.longdouble) * theta[:K].astype(np.longdouble)).sum(axis=1) + np.longdouble(theta[K])
    mag = (np.abs(X.astype(np.float64)) * np.abs(theta[:K])).sum(axis=1) + abs(theta[K])
    for ldx in (K, K + 3):
        Xd = _strided(X, ldx, torch.float32)
        o64 = ops.calib_apply_linear(Xd, _dev(theta)).cpu().numpy()
        assert o64.dtype == np.float64
        assert np.all(np.abs(o64.astype(np.longdouble) - exact) <= 4 * np.spacing(mag))
        o32 = ops.calib_apply_linear(Xd, _dev(theta), out_dtype=torch.float32).cpu().numpy()
        assert o32.dtype == np.float32
        assert np.all(np.abs(o32.astype(np.longdouble) - exact) <= np.spacing(np.abs(exact).astype(np.float32)))


# 8. metrics ------------------------------------------------------------------------------------------------------------
def test_cllr_and_counts(hip_lib):
    from neuralplda_amd import metrics, ops
    for N in (65, 4099, _sweep_rows() + 1):
        X, t = _recipe(N, 1)
        llr = X[:, 0].copy()
        ths = [0.0, float(llr[5]), float(llr[11]), float("inf"), float("-inf"), -1.5]  # two thresholds tie with a score
        llr[20:30] = llr[5]
        for dtype in (torch.float32, torch.float64):
            L, T = _dev(llr, dtype), _dev(t)
            assert abs(metrics.cllr(L, T) - cr.cllr(llr, t)) <= REL * cr.cllr(llr, t)
            cnt, miss, fa, sums = ops.calib_costs(L, T, ths)
            rm, rf = cr.counts(llr, t, ths)
            assert cnt.tolist() == [int((t > 0.5).sum()), int((t < 0.5).sum())]
            assert miss.tolist() == rm and fa.tolist() == rf
            assert miss[3].item() == cnt[0].item() and fa[3].item() == 0 and miss[4].item() == 0 and fa[4].item() == cnt[1].item()
            st, sn, _, _ = cr.cllr_sums(llr, t)
            assert abs(sums[0].item() - st) <= REL * st and abs(sums[1].item() - sn) <= REL * sn
    big = np.array([1e4, -1e4, 0.0, 1e4, -1e4, 0.0], dtype=np.float32)
    tb = np.array([1, 1, 1, 0, 0, 0], dtype=np.float32)
    want = 0.5 * ((0 + 1e4 + np.log(2.0)) / 3 + (1e4 + 0 + np.log(2.0)) / 3) / np.log(2.0)
    assert abs(metrics.cllr(_dev(big), _dev(tb)) - want) <= REL * want


@pytest.mark.parametrize("n,ptgt,quant", [(2, 0.5, None), (17, 0.3, None), (1000, 0.1, 0.05), (4097, 0.02, None)])
def test_act_cost_bounds_minc_exact(hip_lib, n, ptgt, quant):
    from neuralplda_amd import metrics
    rg = np.random.default_rng(n)  # the inputs of tests/test_metrics_gpu.py::test_sweep_vs_oracle
    t = (rg.random(n) < ptgt).astype(np.float32)
    t[0], t[1] = 1.0, 0.0
    s = (rg.standard_normal(n) + 2.0 * t).astype(np.float32)
    if quant:
        s = (np.round(s / quant) * quant).astype(np.float32)
    betas = [99.0, 199.0, 9.9]
    S, T = _dev(s), _dev(t)
    avg, cost = metrics.act_cost(S, T, betas)
    nt, nn = int((t > 0.5).sum()), int((t < 0.5).sum())
    rm, rf = cr.counts(s, t, [np.log(b) for b in betas])
    for k, b in enumerate(betas):
        assert cost[b] == rm[k] / nt + b * (rf[k] / nn)
        mc, _ = metrics.minc_exact(S, T, [b])
        assert cost[b] >= mc.item() - 1e-6 * max(1.0, cost[b])  # minc_exact returns float32
    assert abs(avg - sum(cost.values()) / 3) <= 1e-15 * avg
    avg2, cost2 = metrics.act_cost(S, T, [99.0, 99.0, 9.9])  # a repeated beta counts twice in the average
    assert cost2 == {99.0: cost[99.0], 9.9: cost[9.9]} and abs(avg2 - (2 * cost[99.0] + cost[9.9]) / 3) <= 1e-15 * max(avg2, 1.0)
    for p_target, c_miss, c_fa in ((0.01, 1.0, 1.0), (0.005, 1.0, 1.0), (0.5, 10.0, 1.0)):
        wm, wf = c_miss * p_target, c_fa * (1.0 - p_target)
        (m1,), (f1,) = cr.counts(s, t, [np.log(wf / wm)])
        want = (wm * m1 / nt + wf * f1 / nn) / min(wm, wf)
        assert abs(metrics.act_dcf(S, T, p_target, c_miss, c_fa) - want) <= 1e-15 * max(want, 1.0)
    # beta = c_fa (1 - p) / (c_miss p): act_dcf is act_cost renormalised
    assert abs(metrics.act_dcf(S, T, 0.01) - cost[99.0] * (0.01 / min(0.01, 0.99))) <= 1e-12


# 9. determinism ---------------------------------------------------------------------------------------------------------
def test_bitwise_repeatable(hip_lib):
    from neuralplda_amd import ops, score_calibration as sc
    N, K = _sweep_rows() + 1, 3
    X, t = _recipe(N, K)
    theta = _dev(np.array([0.4, 0.3, 0.2, -0.1]))
    Xc, T = _dev(X), _dev(t)
    Xv = _strided(X, K + 3, torch.float32)
    assert not Xv.is_contiguous()
    a = torch.cat(ops.calib_logreg_pass(Xc, T, theta, p_target=0.05, l2=1e-3))
    b = torch.cat(ops.calib_logreg_pass(Xc, T, theta, p_target=0.05, l2=1e-3))
    c = torch.cat(ops.calib_logreg_pass(Xv, T, theta, p_target=0.05, l2=1e-3))
    assert torch.equal(a, b) and torch.equal(a, c)
    fits = [sc.fit_linear(x, T, p_target=0.05) for x in (Xc, Xc, Xv)]
    for m in fits[1:]:
        assert m.a.tolist() == fits[0].a.tolist() and m.b == fits[0].b and m.objective == fits[0].objective
        assert m.passes == fits[0].passes
    # the whole budget in one call gives the bits of the chunked default
    th1 = _dev(np.append(np.full(K, 1.0 / K), 0.0))
    rep = ops.calib_logreg_fit(Xc, T, th1, p_target=0.05, chunk=None)
    assert th1.cpu().numpy().tolist() == np.append(fits[0].a, fits[0].b).tolist() and rep[3].item() == fits[0].passes
    s2 = _dev(np.repeat(X[:4099, 0], 2))[::2]  # every other element of a 1-D tensor
    assert not s2.is_contiguous()
    m1, m2 = sc.fit_linear(s2, T[:4099]), sc.fit_linear(s2.contiguous(), T[:4099])
    assert m1.a.tolist() == m2.a.tolist() and m1.b == m2.b


# 10. device placement ----------------------------------------------------------------------------------------------------
def test_cpu_inputs_give_cpu_outputs(hip_lib):
    from neuralplda_amd import metrics, score_calibration as sc
    X, t = _recipe(4099, 2)
    md = sc.fit_linear(_dev(X), _dev(t), p_target=0.05)
    for Xc, tc in ((X, t), (torch.tensor(X), torch.tensor(t))):
        mc = sc.fit_linear(Xc, tc, p_target=0.05)
        assert mc.a.tolist() == md.a.tolist() and mc.b == md.b
        out = mc.apply(Xc)
        assert isinstance(out, type(Xc)) and (not isinstance(out, torch.Tensor) or out.device.type == "cpu")
        assert np.array_equal(np.asarray(out), md.apply(_dev(X)).cpu().numpy())
        g = sc.calibrate_train(Xc[:, 0], tc)
        gd = sc.calibrate_train(_dev(X[:, 0]), _dev(t))
        assert (g.mu_tgt, g.std_tgt, g.mu_imp, g.std_imp) == (gd.mu_tgt, gd.std_tgt, gd.mu_imp, gd.std_imp)
        cal = sc.calibrate_apply(Xc[:, 0], g)
        assert isinstance(cal, type(Xc)) and (not isinstance(cal, torch.Tensor) or cal.device.type == "cpu")
        cald = sc.calibrate_apply(_dev(X[:, 0]), gd)
        assert cald.is_cuda and np.array_equal(np.asarray(cal), cald.cpu().numpy())
        assert metrics.cllr(np.asarray(cal), tc) == metrics.cllr(cald, _dev(t))
    assert md.apply(_dev(X)).is_cuda


# 11. file level --------------------------------------------------------------------------------------------------------
def _write_fixtures(tmp_path):
    rg = np.random.default_rng(11)
    n_dev, n_eval = 40, 25
    is_t = np.arange(n_dev) % 3 == 0
    dev = np.where(is_t, 1.5, -1.5) + 1.5 * rg.standard_normal(n_dev)
    names = ["target" if k % 2 else "tgt" for k in range(n_dev)]
    labels = [names[k] if is_t[k] else ("nontarget" if k % 2 else "imp") for k in range(n_dev)]
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
    keep = np.array([lab != "unknown" for lab in labels])
    t = np.where(np.isin(labels, ["target", "tgt"]), 1.0, 0.0)
    return dev_path, key_path, eval_path, dev[keep], t[keep], np.array([float(f"{v:.7f}") for v in ev])


@pytest.mark.parametrize("method", ["gaussian", "linear"])
def test_calibrate_scorefile(hip_lib, tmp_path, method):
    from neuralplda_amd import score_calibration as sc
    dev_path, key_path, eval_path, dev, t, ev = _write_fixtures(tmp_path)
    out, model = sc.calibrate_scorefile(dev_path, key_path, eval_path, method=method)
    assert out == str(tmp_path / "eval_scores_calibrated.tsv") and os.path.exists(out)
    if method == "gaussian":
        want = cr.gauss_apply(ev, cr.gauss_train(dev, t))
    else:
        th, info = cr.newton(dev, t)
        assert info["converged"] and model.converged
        want = th[0] * ev + th[1]
    src, dst = open(eval_path).read().split("\n"), open(out).read().split("\n")
    assert len(src) == len(dst) == 27 and dst[0] == src[0] and dst[-1] == src[-1] == ""
    for k in range(25):
        a, b = src[k + 1].rsplit("\t", 1), dst[k + 1].rsplit("\t", 1)
        assert a[0] == b[0]
        assert len(b[1].split(".")[1]) == 6 and abs(float(b[1]) - want[k]) <= 1.5e-6
    # an explicit output path; the input is not touched
    out2, _ = sc.calibrate_scorefile(dev_path, key_path, eval_path, method=method, out=str(tmp_path / "elsewhere.txt"))
    assert out2 == str(tmp_path / "elsewhere.txt") and open(out2).read() == open(out).read()
    assert open(eval_path).read().split("\n") == src


def test_command_line_tool(hip_lib, tmp_path, capsys):
    """tools/calibrate_scores.py in-process: writes the calibrated file and, given a key, prints the metrics before and after."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("calibrate_scores_tool", os.path.join(root, "tools", "calibrate_scores.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    dev_path, key_path, eval_path, dev, t, ev = _write_fixtures(tmp_path)
    eval_key = str(tmp_path / "eval_key.tsv")
    lab = ["target" if (k % 4 == 0) == (ev[k] > -1.0) or k % 7 == 0 else "nontarget" for k in range(25)]
    with open(eval_key, "w") as fh:
        fh.write("modelid\tsegmentid\tside\ttargettype\n")
        for k in range(25):
            fh.write(f"e{k:03d}\tutt{k:03d}.sph\tb\t{lab[k]}\n")
    te = np.array([1.0 if x == "target" else 0.0 for x in lab])
    assert 0 < te.sum() < 25
    for method in ("gaussian", "linear"):
        tool.main([dev_path, key_path, eval_path, "--method", method, "--key", eval_key, "--betas", "9.9,99"])
        out = capsys.readouterr().out
        assert "wrote " + str(tmp_path / "eval_scores_calibrated.tsv") in out
        rows = {ln.split(":")[0].strip(): ln for ln in out.splitlines() if ln.lstrip().startswith(("before", "after"))}
        assert set(rows) == {"before", "after"}
        before = float(rows["before"].split("Cllr = ")[1].split()[0])
        assert abs(before - cr.cllr(ev, te)) <= 1e-6
        for ln in rows.values():  # the cost at the Bayes threshold cannot beat the minimum over thresholds
            assert float(ln.split("act_cost = ")[1].split()[0]) >= float(ln.split("minc_exact = ")[1].split()[0]) - 1e-6
