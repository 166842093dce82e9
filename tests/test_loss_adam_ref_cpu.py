"""The numpy references of the loss and Adam tests (tests/loss_ref.py, tests/adam_ref.py), checked on the CPU.

Tolerances, all derived:
  * loss_ref at float64 against the same form in np.longdouble: the rounding count of loss_ref.softcdet_sum_bound /
    bce_sum_bound with 2^-53 in place of 2^-24 (numpy's exp, log1p are within one ulp, which is what the count assumes for
    the device), i.e. bound * 2^-29; per element of g, (16 + 3.5 max_k |v_k|) 2^-53 sum_k |contribution_k| (c_d <= 12 + 3.5 |v|
    for sigma', four more roundings for the coefficients and the sum).  On a platform whose long double is float64 both
    sides are the same numbers and the check is vacuous but still true.
  * loss_ref against the oracle where the oracle is accurate (|v| < 2: sg (1 - sg) loses at most 1 / (1 - sg) <= 8.4 ulps):
    1e-13 relative on g elementwise and on the scalars, ~500 float64 ulps, covers the oracle's different summation order
    over 2000 terms (n 2^-53 = 2e-13 worst case, sqrt(n) typical).
  * BCE against torch on CPU float64, |x| <= 8: torch evaluates log(1 - p) with p's rounding amplified by e^x <= 2981:
    2981 * 4 * 2^-53 = 1.3e-12 absolute per term; 2e-12 taken.
  * adam_ref at float64 against torch.optim.Adam on CPU float64 tensors: torch orders a few operations differently
    (addcdiv, lerp): ~10 roundings per step on quantities of the size of |dp|, m, v; 64 ulps relative to the largest
    magnitude of the tensor are taken per step, times the 6 steps."""
import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc
from tests import adam_ref, loss_ref

THETA = [-0.8, -0.6, -1.1, 0.3]
BETA = [99.0, 199.0, 9.9, 19.9]
ALPHA = 15.0
TH32 = [float(np.float32(x)) for x in THETA]
B32 = [float(np.float32(x)) for x in BETA]  # (the references take beta as the float32 the ABI receives)


def _scores(n, seed, extremes=True):
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal(n) * 2.5 - 1).astype(np.float32)
    t = (rng.random(n) < 0.15).astype(np.float32)
    if extremes:
        s[:8] = [50, -50, 1e4, -1e4, 50, -50, 1e4, -1e4]
        t[:8] = [1, 1, 1, 1, 0, 0, 0, 0]
    t[8], t[9] = 1, 0
    return s, t


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_softcdet_float64_against_long_double(K):
    s, t = _scores(3000, K)
    r = loss_ref.softcdet(s, t, THETA[:K], BETA[:K], ALPHA, np.float64)
    q = loss_ref.softcdet(s, t, THETA[:K], BETA[:K], ALPHA, np.longdouble)
    bound = loss_ref.softcdet_sum_bound(s, t, THETA[:K], ALPHA) * 2.0 ** -29
    assert r.sums[0] == q.sums[0] == t.sum() and r.sums[1] == q.sums[1]
    assert np.all(np.abs(r.sums - q.sums) <= bound), (np.abs(r.sums - q.sums), bound)
    nt, nn = r.sums[0], r.sums[1]
    vmax = np.zeros(s.shape)
    contrib = np.zeros(s.shape, np.longdouble)
    for k in range(K):
        vmax = np.maximum(vmax, np.abs(ALPHA * (TH32[k] - s.astype(np.float64))))
        d = q.terms[4 + 4 * k] + q.terms[5 + 4 * k]
        contrib += d * np.where(t > 0.5, ALPHA / (nt * K), BETA[k] * ALPHA / (nn * K))
    tol = (16 + 3.5 * vmax) * 2.0 ** -53 * contrib.astype(np.float64) + 1e-300
    assert np.all(np.abs(r.g - q.g).astype(np.float64) <= tol)
    assert abs(r.loss - q.loss) <= 8 * 2.0 ** -53 * abs(q.loss)
    # the hard cost: integers
    h = loss_ref.softcdet(s, t, THETA[:K], BETA[:K], 0.0, np.float64, hard=True)
    for k in range(K):
        assert h.sums[2 + 4 * k] == np.sum((s < np.float32(THETA[k])) & (t > 0.5))
        assert h.sums[3 + 4 * k] == np.sum((s > np.float32(THETA[k])) & (t < 0.5))
        assert h.sums[4 + 4 * k] == 0 and h.sums[5 + 4 * k] == 0


def test_bce_float64_against_long_double():
    s, t = _scores(3000, 11, extremes=False)
    s = np.clip(s, THETA[0] - 7.99, THETA[0] + 7.99)
    r = loss_ref.bce(s, t, THETA[0], np.float64)
    q = loss_ref.bce(s, t, THETA[0], np.longdouble)
    bound = loss_ref.bce_sum_bound(s, t, THETA[0]) * 2.0 ** -29
    assert np.all(np.abs(r.sums[2:] - q.sums[2:]).astype(np.float64) <= bound[2:])
    assert np.all(np.abs(r.g - q.g).astype(np.float64) <= 16 * 2.0 ** -53 / s.size)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_float32_unit_stays_within_the_sum_bound(K):
    """The bound the GPU test holds the kernels to is a worst case: the float32 evaluation of the same form (numpy's exp,
    and the model of the device's fast exponential) must sit inside it on the GPU test's kind of input."""
    s, t = _scores(5000, 20 + K)
    ref = loss_ref.softcdet(s, t, THETA[:K], BETA[:K], ALPHA, np.float64)
    bound = loss_ref.softcdet_sum_bound(s, t, THETA[:K], ALPHA)
    for exp in (None, loss_ref.expf_intrinsic_model):
        r32 = loss_ref.softcdet(s, t, THETA[:K], BETA[:K], ALPHA, np.float32, exp=exp)
        assert np.all(np.abs(r32.sums - ref.sums) <= bound), (exp, np.abs(r32.sums - ref.sums) / bound)
    sb = np.clip(s, THETA[0] - 7.99, THETA[0] + 7.99)
    for form in ("stable", "naive"):
        b32 = loss_ref.bce(sb, t, THETA[0], np.float32, form=form)
        b64 = loss_ref.bce(sb, t, THETA[0], np.float64)
        bb = loss_ref.bce_sum_bound(sb, t, THETA[0])
        assert np.all(np.abs(b32.sums - b64.sums)[2:] <= bb[2:]), (form, np.abs(b32.sums - b64.sums) / bb)


def test_against_the_oracle_where_it_is_accurate():
    rng = np.random.default_rng(5)
    K = 2
    # every |v_k| < 2: scores within 2 / alpha of both thresholds (they are 0.2 apart: |s - theta_k| < 0.12)
    s = (rng.uniform(-0.72, -0.68, 2000)).astype(np.float32)
    t = (rng.random(2000) < 0.15).astype(np.float32)
    t[0], t[1] = 1, 0
    assert np.abs(ALPHA * (np.array(TH32[:K])[:, None] - s[None, :])).max() < 2
    r = loss_ref.softcdet(s, t, THETA[:K], BETA[:K], ALPHA, np.float64)
    og, odth = orc.softcdet_grad(s, t, TH32[:K], BETA[:K], ALPHA, np.float64)
    assert np.all(np.abs(r.g - og) <= 1e-13 * np.abs(og))
    scale = np.abs(ALPHA * r.sums[4:6]).max()  # dtheta is a difference of two such quantities
    assert np.all(np.abs(r.dtheta - odth) <= 1e-13 * max(scale, np.abs(odth).max()))
    assert abs(r.loss - orc.softcdet(s, t, TH32[:K], BETA[:K], ALPHA, np.float64)) <= 1e-13 * abs(r.loss)
    # the hard cost and BCE on wide scores (|x| <= 8 for BCE)
    s2, t2 = _scores(2000, 6, extremes=False)
    h = loss_ref.softcdet(s2, t2, THETA[:3], BETA[:3], 0.0, np.float64, hard=True)
    assert abs(h.loss - orc.cdet(s2, t2, TH32[:3], B32[:3], np.float64)) <= 1e-13 * abs(h.loss)
    sb = np.clip(s2, THETA[0] - 7.99, THETA[0] + 7.99)
    b = loss_ref.bce(sb, t2, THETA[0], np.float64)
    assert abs(b.loss - orc.crossentropy(sb, t2, TH32[0], np.float64)) <= 2e-12
    bg, bd = orc.crossentropy_grad(sb, t2, TH32[0], np.float64)
    assert np.all(np.abs(b.g - bg) <= 1e-13 * np.abs(bg)) and abs(b.dtheta[0] - bd[0]) <= 1e-13
    # ... and where it is not: the documented tail of the oracle's sigma' (module docstring of loss_ref)
    sw = np.float32(THETA[0]) - np.float32(20.0 / ALPHA) * np.ones(4, np.float32)
    tw = np.array([1, 0, 1, 0], np.float32)
    rw = loss_ref.softcdet(sw, tw, THETA[:1], BETA[:1], ALPHA, np.float64)
    qw = loss_ref.softcdet(sw, tw, THETA[:1], BETA[:1], ALPHA, np.longdouble)
    ow, _ = orc.softcdet_grad(sw, tw, TH32[:1], BETA[:1], ALPHA, np.float64)
    assert np.all(np.abs(rw.g - qw.g) <= 1e-14 * np.abs(qw.g)) and np.abs(ow / rw.g - 1).max() > 1e-9


def test_bce_against_torch_and_its_float32_saturation():
    s, t = _scores(3000, 12, extremes=False)
    sb = np.clip(s, THETA[0] - 7.99, THETA[0] + 7.99)
    x = torch.from_numpy(sb.astype(np.float64)) - TH32[0]
    tt = torch.from_numpy(t.astype(np.float64))
    ref = torch.nn.functional.binary_cross_entropy(torch.sigmoid(x), tt, reduction="none").numpy()
    b = loss_ref.bce(sb, t, THETA[0], np.float64)
    assert np.all(np.abs(b.terms[2] - ref) <= 2e-12)
    assert abs(b.loss - ref.mean()) <= 2e-12
    # float32 semantics outside |x| <= 8 (what the kernel restates and tests/test_loss_fp32_gpu.py pins)
    xs = torch.tensor([20.0, -120.0, -20.0], dtype=torch.float32)
    ts = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float32)
    sat = torch.nn.functional.binary_cross_entropy(torch.sigmoid(xs), ts, reduction="none").numpy()
    assert sat[0] == 100.0 and sat[1] == 100.0 and abs(sat[2] - 20.0) <= np.spacing(np.float32(20.0))
    naive = loss_ref.bce(xs.numpy(), ts.numpy(), 0.0, np.float32, form="naive").terms[2]
    assert naive[0] == 100.0 and naive[1] == 100.0 and abs(naive[2] - 20.0) <= np.spacing(np.float32(20.0))
    stable = loss_ref.bce(xs.numpy(), ts.numpy(), 0.0, np.float64).terms[2]
    assert abs(stable[0] - 20.0) <= 1e-8 and stable[1] == 100.0  # the true cost of the first is 20, not the clamp


def test_adam_against_torch_with_a_lagging_parameter():
    rng = np.random.default_rng(3)
    shapes = [(5, 7), (33,), (4,)]
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-5
    p0 = [rng.standard_normal(sh).astype(np.float32) * 0.05 for sh in shapes]
    tp = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in p0]
    f = lambda x: float(np.float32(x))  # noqa: E731
    opt = torch.optim.Adam(tp, lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps), weight_decay=f(wd))
    drv = adam_ref.Driver(p0, lr, b1, b2, eps, wd, np.float64)
    has = [[1, 1, 1], [1, 0, 1], [1, 0, 1], [1, 1, 0], [1, 1, 1], [1, 1, 1]]  # parameter 1 lags by two steps, 2 by one
    for it, row in enumerate(has):
        grads = [(rng.standard_normal(sh) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32) if h else None
                 for sh, h in zip(shapes, row)]
        for q, g in zip(tp, grads):
            q.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
        opt.step()
        drv.step(grads)
        for i, q in enumerate(tp):
            tol = 64 * (it + 1) * 2.0 ** -53
            st = opt.state[q]
            assert int(st["step"]) == drv.t[i]
            for got, ref in ((q.detach().numpy(), drv.p[i]), (st["exp_avg"].numpy(), drv.m[i]),
                             (st["exp_avg_sq"].numpy(), drv.v[i])):
                assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), (it, i)
    assert drv.t == [6, 4, 5]


@pytest.mark.parametrize("B", loss_ref.BATCHES)
def test_float32_unit_within_the_bounds_on_the_gpu_tests_inputs(B):
    """tests/test_loss_fp32_gpu.py holds the kernels to softcdet_sum_bound / softcdet_g_bound / bce_sum_bound on
    loss_ref.make_scores: the float32 unit (numpy's exp, and the model of the device's fast exponential) is inside them on
    every one of those inputs."""
    for K in (1, 2, 3, 4):
        s, t = loss_ref.make_scores(B, K)
        r64 = loss_ref.softcdet(s, t, loss_ref.THETA[:K], loss_ref.BETA[:K], loss_ref.ALPHA, np.float64)
        sb = loss_ref.softcdet_sum_bound(s, t, loss_ref.THETA[:K], loss_ref.ALPHA)
        near = loss_ref.vmin(s, K) < 80
        for exp in (None, loss_ref.expf_intrinsic_model):
            r32 = loss_ref.softcdet(s, t, loss_ref.THETA[:K], loss_ref.BETA[:K], loss_ref.ALPHA, np.float32, exp=exp)
            assert r32.sums[0] == t.sum() and r32.sums[1] == (1 - t).sum()
            assert np.all(np.abs(r32.sums - r64.sums) <= sb)
            if B >= 2:
                gb = loss_ref.softcdet_g_bound(s, t, loss_ref.THETA[:K], loss_ref.BETA[:K], loss_ref.ALPHA)
                assert np.all(np.abs(r32.g.astype(np.float64) - r64.g)[near] <= gb[near])
    s, t = loss_ref.make_scores(B, 1, bce=True)
    b64 = loss_ref.bce(s, t, loss_ref.THETA[0], np.float64)
    bb = loss_ref.bce_sum_bound(s, t, loss_ref.THETA[0])
    for form in ("stable", "naive"):
        b32 = loss_ref.bce(s, t, loss_ref.THETA[0], np.float32, form=form)
        assert np.all(np.abs(b32.sums - b64.sums)[2:] <= bb[2:])


@pytest.mark.parametrize("hyper", ["default", "no-decay", "fast-betas"])
def test_float32_adam_within_its_rounding_bounds(hyper):
    """adam_ref.bounds is what tests/test_adam_fp32_gpu.py holds every element of the device's p', m', v' to: the float32
    evaluation of the reference is inside it on that test's kind of state, at every t it uses — and a step taken with the
    wrong t is far outside."""
    from tests.test_adam_fp32_gpu import HYPER, SMALL_SIZES, make_state
    hp = HYPER[hyper]
    for t in (1, 2, 3, 10, 1000, 100000):
        for p, g, m, v in make_state(SMALL_SIZES + [100000], t, hp, seed=t):
            r64 = adam_ref.step(p, g, m, v, t, *hp, dtype=np.float64)
            r32 = adam_ref.step(p, g, m, v, t, *hp, dtype=np.float32)
            for a, b, bd in zip(r32, r64, adam_ref.bounds(p, g, m, v, t, *hp)):
                assert np.all(np.abs(a.astype(np.float64) - b) <= bd)
            if p.size == 100000 and t in (2, 3):
                off = adam_ref.step(p, g, m, v, t + 1, *hp, dtype=np.float32)[0]
                assert np.mean(np.abs(off.astype(np.float64) - r64[0]) > adam_ref.bounds(p, g, m, v, t, *hp)[0]) > 0.5
