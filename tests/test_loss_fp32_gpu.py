"""The loss kernels (csrc/nplda_loss.hip, nplda_loss_math.h, nplda_loss_single.h) against tests/loss_ref.py at float32
resolution: SoftCdet for K = 1 .. 4 thresholds (K = 4 is the `default:` arm of the launch switches), the hard cost, BCE.

Inputs (loss_ref.make_scores): scores N(-1, 2.5) with 8 % moved into every band of min_k |v_k| = min_k |alpha (theta_k - s)|,
the extremes +-50 and +-1e4, scores exactly equal to every theta_k, ~15 % targets.  Batches (loss_ref.BATCHES): the
one-block form and its float4 / tail split (1 .. 5, 1023 .. 1025, 4095, 4096), the multi-block form (4097; the views offset
by one element at 1025 and 4096, which are not 16-byte aligned), the grid-stride loop's second pass (more than 1024 x 256
pairs: 262 145) and third (600 001).  Both forms of every batch: loss_sums + loss_finish, and loss_fwd_bwd.

Checks
  sums       N_t, N_n exact; every other entry within loss_ref.softcdet_sum_bound / bce_sum_bound of the float64 reference:
             2^-24 sum_i c_i |term_i| with c_i a count of the float32 roundings of softcdet_accumulate / bce_accumulate
             (written out in those functions' docstrings) — a worst case, not a measurement; the float32 evaluation of the
             reference is held to the same bound on the same inputs in tests/test_loss_adam_ref_cpu.py.
  loss, dθ   recomputed in float64 from the device's OWN sums by the formulas of softcdet_scalars / bce_scalars: the device's
             float32 value is that number rounded once (2^-24 relative; dθ is a difference a - b formed in fp64, so
             2^-24 |a - b| + 2^-48 (|a| + |b|)).
  g          every element within loss_ref.softcdet_g_bound (the same rounding count) for min_k |v_k| < 80; per band of
             min_k |v_k| that holds >= 256 elements, fp32_units.ratios against loss_ref in float64 / float32 at the default
             gates 3 (rms) / 5 (max); beyond 80, where float32 exp goes denormal, finite and no larger than the
             reference's magnitude at |v| = 80.
  hard cost  miss and false-alarm counts are exact integers; a score equal to theta_k counts as neither.
  BCE        the bound and the units for |s - theta| <= 8; outside, the float32 semantics of
             binary_cross_entropy(sigmoid(x), t) that the kernel restates are pinned: see test_bce_saturation.

B = 1 has one class only (N_n = 0: the loss is 0/0 as in the reference's formula): sums only.

Measured on MI355X (the CPU emulation with __expf modelled as exp2 of a rounded product gives 1.0-1.5 / 0.8-1.7 for g):

    case (both forms give the same figures; worst over K = 1 .. 4)     measured
    ------------------------------------------------------------------  -----------------------------------------------
    SoftCdet g, rms / max fp32 units, band [0, 2)                       1.04 / 1.18
                                      band [2, 10)                      1.29 / 1.88
                                      band [10, 30)                     1.77 / 2.26
                                      band [30, 60)                     1.66 / 1.88
                                      band [60, 80)                     1.51 / 1.98
    SoftCdet sums, share of the rounding bound, B <= 5                  0.02 - 0.58
                                                B >= 1023               0.008 - 0.048
    BCE sums, share of the rounding bound                               0.006 - 0.079
    BCE g, rms / max fp32 units (B >= 1023)                             0.66 - 0.98 / 0.81 - 1.00
    loss inside train_step, K = 4: |dL| / tolerance                     0.010 (B = 1003), 0.001 (B = 4096)
                                   |d dtheta| / tolerance               <= 0.008
    loss inside dplda_update_loss: |dL|, |d dtheta| / tolerance         0.04 - 0.12, <= 0.07
"""
import numpy as np
import pytest
import torch

from tests import fp32_units as fu
from tests import loss_ref as lr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_refs = {}


def reference(B, K, kind):
    """(s, t, ref64, ref32, sum bound, g bound) of a case, computed once and shared by the tests that use it."""
    key = (B, K, kind)
    if key not in _refs:
        if kind == "bce":
            s, t = lr.make_scores(B, 1, bce=True)
            r64, r32 = lr.bce(s, t, lr.THETA[0], np.float64), lr.bce(s, t, lr.THETA[0], np.float32)
            sb, gb = lr.bce_sum_bound(s, t, lr.THETA[0]), None
        else:
            s, t = lr.make_scores(B, K)
            r64 = lr.softcdet(s, t, lr.THETA[:K], lr.BETA[:K], lr.ALPHA, np.float64, hard=kind == "hard")
            r32 = None if kind == "hard" else lr.softcdet(s, t, lr.THETA[:K], lr.BETA[:K], lr.ALPHA, np.float32)
            sb = None if kind == "hard" else lr.softcdet_sum_bound(s, t, lr.THETA[:K], lr.ALPHA)
            gb = None if kind == "hard" or B < 2 else lr.softcdet_g_bound(s, t, lr.THETA[:K], lr.BETA[:K], lr.ALPHA)
        for a in (s, t):
            a.setflags(write=False)
        _refs[key] = (s, t, r64, r32, sb, gb)
    return _refs[key]


def device_pair(s, t, offset):
    """(S, T) on the device; offset=1: views one element into a larger buffer (not 16-byte aligned: the multi-block path)."""
    if not offset:
        return torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    S, T = torch.zeros(s.size + 8, device="cuda"), torch.zeros(s.size + 8, device="cuda")
    S[1:1 + s.size] = torch.from_numpy(s).cuda()
    T[1:1 + s.size] = torch.from_numpy(t).cuda()
    S, T = S[1:1 + s.size], T[1:1 + s.size]
    assert S.data_ptr() % 16 == 4 and S.is_contiguous()
    return S, T


def thetas(K):
    return [torch.tensor([x], dtype=torch.float32, device="cuda") for x in lr.THETA[:K]]


def check_sums(sums, r64, bound, what):
    assert sums[0] == r64.sums[0] and sums[1] == r64.sums[1], (what, sums[:2], r64.sums[:2])
    err = np.abs(sums - r64.sums)[2:]
    assert np.all(err <= bound[2:]), f"{what}: sums off by {err / bound[2:]} of the rounding bound"
    return float((err / bound[2:]).max())


def check_scalars(sums, loss, dth, K, kind, what):
    if kind == "bce":
        L, d = lr.bce_scalars(sums)
        n = sums[0] + sums[1]
        tol = U * np.abs(d) + 2.0 ** -48 * np.abs(sums[3]) / n
    else:
        L, d = lr.softcdet_scalars(sums, lr.BETA[:K], lr.ALPHA, K)
        a = float(np.float32(lr.ALPHA))
        b = np.array([float(np.float32(x)) for x in lr.BETA[:K]])
        mag = (a * sums[4::4] / sums[0] + b * a * sums[5::4] / sums[1]) / K
        tol = U * np.abs(d) + 2.0 ** -48 * mag
    assert abs(loss - L) <= U * abs(L), (what, loss, L)
    if dth is not None:
        assert np.all(np.abs(dth - d) <= tol), (what, dth, d)


def check_g(g, B, K, r64, r32, gbound, s, t, what):
    v = lr.vmin(s, K)
    near = v < 80
    err = np.abs(g.astype(np.float64) - r64.g)
    assert np.all(np.isfinite(g)), what
    assert np.all(err[near] <= gbound[near]), f"{what}: g off by up to {(err[near] / gbound[near]).max():.2f} of the rounding bound"
    out = {}
    for lo, hi in lr.BANDS:
        m = (v >= lo) & (v < hi)
        if m.sum() >= fu.REGION_ROWS:
            out[(lo, hi)] = fu.ratios(g[m], r64.g[m], r32.g[m])
    bad = {k: r for k, r in out.items() if not (r[0] <= fu.RMS_MAX and r[1] <= fu.MAX_MAX)}
    assert not bad, f"{what}: g above {fu.RMS_MAX} / {fu.MAX_MAX} fp32 units in bands {bad} (all: {out})"
    if (~near).any():
        # the reference's magnitude at |v_k| = 80 for every k (0.1 % for the roundings of the float32 evaluation)
        a = float(np.float32(lr.ALPHA))
        d80 = np.exp(-80.0) / (1 + np.exp(-80.0)) ** 2
        coef = sum(np.where(t > 0.5, a / (r64.sums[0] * K), float(np.float32(lr.BETA[k])) * a / (r64.sums[1] * K)) for k in range(K))
        assert np.all(np.abs(g[~near]) <= 1.001 * d80 * coef[~near]), what
    return out


CASES = [(B, 0) for B in lr.BATCHES] + [(1025, 1), (4096, 1)]


@pytest.mark.parametrize("B,offset", CASES)
def test_softcdet_sums_loss_and_gradient(hip_lib, B, offset):
    from neuralplda_amd import ops
    for K in (1, 2, 3, 4):
        s, t, r64, r32, sb, gb = reference(B, K, "soft")
        S, T = device_pair(s, t, offset)
        ths = thetas(K)
        sums = ops.loss_sums(S, T, ths, lr.ALPHA, ops.LOSS_SOFTCDET)
        two = ops.loss_finish(S, T, ths, lr.BETA[:K], lr.ALPHA, ops.LOSS_SOFTCDET, sums) + (sums,)
        one = ops.loss_fwd_bwd(S, T, ths, lr.BETA[:K], lr.ALPHA, ops.LOSS_SOFTCDET)
        for form, (loss, g, dth, sm) in (("sums + finish", two), ("fwd_bwd", one)):
            what = f"SoftCdet {form} B={B}{'+1' if offset else ''} K={K}"
            sm, g, dth = sm.cpu().numpy(), g.cpu().numpy(), dth.cpu().numpy().astype(np.float64)
            worst = check_sums(sm, r64, sb, what)
            if B < 2:
                continue
            check_scalars(sm, float(loss.item()), dth, K, "soft", what)
            bands = check_g(g, B, K, r64, r32, gb, s, t, what)
            print(f"{what}: sums {worst:.3f} of the bound; g " +
                  " ".join(f"[{lo},{hi}) {r[0]:.2f}/{r[1]:.2f}" for (lo, hi), r in bands.items()))


@pytest.mark.parametrize("B,offset", CASES)
def test_hard_cdet_counts_are_exact(hip_lib, B, offset):
    from neuralplda_amd import ops
    for K in (1, 2, 3, 4):
        s, t, r64, _, _, _ = reference(B, K, "hard")
        S, T = device_pair(s, t, offset)
        ths = thetas(K)
        sums = ops.loss_sums(S, T, ths, 0.0, ops.LOSS_HARD_CDET)
        sm = sums.cpu().numpy()
        assert np.array_equal(sm, r64.sums), (B, K, sm, r64.sums)
        if B >= 64:  # the scores equal to theta_k are neither a miss nor a false alarm: the counts leave them out
            for k in range(K):
                eq_t = np.sum((s == np.float32(lr.THETA[k])) & (t > 0.5))
                eq_n = np.sum((s == np.float32(lr.THETA[k])) & (t < 0.5))
                assert eq_t >= 3 and eq_n >= 3
                assert sm[2 + 4 * k] == np.sum((s <= np.float32(lr.THETA[k])) & (t > 0.5)) - eq_t
                assert sm[3 + 4 * k] == np.sum((s >= np.float32(lr.THETA[k])) & (t < 0.5)) - eq_n
        if B >= 2:
            loss, _, _ = ops.loss_finish(S, T, ths, lr.BETA[:K], 0.0, ops.LOSS_HARD_CDET, sums, want_grad=False)
            check_scalars(sm, float(loss.item()), None, K, "hard", f"hard Cdet B={B} K={K}")


@pytest.mark.parametrize("B,offset", CASES)
def test_bce_sums_loss_and_gradient(hip_lib, B, offset):
    from neuralplda_amd import ops
    s, t, r64, r32, sb, _ = reference(B, 1, "bce")
    S, T = device_pair(s, t, offset)
    ths = thetas(1)
    sums = ops.loss_sums(S, T, ths, 0.0, ops.LOSS_BCE)
    two = ops.loss_finish(S, T, ths, [], 0.0, ops.LOSS_BCE, sums) + (sums,)
    one = ops.loss_fwd_bwd(S, T, ths, [], 0.0, ops.LOSS_BCE)
    for form, (loss, g, dth, sm) in (("sums + finish", two), ("fwd_bwd", one)):
        what = f"BCE {form} B={B}{'+1' if offset else ''}"
        sm, g, dth = sm.cpu().numpy(), g.cpu().numpy(), dth.cpu().numpy().astype(np.float64)
        worst = check_sums(sm, r64, sb, what)
        check_scalars(sm, float(loss.item()), dth, 1, "bce", what)
        # g_i = (p - t) / N: p to c_p = 4 + |x| roundings (loss_ref.bce_sum_bound), the difference, 1 / N and the product
        x = s.astype(np.float64) - float(np.float32(lr.THETA[0]))
        p = 1.0 / (1.0 + np.exp(-x))
        gb = U * 1.001 * ((4 + np.abs(x)) * p + 3 * np.abs(r64.g) * B) / B
        err = np.abs(g - r64.g)
        assert np.all(err <= gb), f"{what}: g off by up to {(err / gb).max():.2f} of the rounding bound"
        r = fu.ratios(g, r64.g, r32.g) if B >= fu.REGION_ROWS else (0.0, 0.0)
        assert r[0] <= fu.RMS_MAX and r[1] <= fu.MAX_MAX, (what, r)
        print(f"{what}: sums {worst:.3f} of the bound; g {r[0]:.2f}/{r[1]:.2f}")


def test_bce_saturation(hip_lib):
    """Outside |s - theta| <= 8 the kernel restates torch's float32 binary_cross_entropy(sigmoid(x), t), saturation
    included (tests/test_loss_adam_ref_cpu.py confirms these three against torch on the CPU): p rounds to 1 from x ~ 17, so
    a non-target at x = +20 costs the clamp, exactly 100, not 20; a target at x = -120 has p = 0 and costs exactly 100; a
    target at x = -20 costs 20 to one float32 ulp."""
    from neuralplda_amd import ops
    th = [torch.tensor([0.25], dtype=torch.float32, device="cuda")]
    for x, tgt, want, tol in ((20.0, 0.0, 100.0, 0.0), (-120.0, 1.0, 100.0, 0.0), (-20.0, 1.0, 20.0, float(np.spacing(np.float32(20.0))))):
        S = torch.tensor([0.25 + x], dtype=torch.float32, device="cuda")
        T = torch.tensor([tgt], dtype=torch.float32, device="cuda")
        sm = ops.loss_sums(S, T, th, 0.0, ops.LOSS_BCE).cpu().numpy()
        assert abs(sm[2] - want) <= tol, (x, tgt, sm)
        sm2 = ops.loss_fwd_bwd(S, T, th, [], 0.0, ops.LOSS_BCE)[3].cpu().numpy()
        assert abs(sm2[2] - want) <= tol, (x, tgt, sm2)


@pytest.mark.parametrize("B", [1003, 4096])
def test_loss_inside_the_fused_train_step(hip_lib, B):
    """ops.train_step at D = 150 with K = 4 thresholds (the `else` arm of the loss tail's K dispatch): `lbuf` and the
    dL/dtheta it reports in grad_out[n:], against loss_ref on the fp64 oracle's scores.  The step's own scores are not
    visible, so the tolerance has a term for them: the forward kernels are held to 5 fp32 units (max) of the oracle
    (tests/test_fp32_units_fwd_gpu.py), delta = 5 max|forward32 - forward64|; to first order (alpha delta ~ 1e-5, 1 % on top)
    |dL| <= delta sum_i |g_i| and |d dtheta_k| <= alpha delta (alpha D_t_k / N_t + beta_k alpha D_n_k / N_n) / K, since
    |sigma''| <= sigma'.  To that the rounding bound of the sums (propagated through softcdet_scalars) and one float32
    rounding of the result are added."""
    from neuralplda_amd import ops
    from oracle import nplda_oracle as orc
    D, K = 150, 4
    rng = np.random.default_rng(B)
    k1, k2 = 1 / np.sqrt(512), 1 / np.sqrt(D)
    p = orc.Params(rng.uniform(-k1, k1, (D, 512)).astype(np.float32), rng.uniform(-k1, k1, D).astype(np.float32),
                   rng.uniform(-k2, k2, (D, D)).astype(np.float32), rng.uniform(-k2, k2, D).astype(np.float32),
                   rng.uniform(0, 1, D).astype(np.float32), rng.uniform(0, 1, D).astype(np.float32))
    prm = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in p.tensors()]
    x1 = rng.standard_normal((B, 512)).astype(np.float32)
    x2 = rng.standard_normal((B, 512)).astype(np.float32)
    t = (rng.random(B) < 0.15).astype(np.float32)
    t[0], t[-1] = 1.0, 0.0
    s64 = orc.forward(x1, x2, p, np.float64)
    delta = 5 * np.abs(orc.forward(x1, x2, p, np.float32).astype(np.float64) - s64).max()
    # thresholds around the scores' median, spaced as loss_ref.THETA, so that the sigmoids are in their steep part
    theta = [float(np.float32(np.median(s64) + x - lr.THETA[0])) for x in lr.THETA]
    ths = [torch.tensor([x], dtype=torch.float32, device="cuda") for x in theta]
    packed = ops.pack_params(*prm)
    n = int(sum(q.numel() for q in prm))
    m, v, step = torch.zeros(n + K, device="cuda"), torch.zeros(n + K, device="cuda"), torch.zeros(2, device="cuda")
    out, lbuf = torch.zeros(n + K, device="cuda"), torch.zeros((), device="cuda")
    ws = ops.train_step_workspace(B, packed)
    ops.train_step(torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda(), torch.from_numpy(t).cuda(), prm, ths, lr.BETA, lr.ALPHA,
                   ops.LOSS_SOFTCDET, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1e-5, packed, ws, lbuf, grad_out=out)
    # the reference on the oracle's scores, in float64 throughout (loss_ref rounds its scores to float32: done by hand)
    a = float(np.float32(lr.ALPHA))
    b = np.array([float(np.float32(x)) for x in lr.BETA])
    nt, nn = t.sum(dtype=np.float64), (1 - t).sum(dtype=np.float64)
    sums = np.zeros(2 + 4 * K)
    sums[0], sums[1] = nt, nn
    gabs = np.zeros(B)
    for k in range(K):
        vk = a * (theta[k] - s64)
        e = np.exp(-np.abs(vk))
        inv = 1 / (1 + e)
        d = e * inv * inv
        sums[2 + 4 * k:6 + 4 * k] = [np.sum(np.where(vk >= 0, inv, e * inv) * t), np.sum(np.where(vk >= 0, e * inv, inv) * (1 - t)),
                                     np.sum(d * t), np.sum(d * (1 - t))]
        gabs += d * np.where(t > 0.5, a / (nt * K), b[k] * a / (nn * K))
    L, dth = lr.softcdet_scalars(sums, lr.BETA, lr.ALPHA, K)
    sb = lr.softcdet_sum_bound(s64.astype(np.float32), t, theta, lr.ALPHA)
    mag = (a * sums[4::4] / nt + b * a * sums[5::4] / nn) / K
    tol_L = 1.01 * delta * gabs.sum() + sum((sb[2 + 4 * k] / nt + b[k] * sb[3 + 4 * k] / nn) / K for k in range(K)) + U * abs(L)
    tol_d = 1.01 * a * delta * mag + a * (sb[4::4] / nt + b * sb[5::4] / nn) / K + U * mag
    got_L, got_d = float(lbuf.item()), out[n:].cpu().numpy().astype(np.float64)
    print(f"train_step loss B={B}: |dL| {abs(got_L - L):.2e} of {tol_L:.2e}; |d dtheta| / tol {np.abs(got_d - dth) / tol_d}")
    assert abs(got_L - L) <= tol_L, (got_L, L, tol_L)
    assert np.all(np.abs(got_d - dth) <= tol_d), (got_d, dth, tol_d)


@pytest.mark.parametrize("D1,B", [(24, 100), (170, 777)])
def test_loss_inside_the_dplda_update(hip_lib, D1, B):
    """ops.dplda_update_loss: the loss block that rides in the weighted-moments launch.  Its sums are not returned, so `loss`
    and `dtheta` are held to the float64 reference within the rounding bound of the sums propagated through
    softcdet_scalars, plus one float32 rounding of the result."""
    from neuralplda_amd import ops
    K = 2
    s, t = lr.make_scores(B, K, seed=D1)
    r64 = lr.softcdet(s, t, lr.THETA[:K], lr.BETA[:K], lr.ALPHA, np.float64)
    sb = lr.softcdet_sum_bound(s, t, lr.THETA[:K], lr.ALPHA)
    rng = np.random.default_rng(D1)
    n = 2 * D1 * D1 + D1
    paired = torch.from_numpy(rng.standard_normal((B, 2 * D1)).astype(np.float32)).cuda()
    wlr = torch.from_numpy((0.05 * rng.standard_normal(n)).astype(np.float32)).cuda()
    blr = torch.zeros(1, device="cuda")
    m, v, step = torch.zeros(n + 1, device="cuda"), torch.zeros(n + 1, device="cuda"), torch.zeros(2, device="cuda")
    res = ops.dplda_update_loss(paired, torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), thetas(K), lr.BETA[:K], lr.ALPHA,
                                ops.LOSS_SOFTCDET, wlr, blr, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1e-5)
    assert res is not None
    loss, dth = float(res[0].item()), res[1].cpu().numpy()[:K].astype(np.float64)
    a = float(np.float32(lr.ALPHA))
    b = np.array([float(np.float32(x)) for x in lr.BETA[:K]])
    nt, nn = r64.sums[0], r64.sums[1]
    mag = (a * r64.sums[4::4] / nt + b * a * r64.sums[5::4] / nn) / K
    tol_L = sum((sb[2 + 4 * k] / nt + b[k] * sb[3 + 4 * k] / nn) / K for k in range(K)) + U * abs(r64.loss)
    tol_d = a * (sb[4::4] / nt + b * sb[5::4] / nn) / K + U * mag
    print(f"dplda_update_loss D1={D1} B={B}: |dL| / tol {abs(loss - r64.loss) / tol_L:.3f}; |d dtheta| / tol {np.abs(dth - r64.dtheta) / tol_d}")
    assert abs(loss - r64.loss) <= tol_L, (loss, r64.loss, tol_L)
    assert np.all(np.abs(dth - r64.dtheta) <= tol_d), (dth, r64.dtheta, tol_d)
