"""The detection-cost sweep (nplda_detcost_sweep_f32, csrc/nplda_detcost.hip) against its NumPy twin (tests/detcost_ref.py)
at labels outside {0, 1}, empty classes, ties, special values, NaN scores and every reduction boundary of the arg-min.

Reference mode: minc, minc_avg and thr are bit-equal to the twin (the kernel's __fdiv_rn / __fmul_rn / __fadd_rn leave no
freedom; a zero threshold is compared with ==).  Exact mode: thr is equal, minc, minc_avg and eer lie within half a float32
ulp, times (1 + 2^-20), of the twin's exact rational — one float64 evaluation rounded once — under the precondition,
asserted on the twin, that the exact costs of different counts are either tied or at least 1e-9 apart (relative), so that
a float64 evaluation cannot reorder the candidates."""
import os

import numpy as np
import pytest
import torch

from tests import detcost_cases as cases
from tests import detcost_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gpu_sweep(s, t, betas, exact):
    from neuralplda_amd import ops
    S = torch.from_numpy(np.ascontiguousarray(s, dtype=F32)).cuda()
    T = torch.from_numpy(np.ascontiguousarray(t, dtype=F32)).cuda()
    mc, th, avg, e = ops.detcost_sweep(S, T, betas, exact=exact, want_eer=exact)
    return mc.cpu().numpy(), th.cpu().numpy(), avg.cpu().numpy()[0], (e.cpu().numpy()[0] if exact else None)


def bits(a):
    return np.asarray(a, F32).reshape(-1).view(np.uint32)


def same_thr(got, want):
    """Equal float32 thresholds: bit-equal, except that a zero is compared with == (either sign) and NaN matches NaN."""
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    return bool(np.all((bits(got) == bits(want)) | ((want == 0) & (got == 0)) | (np.isnan(want) & np.isnan(got))))


def same_val(got, want):
    """Bit-equal float32 values; any NaN matches any NaN (the payload of 0/0 is not part of the contract)."""
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(want) & np.isnan(got))))


def check_reference(s, t, betas):
    want = ref.sweep(s, t, betas, exact=False)
    mc, th, avg, _ = gpu_sweep(s, t, betas, exact=False)
    print("reference mode: minc", mc, want["minc"], "thr", th, want["thr"], "avg", avg, want["minc_avg"])
    assert same_val(mc, want["minc"]) and same_val(avg, want["minc_avg"]) and same_thr(th, want["thr"])
    return mc, th, avg


def check_exact(s, t, betas):
    want = ref.sweep(s, t, betas, exact=True)
    # precondition on the twin: no two candidates with different counts closer than 1e-9 (relative) unless truly tied
    assert all(g == 0.0 or g >= 1e-9 for g in want["gap"]), want["gap"]
    mc, th, avg, eer = gpu_sweep(s, t, betas, exact=True)
    print("exact mode: minc", mc, want["minc"], "thr", th, want["thr"], "avg", avg, want["minc_avg"], "eer", eer, want["eer"])
    assert same_thr(th, want["thr"])
    for k in range(len(betas)):
        assert ref.within_rounding(mc[k], want["minc_exact"][k]), (k, mc[k], want["minc"][k])
    assert ref.within_rounding(avg, want["minc_avg_exact"]), (avg, want["minc_avg"])
    assert ref.within_rounding(eer, want["eer"]), (eer, want["eer"])
    return mc, th, avg, eer


@pytest.mark.parametrize("n", [1, 2, 17, 255, 256, 257, 4097])
def test_labels_outside_0_and_1(hip_lib, n):
    """Labels from {0, 0.25, 0.5, 0.75, 1}, a quarter of them 0.5: reference mode divides by the label SUMS over all trials
    (exact in float32 here), exact mode by the class counts; trials labelled 0.5 are in neither class."""
    for quant in (None, 0.25):
        s, t = cases.mixed_labels(n, 100 + n, quant=quant)
        assert (t == 0.5).sum() * 4 >= n and (n < 5 or all((t == v).any() for v in (0.0, 0.25, 0.75, 1.0)))
        check_reference(s, t, cases.BETAS)
        check_exact(s, t, cases.BETAS)


def test_reference_golden_g5b(hip_lib):
    """The reference's own minc on 256 trials with labels from {0, 0.25, 0.5, 0.75, 1} (golden G5b), bit for bit."""
    from neuralplda_amd import metrics
    g = np.load(os.path.join(G, "g5b_metrics_labels.npz"))
    betas = [float(b) for b in g["beta"]]
    mc, th = metrics.minc(torch.from_numpy(g["s"]).cuda(), torch.from_numpy(g["t"]).cuda(), betas)
    print("G5b minc", mc.item(), float(g["minc"]), "thr", [th[b].item() for b in betas], g["minc_th"])
    assert same_val(mc.item(), g["minc"])
    assert same_thr([th[b].item() for b in betas], g["minc_th"])


@pytest.mark.parametrize("name", sorted(cases.composition_cases()))
def test_class_composition(hip_lib, name):
    """N = 0, empty classes and the two-trial problems: the NaN / inf results are the twin's (reference mode with no
    non-target divides by sum (1 - t) = 0 as the reference does)."""
    s, t = cases.composition_cases()[name]
    for betas in ([1.0], cases.BETAS):
        check_reference(s, t, betas)
        check_exact(s, t, betas)


@pytest.mark.parametrize("name", sorted(cases.special_value_cases()))
def test_ties_and_special_values(hip_lib, name):
    s, t = cases.special_value_cases()[name]
    for betas in ([1.0], cases.BETAS):
        check_reference(s, t, betas)
        check_exact(s, t, betas)


@pytest.mark.parametrize("n", cases.BOUNDARY_SIZES)
def test_first_occurrence_zigzag(hip_lib, n):
    """Alternating non-target / target scores, beta = 1: the minimum is taken at thresholds spread over the whole sorted
    array — every lane, wave, block and grid-stride pass holds one — and the first must win (tests/test_detcost_cpu.py
    derives the answers by hand)."""
    s, t, P = cases.zigzag(n)
    _, th, _ = check_reference(s, t, [1.0])
    mc, the, _, eer = check_exact(s, t, [1.0])
    assert the[0] == (1.0 if n > 2 * P else 2.0) and mc[0] == F32(1) - F32(1) / F32(P) and eer == 0.5
    assert n != 2 * P or th[0] == 6.0


@pytest.mark.parametrize("n", cases.BOUNDARY_SIZES)
def test_first_occurrence_separated(hip_lib, n):
    """Scores 0 .. n-1, targets from j on: the single exact-mode optimum sits at sorted position j, placed on each side of
    every reduction boundary."""
    for j in cases.separated_positions(n):
        s, t = cases.separated(n, j)
        check_reference(s, t, [99.0])
        mc, th, _, eer = check_exact(s, t, [1.0, 99.0])
        assert list(th) == [j, j] and list(mc) == [0.0, 0.0] and (j == 0 or eer == 0.0)


def test_betas(hip_lib):
    """K = 1, K = 8 with a repeated value, beta = 0, 2^-20 and 2^40; K = 9 raises."""
    from neuralplda_amd import _lib, ops
    eight = [99.0, 0.0, 2.0 ** -20, 2.0 ** 40, 99.0, 1.0, 9.9, 199.0]
    for s, t in (cases.binary(1000, 7, quant=0.05), cases.mixed_labels(257, 8)):
        for betas in ([99.0], [0.0], [2.0 ** -20], [2.0 ** 40], eight):
            mc, th, _ = check_reference(s, t, betas)
            mce, the, _, _ = check_exact(s, t, betas)
        assert bits(mc)[0] == bits(mc)[4] and bits(th)[0] == bits(th)[4]
        assert bits(mce)[0] == bits(mce)[4] and bits(the)[0] == bits(the)[4]
    # sum (1 - t) = 0.25 here but no non-target: beta = 0 meets 1.0 / 0.25 and stays finite; with only labels of 1 the
    # product is 0 * inf, a NaN cost, which never wins: minc and threshold are NaN
    so, to = cases.composition_cases()["only_targets"]
    mc, th, _ = check_reference(so, to, [0.0, 1.0])
    assert mc[0] == 0.0 and mc[1] == 4.0
    mc, th, _ = check_reference(so, np.ones(4, F32), [0.0, 1.0])
    assert np.isnan(mc[0]) and np.isnan(th[0]) and np.isinf(mc[1]) and th[1] == 1.0
    S, T = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    with pytest.raises(_lib.NpldaHipError):
        ops.detcost_sweep(S, T, [1.0] * 9)
    with pytest.raises(_lib.NpldaHipError):
        ops.detcost_sweep(S, T, [1.0] * 9, exact=True)


@pytest.mark.parametrize("name", sorted(cases.eer_cases()))
def test_eer_branches(hip_lib, name):
    from neuralplda_amd import metrics
    s, t = cases.eer_cases()[name]
    _, _, _, eer = check_exact(s, t, [1.0])
    assert metrics.eer(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()) == float(eer)


@pytest.mark.parametrize("n,kind", cases.NAN_CASES)
def test_nan_scores(hip_lib, n, kind):
    """A trial whose score is NaN (either sign, either class) is in neither class and disturbs no other trial's counts; in
    reference mode its label still enters the normalisers.  The same problem with those trials labelled 0.5 and scored 0
    gives the same bits: everywhere in exact mode, and in reference mode whenever the relabelling keeps the label sums
    (every kind but the NaN on a target labelled 1; there the thresholds stay)."""
    s, t, mask = cases.with_nans(n, n, kind)
    s2, t2 = cases.nans_replaced(s, t, mask)
    a = check_reference(s, t, cases.BETAS)
    b = check_reference(s2, t2, cases.BETAS)
    assert same_thr(a[1], b[1])
    if kind != "one_target":
        assert np.array_equal(bits(a[0]), bits(b[0])) and bits(a[2])[0] == bits(b[2])[0]
    a = check_exact(s, t, cases.BETAS)
    b = check_exact(s2, t2, cases.BETAS)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_layout_and_determinism(hip_lib):
    """Non-contiguous and CPU inputs through metrics.minc; two calls give identical bytes."""
    from neuralplda_amd import metrics
    s, t = cases.mixed_labels(4097, 11, quant=0.125)
    want = ref.sweep(s, t, cases.BETAS, exact=False)
    wide_s, wide_t = np.zeros((4097, 3), F32), np.full((4097, 3), 0.5, F32)
    wide_s[:, 1], wide_t[:, 1] = s, t
    for dev in ("cpu", "cuda"):
        S, T = torch.from_numpy(wide_s).to(dev)[:, 1], torch.from_numpy(wide_t).to(dev)[:, 1]
        assert not S.is_contiguous()
        outs = []
        for _ in range(2):
            mc, th = metrics.minc(S, T, cases.BETAS)
            mce, the = metrics.minc_exact(S, T, cases.BETAS)
            assert mc.device.type == dev
            outs.append(np.asarray([mc.item(), mce.item()] + [th[b].item() for b in cases.BETAS]
                                   + [the[b].item() for b in cases.BETAS], F32))
        assert outs[0].tobytes() == outs[1].tobytes()
        assert same_val(outs[0][0], want["minc_avg"]) and same_thr(outs[0][2:5], want["thr"])
