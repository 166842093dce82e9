"""The NumPy twin of the detection-cost sweep (tests/detcost_ref.py) against an O(N^2) restatement, the oracle, the
reference's own outputs on labels outside {0, 1} (golden G5b) and hand-derived answers for every planted case of
tests/detcost_cases.py — so that a wrong twin cannot pass silently in tests/test_detcost_gpu.py.  Then the library without
a device: the workspace size and every status code of nplda_detcost_sweep_f32."""
import math
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import nplda_oracle as orc
from tests import detcost_cases as cases
from tests import detcost_ref as ref

F32 = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN, INF = math.nan, math.inf


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).reshape(-1).view(np.uint32), np.asarray(b, F32).reshape(-1).view(np.uint32))


def same_f32(a, b):
    """Equal float32 values, NaN equal to NaN and -0.0 equal to +0.0."""
    a, b = np.asarray(a, F32).reshape(-1), np.asarray(b, F32).reshape(-1)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_twin_equals_brute_force():
    """200 seeded problems of N <= 200, labels from {0, 0.25, 0.5, 0.75, 1}, scores on a coarse grid (ties are common)."""
    rg = np.random.default_rng(2024)
    seen_ties = 0
    for _ in range(200):
        n = int(rg.integers(0, 201))
        t = cases.LABELS[rg.integers(0, 5, n)]
        s = (np.round((rg.standard_normal(n) + (t > 0.5)) * 4) / 4).astype(F32)
        seen_ties += int(np.unique(s).size < n)
        betas = [99.0, 9.9, 1.0][:int(rg.integers(1, 4))]
        got = ref.sweep(s, t, betas, exact=False)
        minc, thr, avg = ref.brute(s, t, betas)
        assert same_bits(got["minc"], minc) and same_bits(got["thr"], thr) and same_bits(got["minc_avg"], avg), (n, betas)
    assert seen_ties > 150


def test_twin_equals_oracle_on_binary_labels():
    """On 0/1 labels without infinite scores the twin, minc_reference, minc_exact and eer define the same numbers."""
    for n, seed, quant in [(2, 1, None), (17, 2, None), (200, 3, 0.25), (1000, 4, 0.05), (4097, 5, None)]:
        s, t = cases.binary(n, seed, quant=quant)
        r = ref.sweep(s, t, cases.BETAS, exact=False)
        mc, th = orc.minc_reference(s, t, cases.BETAS)
        assert same_bits(r["minc_avg"], mc) and same_bits(r["thr"], [th[b] for b in cases.BETAS])
        betas32 = [float(F32(b)) for b in cases.BETAS]  # the sweep takes float32 betas; the oracle any float
        e = ref.sweep(s, t, betas32, exact=True)
        mce, the = orc.minc_exact(s, t, betas32)
        assert abs(e["minc_avg"] - mce) <= 1e-12 and same_bits(e["thr"], [the[b] for b in betas32])
        assert abs(e["eer"] - orc.eer(s, t)) <= 1e-12
        assert all(g == 0.0 or g >= 1e-9 for g in e["gap"])


def test_twin_keeps_accept_nothing_apart_from_an_infinite_score():
    """The one deliberate difference from the oracle: with a score of +inf, np.unique merges the accept-nothing point
    (P_miss = 1, P_fa = 0) into that score (P_fa > 0 when a non-target sits there).  The twin, like the kernel, keeps both."""
    s, t = np.asarray([np.inf, 0.0], F32), np.asarray([0.0, 1.0], F32)
    e = ref.sweep(s, t, [3.0], exact=True)
    assert e["minc_exact"] == [Fr(1)] and e["thr"][0] == np.inf  # accept nothing: 1 + 3 * 0
    mce, the = orc.minc_exact(s, t, [3.0])
    assert mce == 3.0 and the[3.0] == 0.0  # the oracle only sees 0 -> 3 and +inf -> 1 + 3


def test_twin_equals_reference_golden_g5b():
    """G5b is NeuralPlda.minc itself on 256 trials with labels from {0, 0.25, 0.5, 0.75, 1}: bit for bit."""
    g = np.load(os.path.join(G, "g5b_metrics_labels.npz"))
    assert g["minc"].dtype == np.float32 and set(np.unique(g["t"])) == {0.0, 0.25, 0.5, 0.75, 1.0}
    r = ref.sweep(g["s"], g["t"], list(g["beta"]), exact=False)
    assert same_bits(r["minc_avg"], g["minc"]) and same_bits(r["thr"], g["minc_th"])
    # the class counts as normalisers (what the sweep divided by before) give another number
    k = g["t"] != 0.5
    wrong, _ = orc.minc_reference(g["s"][k], (g["t"][k] > 0.5).astype(F32), list(g["beta"]))
    assert abs(float(wrong) - float(g["minc"])) > 0.1


def test_issue_example_label_sums_versus_counts():
    """64 trials, 16 targets, 16 labels of 0.5: the normalisers are 24 and 40, not 16 and 32."""
    t = np.concatenate([np.ones(16), np.full(16, 0.5), np.zeros(32)]).astype(F32)
    assert tuple(ref.normalisers(t)) == (24.0, 40.0)
    assert tuple(ref.normalisers(np.asarray([0.25, 0.75, 1.0], F32))) == (2.0, 1.0)


# name -> reference mode (minc, thr), exact mode (minc, thr, eer); beta = 1.  Derived by hand from the definitions in
# tests/detcost_ref.py's docstring (counts below each case).
HAND = {
    "empty": ((NAN, NAN), (Fr(0), INF, NAN)),
    "one_target": ((INF, 2.0), (Fr(0), 2.0, NAN)),               # 1/1 + 1 * (1.0 / 0)
    "one_nontarget": ((NAN, NAN), (Fr(0), INF, NAN)),
    "one_excluded": ((NAN, NAN), (Fr(0), 2.0, NAN)),
    "only_targets": ((4.0, 2.0), (Fr(0), 1.0, NAN)),             # sums 3.75 / 0.25: rank 1 costs 0 / 3.75 + 1.0 / 0.25
    "only_nontargets": ((NAN, NAN), (Fr(0), INF, NAN)),
    "only_excluded": ((NAN, NAN), (Fr(0), 1.0, NAN)),
    "tgt_above_non": ((2.0, 1.0), (Fr(0), 1.0, 0.0)),            # both sets empty: 1.0 / 1 + 1.0 / 1
    "non_above_tgt": ((1.0, 0.0), (Fr(1), 0.0, 1.0)),            # one non-target at or above: index 0
    "non_first_tgt_above": ((2.0, 1.0), (Fr(0), 1.0, 0.0)),
    "tgt_equals_non": ((1.0, 1.0), (Fr(1), 1.0, 0.5)),           # exact: accept all (1) ties with accept nothing (1)
    "all_equal": ((1.0, 0.5), (Fr(1), 0.5, 0.5)),                # 1.0 / 2 + 1 / 2
    "all_equal_257": ((float(F32(F32(1) / F32(86)) + F32(F32(170) / F32(171))), -1.25), (Fr(1), -1.25, 0.5)),
    "three_values": ((0.25, 0.0), (Fr(7, 10), 0.0, 5 / 13)),
    "signed_zeros": ((0.75, 0.0), (Fr(3, 4), 0.0, 0.375)),
    "infinities": ((0.5, -1.0), (Fr(1), -INF, 0.5)),
    "subnormals": ((0.25, 1e-45), (Fr(3, 4), 1e-45, 5 / 12)),
    "largest_finite": ((0.0, 1.0), (Fr(1, 2), 1.0, 0.25)),
    "zero_at_crossing": (None, (Fr(3, 4), 1.0, 0.5)),
    "no_crossing": (None, (Fr(1), 1.0, 0.5)),
    "no_crossing_several_scores": (None, (Fr(1), 0.0, 0.5)),
    "separated": (None, (Fr(0), 2.0, 0.0)),
    "reversed": (None, (Fr(1), 0.0, 1.0)),
    "tie_run_straddles": (None, (Fr(3, 5), 3.0, 1 / 3)),
    "interpolated": (None, (Fr(8, 15), 5.0, 1 / 3)),
}


def _planted():
    d = {}
    d.update(cases.composition_cases())
    d.update(cases.special_value_cases())
    d.update(cases.eer_cases())
    return d


@pytest.mark.parametrize("name", sorted(HAND))
def test_planted_cases_by_hand(name):
    s, t = _planted()[name]
    want_ref, (mc, th, eer) = HAND[name]
    e = ref.sweep(s, t, [1.0], exact=True)
    assert e["minc_exact"] == [mc] and same_f32(e["thr"], [th]) and e["minc_avg_exact"] == mc
    assert (math.isnan(eer) and math.isnan(e["eer"])) or abs(e["eer"] - eer) <= 1e-15
    if want_ref is not None:
        r = ref.sweep(s, t, [1.0], exact=False)
        assert same_f32(r["minc"], [want_ref[0]]) and same_f32(r["thr"], [want_ref[1]]) and same_f32(r["minc_avg"], want_ref[0])
    if s.size <= 200:
        r = ref.sweep(s, t, [1.0, 9.9], exact=False)
        minc, thr, avg = ref.brute(s, t, [1.0, 9.9])
        assert same_bits(r["minc"], minc) and same_f32(r["thr"], thr) and same_bits(r["minc_avg"], avg)


def test_every_planted_case_has_a_hand_answer():
    assert set(HAND) == set(_planted())


@pytest.mark.parametrize("n", cases.BOUNDARY_SIZES)
def test_zigzag_by_hand(n):
    """beta = 1, P targets and P non-targets alternating.  Exact mode: every target position costs (P - 1) / P, every other
    threshold 1: the first is sorted position 1, or the excluded score 1 in front of it, which has the same counts.
    Reference mode with n = 2 P: target ranks 1 .. P - 2 cost (r - 1) / P + (P - r - 2) / P = (P - 3) / P, ranks 0 and P - 1
    cost (P - 1) / P: rank 1 (score 6) wins.  The EER crossing has P_miss = P_fa = 1/2 exactly."""
    s, t, P = cases.zigzag(n)
    assert P & (P - 1) == 0 and 2 * P <= n < 4 * P and (t > 0.5).sum() == P == (t < 0.5).sum()
    e = ref.sweep(s, t, [1.0], exact=True)
    assert e["minc_exact"] == [Fr(P - 1, P)] and e["thr"][0] == (1.0 if n > 2 * P else 2.0) and e["eer"] == 0.5
    assert e["gap"] == [0.0]  # true ties, exact in any evaluation
    if n == 2 * P:  # the normalisers are P: every quotient is exact (with excluded trials they are n / 2 and round)
        r = ref.sweep(s, t, [1.0], exact=False)
        assert r["thr"][0] == 6.0 and Fr(float(r["minc"][0])) == Fr(P - 3, P)


@pytest.mark.parametrize("n", cases.BOUNDARY_SIZES)
def test_separated_by_hand(n):
    """Non-targets on 0 .. j-1, targets on j .. n-1.  Exact mode: cost 0 at the single threshold j (for j = 0 there is no
    non-target, every threshold costs P_miss and 0 wins again), EER 0.  Reference mode: target rank 1 has "index of the last
    target below" 0 and no non-target at or above (1.0): beta / (j); with a single target rank 0: 1.0 / 1 + beta / j."""
    for j in cases.separated_positions(n):
        s, t = cases.separated(n, j)
        e = ref.sweep(s, t, [1.0, 99.0], exact=True)
        assert e["minc_exact"] == [Fr(0), Fr(0)] and list(e["thr"]) == [j, j]
        assert (math.isnan(e["eer"]) if j == 0 else e["eer"] == 0.0)
        assert all(g > 1e-9 for g in e["gap"]) or j == 0
        if j > 0:
            r = ref.sweep(s, t, [99.0], exact=False)
            pf = F32(F32(1) / F32(j))
            if n - j >= 2:
                assert r["thr"][0] == j + 1 and r["minc"][0] == F32(F32(0) + F32(F32(99) * pf))
            else:
                assert r["thr"][0] == j and r["minc"][0] == F32(F32(1) + F32(F32(99) * pf))


@pytest.mark.parametrize("n,kind", cases.NAN_CASES)
def test_nan_scores_are_excluded_and_keep_their_label_in_the_normalisers(n, kind):
    """A NaN score of either sign takes its trial out of both classes; reference mode still sums its label.  The problem
    with the NaN trials labelled 0.5 and scored 0 has the same answer: everywhere in exact mode; in reference mode wherever
    the relabelling keeps the label sums (every kind but a NaN on a target), else up to the normaliser of P_miss."""
    s, t, mask = cases.with_nans(n, n, kind)
    assert np.isnan(s[mask]).all() and not np.isnan(s[~mask]).any() and mask.sum() >= 1
    bits = set(s[mask].view(np.uint32).tolist())
    assert bits == ({cases.NAN_NEG, cases.NAN_POS} if kind == "many" else {cases.NAN_NEG})
    assert kind != "many" or ((t[mask] > 0.5).any() and (t[mask] < 0.5).any() and 0.08 <= mask.mean() <= 0.12)
    s2, t2 = cases.nans_replaced(s, t, mask)
    a, b = ref.sweep(s, t, cases.BETAS, True), ref.sweep(s2, t2, cases.BETAS, True)
    assert a["minc_exact"] == b["minc_exact"] and same_bits(a["thr"], b["thr"]) and a["eer"] == b["eer"]
    a, b = ref.sweep(s, t, cases.BETAS, False), ref.sweep(s2, t2, cases.BETAS, False)
    if kind != "one_target":
        assert ref.normalisers(t) == ref.normalisers(t2)
        assert same_bits(a["minc"], b["minc"]) and same_bits(a["thr"], b["thr"]) and same_bits(a["minc_avg"], b["minc_avg"])
    else:  # the label 1 of the NaN trial stays in sum t: the costs are those of the sums of ALL labels
        assert ref.normalisers(t)[0] == ref.normalisers(t2)[0] + F32(0.5)
        st, sn = np.sort(s[~mask & (t > 0.5)]), np.sort(s[~mask & (t < 0.5)])
        fnt, fnn = ref.normalisers(t)
        c_lt, c_ge = np.searchsorted(st, st, "left"), sn.size - np.searchsorted(sn, st, "left")
        c = (np.where(c_lt > 0, c_lt - 1, 1).astype(F32) / fnt
             + F32(cases.BETAS[0]) * (np.where(c_ge > 0, c_ge - 1, 1).astype(F32) / fnn))
        assert a["minc"][0] == c.min() and a["thr"][0] == st[int(np.argmin(c))]


@pytest.mark.parametrize("n", [257, 1025, 4097])
def test_every_exclusion_keeps_a_quarter_of_the_trials_in_each_class(n):
    """The input of tests/test_metrics_gpu.py::test_one_trial_rule_in_all_four_families: each way out of a class is planted
    on each kind of label, and what stays is no corner case."""
    s, t = cases.every_exclusion(n, n)
    nan = np.isnan(s)
    assert {cases.NAN_NEG, cases.NAN_POS} <= set(s.view(np.uint32).tolist()) and (s == np.inf).any() and (s == -np.inf).any()
    for lab in (t > 0.5, t < 0.5, t == 0.5, np.isnan(t)):
        assert (lab & nan).any() and (lab & ~nan).any()
    assert 4 * ((t > 0.5) & ~nan).sum() >= n and 4 * ((t < 0.5) & ~nan).sum() >= n
    assert np.unique(s[~nan]).size < n // 2  # ties


def test_a_nan_cost_never_wins():
    """Only labels of 1: sum (1 - t) = 0, the empty non-target set gives 1.0 / 0 = inf, and beta = 0 makes the cost
    0 * inf = NaN at every threshold: no winner, NaN results (the reference's torch.min would return the NaN too, with
    the first target score).  beta = 1 gives inf at the first target."""
    s, t = np.asarray([3.0, 1.0, 2.0, 2.0], F32), np.ones(4, F32)
    r = ref.sweep(s, t, [0.0, 1.0], exact=False)
    assert np.isnan(r["minc"][0]) and np.isnan(r["thr"][0]) and r["minc"][1] == np.inf and r["thr"][1] == 1.0
    assert np.isnan(r["minc_avg"])
    minc, thr, avg = ref.brute(s, t, [0.0, 1.0])
    assert same_f32(minc, r["minc"]) and same_f32(thr, r["thr"]) and np.isnan(avg)


# ---- the library: planning and argument checking need no device -------------------------------------------------------
EINVAL, EUNSUPPORTED, ENOSPC = -22, -95, -28


def test_workspace_bytes(hip_lib):
    f = hip_lib.nplda_detcost_workspace_bytes
    ns = [0, 1, 2, 255, 256, 257, 4099, 1 << 20, 10_000_000, 2 ** 31 - 1]
    sizes = [f(n) for n in ns]
    print("nplda_detcost_workspace_bytes", dict(zip(ns, sizes)))
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    for n in (-1, 2 ** 31, 2 ** 40):
        assert f(n) == 0, n
    # five arrays of N keys, counts and prefixes, and the reservation of N * 14 bytes + 4 MiB for the sort
    assert 46 * (1 << 20) + (4 << 20) <= f(1 << 20) <= 46 * (1 << 20) + (4 << 20) + (1 << 18)


def test_status_codes_of_sweep(hip_lib):
    """Every code is returned before anything is enqueued: no valid call is made."""
    import ctypes
    buf = np.zeros(4096, dtype=np.float64)
    a = buf.ctypes.data
    N = 100
    ws = hip_lib.nplda_detcost_workspace_bytes(N)
    betas = (ctypes.c_float * 9)(*([1.0] * 9))

    def call(s=a, t=a, N=N, b=betas, K=2, exact=0, minc=a, thr=a, avg=a, eer=a, w=a, wb=ws):
        return hip_lib.nplda_detcost_sweep_f32(s, t, N, b, K, exact, minc, thr, avg, eer, w, wb, None)

    for name in ("s", "t", "b", "minc", "thr", "avg", "w"):
        assert call(**{name: None}) == EINVAL, name
    assert call(w=a + 8) == EINVAL  # not aligned to 16 bytes
    assert call(N=-1) == EINVAL and call(K=0) == EINVAL and call(K=-2) == EINVAL
    assert call(K=9) == EUNSUPPORTED and call(N=2 ** 31) == EUNSUPPORTED and call(N=2 ** 40) == EUNSUPPORTED
    for exact in (0, 1):
        assert call(exact=exact, wb=ws - 1) == ENOSPC and call(exact=exact, wb=0) == ENOSPC
    for n in (0, 1):
        assert call(N=n, wb=hip_lib.nplda_detcost_workspace_bytes(n) - 1) == ENOSPC


def test_within_rounding_is_half_an_ulp():
    one = Fr(1)
    assert ref.within_rounding(F32(1.0), one) and ref.within_rounding(F32(1.0), one + Fr(1, 1 << 24))
    assert not ref.within_rounding(np.nextafter(F32(1.0), F32(2.0)), one)
    assert not ref.within_rounding(F32(1.0), one + Fr(1, 1 << 23))
    assert ref.within_rounding(F32(0.0), Fr(0)) and not ref.within_rounding(F32(1e-45), Fr(0))
    assert ref.within_rounding(F32(np.nan), math.nan) and not ref.within_rounding(F32(np.nan), 1.0)
    assert ref.within_rounding(F32(1 / 3), Fr(1, 3)) and not ref.within_rounding(np.nextafter(F32(1 / 3), F32(1)), Fr(1, 3))
