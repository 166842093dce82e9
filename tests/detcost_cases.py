"""Inputs of the detection-cost tests (tests/test_detcost_cpu.py checks the twin on them, tests/test_detcost_gpu.py the
kernel against the twin).  Every builder returns float32 (scores, labels); nothing here knows an expected value."""
import numpy as np

F32 = np.float32
LABELS = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0], F32)
NAN_NEG, NAN_POS = 0xFFC00000, 0x7FC00000  # what inf - inf gives on the host, and the canonical quiet NaN
BETAS = [99.0, 199.0, 9.9]


def nan_from_bits(bits):
    return np.asarray([bits], np.uint32).view(F32)[0]


def mixed_labels(n, seed, quant=None):
    """Labels from {0, 0.25, 0.5, 0.75, 1}: at least a quarter exactly 0.5 and, from n = 5 on, one trial in each other
    class.  Every label sum is a multiple of 0.25 below 2^22, hence exact in float32."""
    rg = np.random.default_rng(seed)
    t = LABELS[rg.integers(0, 5, n)]
    if n >= 5:
        idx = rg.permutation(n)
        t[idx[:4]] = [0.0, 0.25, 0.75, 1.0]
        need = (n + 3) // 4
        rest = idx[4:]
        t[rest[:min(need, rest.size)]] = 0.5
    elif n >= 1:
        t[0] = 0.5
    s = (rg.standard_normal(n) + 2.0 * (t > 0.5)).astype(F32)
    if quant:
        s = (np.round(s / quant) * quant).astype(F32)
    return s, t.astype(F32)


def binary(n, seed, ptgt=0.3, quant=None):
    """0/1 labels with both classes present (n >= 2)."""
    rg = np.random.default_rng(seed)
    t = (rg.random(n) < ptgt).astype(F32)
    t[0], t[1] = 1.0, 0.0
    s = (rg.standard_normal(n) + 2.0 * t).astype(F32)
    if quant:
        s = (np.round(s / quant) * quant).astype(F32)
    return s, t


def zigzag(n, seed=0):
    """Non-target, target, non-target, ... on the scores 0, 2, 4, ... with Nt = Nn = P, the largest power of two with
    2 P <= n; the other n - 2 P trials are excluded (label 0.5) on the odd scores 1, 3, ...  Shuffled.  With beta = 1
    every operation of both modes is exact and the minimum is taken at every other threshold of the whole array."""
    P = 1
    while 4 * P <= n:
        P *= 2
    s = np.concatenate([2.0 * np.arange(2 * P), 2.0 * np.arange(n - 2 * P) + 1.0]).astype(F32)
    t = np.concatenate([np.tile([0.0, 1.0], P), np.full(n - 2 * P, 0.5)]).astype(F32)
    perm = np.random.default_rng(seed).permutation(n)
    return s[perm], t[perm], P


def separated(n, j, seed=0):
    """Scores 0 .. n-1, non-targets below j, targets from j on; shuffled."""
    s = np.arange(n, dtype=F32)
    t = (np.arange(n) >= j).astype(F32)
    perm = np.random.default_rng(seed).permutation(n)
    return s[perm], t[perm]


BOUNDARY_SIZES = [128, 512, 16128, 16384, 16640, 131071, 131072, 131073, 262145]


def separated_positions(n):
    """Sorted positions of the single optimum: lane, wave and block boundaries, the last trial, and one past the first
    grid-stride pass of 512 blocks x 256 threads."""
    return sorted({j for j in (0, 63, 64, 255, 256, n - 1, 131073) if j < n})


def composition_cases():
    """name -> (s, t): empty input, empty classes, and the two-trial problems."""
    f = lambda *v: np.asarray(v, F32)  # noqa: E731
    return {
        "empty": (f(), f()),
        "one_target": (f(2.0), f(1.0)),
        "one_nontarget": (f(2.0), f(0.0)),
        "one_excluded": (f(2.0), f(0.5)),
        "only_targets": (f(3.0, 1.0, 2.0, 2.0), f(1.0, 1.0, 0.75, 1.0)),
        "only_nontargets": (f(3.0, 1.0, 2.0), f(0.0, 0.25, 0.0)),
        "only_excluded": (f(2.0, 1.0), f(0.5, 0.5)),
        "tgt_above_non": (f(1.0, 0.0), f(1.0, 0.0)),
        "non_above_tgt": (f(0.0, 1.0), f(1.0, 0.0)),
        "non_first_tgt_above": (f(0.0, 1.0), f(0.0, 1.0)),
        "tgt_equals_non": (f(1.0, 1.0), f(1.0, 0.0)),
    }


def special_value_cases():
    """name -> (s, t): ties and the special float values, both classes on each."""
    f = lambda *v: np.asarray(v, F32)  # noqa: E731
    sub = F32(1e-45)  # the smallest subnormal
    big = np.finfo(F32).max
    return {
        "all_equal": (f(0.5, 0.5, 0.5, 0.5), f(1.0, 0.0, 1.0, 0.0)),
        "all_equal_257": (np.full(257, -1.25, F32), (np.arange(257) % 3 == 0).astype(F32)),
        "three_values": (f(-1.0, 0.0, 0.0, 1.0, 1.0, -1.0, -1.0, 0.0, 1.0), f(1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0)),
        "signed_zeros": (f(-0.0, 0.0, -0.0, 0.0, -1.0, 1.0, 0.0, -0.0), f(1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0)),
        "infinities": (f(-np.inf, -np.inf, np.inf, np.inf, 0.0, 1.0, -1.0, 2.0), f(1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0)),
        "subnormals": (f(sub, -sub, 0.0, -0.0, sub, -sub, 2 * sub, 0.0), f(1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
        "largest_finite": (f(big, big, -big, -big, 0.0, 1.0, big, -big), f(1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0)),
    }


def eer_cases():
    """name -> (s, t) for the branches of the EER."""
    f = lambda *v: np.asarray(v, F32)  # noqa: E731
    return {
        # P_miss - P_fa is -1 at the lowest score of any problem, so "the crossing is the first threshold" happens only
        # when no threshold crosses (the torch form's argmax of an all-false mask): several scores, the top one tied
        "no_crossing_several_scores": (f(0.0, 5.0, 5.0, 5.0, 5.0, 5.0), f(1.0, 1.0, 1.0, 1.0, 0.0, 0.0)),
        # pm - pf == 0 exactly at the crossing (2 of 4 targets below, 2 of 4 non-targets at or above)
        "zero_at_crossing": (f(0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0), f(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)),
        # no crossing: one tie run holds every trial
        "no_crossing": (f(1.0, 1.0, 1.0), f(1.0, 0.0, 1.0)),
        "separated": (f(0.0, 1.0, 2.0, 3.0, 4.0), f(0.0, 0.0, 1.0, 1.0, 1.0)),
        "reversed": (f(0.0, 1.0, 2.0, 3.0, 4.0), f(1.0, 1.0, 1.0, 0.0, 0.0)),
        # the tie run at 2.0 holds both classes and straddles the crossing
        "tie_run_straddles": (f(0.0, 1.0, 2.0, 2.0, 2.0, 2.0, 3.0, 4.0, 1.0), f(0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0)),
        # generic interpolation: 3 targets, 5 non-targets
        "interpolated": (f(0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0), f(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0)),
    }


def with_nans(n, seed, kind):
    """A mixed-label problem with NaN scores -> (s, t, mask of the NaN trials).  kind "one_target": a single NaN with the
    sign bit set on a target labelled 1; "one_excluded": the same on a trial labelled 0.5; "many": about 10 % NaN of both signs, half
    on targets labelled 1 and half on non-targets labelled 0, so that their labels sum to half their number and
    relabelling them 0.5 leaves both label sums as they are.  s[0] = 0 on a non-excluded trial, so that setting the
    NaN trials' scores to 0 adds no threshold."""
    s, t = mixed_labels(n, seed, quant=0.125)
    keep = np.flatnonzero(t == 0.25)[0]
    s[[0, keep]], t[[0, keep]] = s[[keep, 0]], t[[keep, 0]]
    s[0] = 0.0
    later = np.arange(n) > 0
    mask = np.zeros(n, bool)
    if kind == "one_target":
        mask[np.flatnonzero((t == 1.0) & later)[0]] = True
    elif kind == "one_excluded":
        mask[np.flatnonzero((t == 0.5) & later)[0]] = True
    else:
        m = max(1, n // 20)
        ones, zeros = np.flatnonzero((t == 1.0) & later), np.flatnonzero((t == 0.0) & later)
        assert ones.size > m and zeros.size > m  # some of each stay
        mask[ones[:m]] = True
        mask[zeros[:m]] = True
    idx = np.flatnonzero(mask)
    bits = s.view(np.uint32).copy()
    bits[idx[0::2]] = NAN_NEG
    bits[idx[1::2]] = NAN_POS
    return bits.view(F32), t, mask


def every_exclusion(n, seed):
    """One input for all four score-evaluation families: labels from {0, 0.25, 0.5, 0.75, 1, NaN} (42 % in each class, 8 %
    0.5, 8 % NaN), scores on a grid of 0.25 (ties) with about 2 % each of -inf and +inf and 8 % NaN of both signs, drawn
    independently of the labels — so every way a trial can leave a class meets every label."""
    rg = np.random.default_rng(seed)
    t = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0, np.nan], F32)[rg.choice(6, n, p=[0.32, 0.10, 0.08, 0.10, 0.32, 0.08])]
    s = (np.round((rg.standard_normal(n) + 1.5 * (t > 0.5)) * 4) / 4).astype(F32)
    kind = rg.choice(4, n, p=[0.88, 0.02, 0.02, 0.08])
    s[kind == 1], s[kind == 2] = -np.inf, np.inf
    bits = s.view(np.uint32).copy()
    idx = np.flatnonzero(kind == 3)
    bits[idx[0::2]] = NAN_NEG
    bits[idx[1::2]] = NAN_POS
    return bits.view(F32), t


NAN_CASES = [(n, kind) for n in (17, 4097) for kind in ("one_target", "one_excluded", "many")]


def nans_replaced(s, t, mask):
    """The same problem with the NaN trials labelled 0.5 and scored 0."""
    return np.where(mask, F32(0), s).astype(F32), np.where(mask, F32(0.5), t).astype(F32)
