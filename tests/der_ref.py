"""The numpy twin of the diarization error rate (csrc/nplda_der.hip, design/k24_der.md), written from the definitions and not
from the kernel's method: boolean (S, T) activity matrices, the scored mask, the overlap matrix as a matrix product, and the
optimal mapping by scipy's linear_sum_assignment or, for at most 7 speakers a side, by brute force over permutations.

A turn is (begin, end, speaker) in frames of one recording; all counts are exact integers."""
import itertools

import numpy as np

MAX_BRUTE = 7


def activity(turns, S, T):
    """(S, T) bool: speaker s is active at frame t under some turn (bounds clipped to [0, T], speakers outside [0, S) dropped)."""
    A = np.zeros((S, T), bool)
    for b, e, s in np.asarray(turns, np.int64).reshape(-1, 3).tolist():
        if 0 <= s < S:
            A[s, min(max(b, 0), T):min(max(e, 0), T)] = True
    return A


def scored_mask(ref_turns, T, S=64, uem=None, collar=0, skip_overlap=False):
    """(T,) bool by the definition: inside the UEM regions (None: every frame), not within `collar` frames of a boundary of
    a reference turn (f in [b - c, b + c) or [e - c, e + c)), and with skip_overlap at most one reference speaker."""
    if uem is None:
        m = np.ones(T, bool)
    else:
        m = np.zeros(T, bool)
        for b, e in np.asarray(uem, np.int64).reshape(-1, 2).tolist():
            m[min(max(b, 0), T):min(max(e, 0), T)] = True
    f = np.arange(T)
    for b, e, s in np.asarray(ref_turns, np.int64).reshape(-1, 3).tolist():
        if not 0 <= s < S:
            continue
        b, e = min(max(b, 0), T), min(max(e, 0), T)
        if e < b:
            continue
        m &= ~(((f >= b - collar) & (f < b + collar)) | ((f >= e - collar) & (f < e + collar)))
    if skip_overlap:
        m &= activity(ref_turns, S, T).sum(axis=0) <= 1
    return m


def items_activity(frame_item, labels, S, T):
    """The labelled-items form of a hypothesis -> (S, T) bool: frame t belongs to item frame_item[t] (or to none: -1, or an
    index past the labels), whose label names the one active speaker (or none: outside [0, S))."""
    fi = np.asarray(frame_item, np.int64).reshape(-1)[:T]
    lab = np.asarray(labels, np.int64).reshape(-1)
    A = np.zeros((S, T), bool)
    ok = (fi >= 0) & (fi < lab.size)
    fl = np.where(ok, lab[np.where(ok, fi, 0)] if lab.size else -1, -1)
    ok = (fl >= 0) & (fl < S)
    A[fl[ok], np.flatnonzero(ok)] = True
    return A


def best_mapping_scipy(C):
    from scipy.optimize import linear_sum_assignment
    if C.shape[0] == 0 or C.shape[1] == 0:
        return 0, {}
    rows, cols = linear_sum_assignment(C, maximize=True)
    return int(C[rows, cols].sum()), {int(i): int(j) for i, j in zip(rows, cols) if C[i, j] > 0}


def best_mapping_brute(C):
    """Every injection of the shorter side into the longer one."""
    nr, nh = C.shape
    if nr > MAX_BRUTE or nh > MAX_BRUTE:
        raise ValueError(f"brute force takes at most {MAX_BRUTE} speakers a side")
    if nr == 0 or nh == 0:
        return 0, {}
    best, arg = -1, None
    if nr <= nh:
        for perm in itertools.permutations(range(nh), nr):
            v = int(sum(C[i, j] for i, j in enumerate(perm)))
            if v > best:
                best, arg = v, {i: j for i, j in enumerate(perm)}
    else:
        for perm in itertools.permutations(range(nr), nh):
            v = int(sum(C[i, j] for j, i in enumerate(perm)))
            if v > best:
                best, arg = v, {i: j for j, i in enumerate(perm)}
    return best, {i: j for i, j in arg.items() if C[i, j] > 0}


def conf_by_frames(A_ref, A_hyp, scored, mapping):
    """Speaker confusion counted frame by frame under a mapping: min(|R|, |H|) less the reference speakers whose mapped
    hypothesis speaker is active too."""
    nr, nh = A_ref[:, scored].sum(axis=0), A_hyp[:, scored].sum(axis=0)
    correct = np.zeros(int(scored.sum()), np.int64)
    for i, j in mapping.items():
        correct += A_ref[i, scored] & A_hyp[j, scored]
    return int((np.minimum(nr, nh) - correct).sum())


class Counts(dict):
    __getattr__ = dict.__getitem__


def counts_from_activity(A_ref, A_hyp, scored, method="scipy"):
    R, H = A_ref[:, scored], A_hyp[:, scored]
    nr, nh = R.sum(axis=0).astype(np.int64), H.sum(axis=0).astype(np.int64)
    C = np.rint(R.astype(np.float64) @ H.astype(np.float64).T).astype(np.int64)  # (exact: counts far below 2^53; BLAS speed)
    matched, mapping = (best_mapping_scipy if method == "scipy" else best_mapping_brute)(C)
    summin = int(np.minimum(nr, nh).sum())
    return Counts(scored=int(scored.sum()), total=int(nr.sum()), miss=int(np.maximum(nr - nh, 0).sum()),
                  fa=int(np.maximum(nh - nr, 0).sum()), summin=summin, matched=matched, conf=summin - matched, C=C,
                  mapping=mapping)


def der_counts(ref_turns, hyp_turns, T, S_ref=64, S_hyp=64, uem=None, collar=0, skip_overlap=False, method="scipy"):
    scored = scored_mask(ref_turns, T, S_ref, uem, collar, skip_overlap)
    return counts_from_activity(activity(ref_turns, S_ref, T), activity(hyp_turns, S_hyp, T), scored, method)


def der_counts_items(ref_turns, frame_item, labels, T, S_ref=64, S_hyp=64, uem=None, collar=0, skip_overlap=False,
                     method="scipy"):
    scored = scored_mask(ref_turns, T, S_ref, uem, collar, skip_overlap)
    return counts_from_activity(activity(ref_turns, S_ref, T), items_activity(frame_item, labels, S_hyp, T), scored, method)


def der_value(c):
    return (c["miss"] + c["fa"] + c["conf"]) / c["total"] if c["total"] else float("nan")


def random_turns(rng, T, S, n, max_len=None, simultaneous=4):
    """n random turns over S speakers in [0, T]; at most `simultaneous` speakers are active at a frame (a turn that would
    exceed it is dropped).  Lengths up to max_len (default T); empty turns occur."""
    out = np.zeros((0, 3), np.int64)
    if S == 0 or T == 0:
        return out
    depth = np.zeros(T, np.int64)
    rows = []
    for _ in range(n):
        b = int(rng.integers(0, T + 1))
        e = min(T, b + int(rng.integers(0, (max_len or T) + 1)))
        if e > b and depth[b:e].max() >= simultaneous:
            continue
        depth[b:e] += 1
        rows.append((b, e, int(rng.integers(0, S))))
    return np.array(rows, np.int64).reshape(-1, 3)
