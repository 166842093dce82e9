"""The host logic of sliding-window diarization (neuralplda_amd/diarize.py), the chunk planner of
XVectorNet_ETDNN_12Layer.extract_windows and the argument checks of its C entry points, without a GPU.  Every function is
held against a brute-force per-frame twin written here."""
import ctypes
import io

import numpy as np
import pytest

from neuralplda_amd import diarize as dz
from neuralplda_amd import xvector


# ---- twins: one frame at a time -------------------------------------------------------------------------------------

def twin_speech_segments(mask, lengths, min_speech, max_gap):
    out, r0 = [], 0
    for T in lengths:
        m = [bool(v) for v in mask[r0:r0 + T]]
        r0 += T
        speech = [t for t in range(T) if m[t]]
        for t in range(T):  # a non-speech frame between two speech frames at most max_gap + 1 apart is filled
            if not m[t]:
                left = max([s for s in speech if s < t], default=None)
                right = min([s for s in speech if s > t], default=None)
                if left is not None and right is not None and right - left - 1 <= max_gap:
                    m[t] = True
        runs, t = [], 0
        while t < T:
            if m[t]:
                a = t
                while t < T and m[t]:
                    t += 1
                if t - a >= min_speech:
                    runs.append((a, t))
            else:
                t += 1
        out.append(np.array(runs, np.int64).reshape(-1, 2))
    return out


def twin_windows(segments, window, shift, min_frames=24):
    out, dropped = [], []
    for r, segs in enumerate(segments):
        for s in sorted(range(len(segs)), key=lambda i: segs[i][0]):
            b, e = int(segs[s][0]), int(segs[s][1])
            if e - b < min_frames:
                dropped.append((r, s, e - b))
            elif e - b <= window:
                out.append((r, s, b, e))
            else:
                k = 0
                while b + k * shift + window <= e:
                    out.append((r, s, b + k * shift, b + k * shift + window))
                    k += 1
                if out[-1][3] < e:
                    out.append((r, s, e - window, e))
    return np.array(out, np.int64).reshape(-1, 4), dropped


def twin_frame_label(windows, labels, r, s, f):
    """The label of frame f of segment (r, s), or -1: the covering window with the nearest centre, the earlier on a tie."""
    best, lab = None, -1
    for (wr, ws, b, e), l in zip(windows.tolist(), labels):
        if (wr, ws) == (r, s) and b <= f < e:
            d = abs((f + 0.5) - (b + e) / 2.0)
            if best is None or d < best:
                best, lab = d, int(l)
    return lab


def twin_turns(windows, labels):
    out = []
    for r, s in sorted({(int(w[0]), int(w[1])) for w in windows}):
        rows = windows[(windows[:, 0] == r) & (windows[:, 1] == s)]
        b0, e1 = int(rows[:, 2].min()), int(rows[:, 3].max())
        cur = None
        for f in range(b0, e1 + 1):
            l = twin_frame_label(windows, labels, r, s, f) if f < e1 else -1
            if cur is not None and l != cur[3]:
                out.append((cur[0], cur[1], f, cur[3]))
                cur = None
            if cur is None and l >= 0:
                cur = (r, f, None, l)
    out.sort(key=lambda t: (t[0], t[1]))
    return np.array(out, np.int64).reshape(-1, 4)


def random_segments(rng, n_reco, T, lo=5, hi=160):
    segs = []
    for _ in range(n_reco):
        t, rows = int(rng.integers(0, 20)), []
        while True:
            n = int(rng.integers(lo, hi)) if rows else 23  # the first one is a frame too short for a window
            if t + n > T:
                break
            rows.append((t, t + n))
            t += n + int(rng.integers(0, 40))  # a gap of 0 makes two segments abut
        rng.shuffle(rows)
        segs.append(np.array(rows, np.int64).reshape(-1, 2))
    return segs


# ---- speech_segments ------------------------------------------------------------------------------------------------

def test_speech_segments_against_the_twin():
    rng = np.random.default_rng(1)
    for min_speech, max_gap in [(1, 0), (5, 3), (10, 0), (3, 8)]:
        lengths = [int(v) for v in rng.integers(0, 200, 5)]
        raw = rng.random(sum(lengths)) < 0.5
        # runs of a few frames, not single frames: smooth the coin flips
        mask = np.repeat(raw[::4], 4)[:sum(lengths)].astype(np.uint8) if sum(lengths) else np.zeros(0, np.uint8)
        got = dz.speech_segments(mask, lengths, min_speech, max_gap)
        ref = twin_speech_segments(mask, lengths, min_speech, max_gap)
        assert len(got) == len(lengths)
        for g, r in zip(got, ref):
            assert g.dtype == np.int64 and np.array_equal(g, r)


def test_speech_segments_by_hand():
    #        0         1         2         3
    #        0123456789012345678901234567890123456789
    text = "..#####..###......##########...#........"
    mask = np.array([c == "#" for c in text], np.uint8)
    assert dz.speech_segments(mask, [40], min_speech=1, max_gap=0)[0].tolist() == [[2, 7], [9, 12], [18, 28], [31, 32]]
    assert dz.speech_segments(mask, [40], min_speech=4, max_gap=0)[0].tolist() == [[2, 7], [18, 28]]
    # gaps close first: [2, 7) + [9, 12) is one run of 10, then [31, 32) joins [18, 28) over the 3-frame gap
    assert dz.speech_segments(mask, [40], min_speech=4, max_gap=3)[0].tolist() == [[2, 12], [18, 32]]
    # recordings are apart: a run at the end of one does not join a run at the start of the next
    assert [s.tolist() for s in dz.speech_segments(np.ones(10, np.uint8), [4, 6], 1, 5)] == [[[0, 4]], [[0, 6]]]
    with pytest.raises(ValueError):
        dz.speech_segments(mask, [39])


# ---- uniform_windows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window,shift", [(48, 12), (30, 30), (24, 1), (40, 55), (150, 75)])
def test_uniform_windows_against_the_twin(window, shift):
    rng = np.random.default_rng(window * 100 + shift)
    segs = random_segments(rng, 4, 900)
    got, dropped = dz.uniform_windows(segs, window, shift)
    ref, ref_dropped = twin_windows(segs, window, shift)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert dropped == ref_dropped and len(dropped) > 0
    for r in range(4):
        w = got[got[:, 0] == r]
        assert (np.diff(np.flatnonzero(got[:, 0] == r)) == 1).all()              # a recording's windows are together
        assert (np.diff(w[:, 2]) >= 0).all() and (np.diff(w[:, 3]) >= 0).all()  # time order per recording
        assert (w[:, 3] - w[:, 2] >= 24).all() and (w[:, 3] - w[:, 2] <= window).all()
        covered = np.zeros(900, bool)
        for _, _, b, e in w.tolist():
            covered[b:e] = True
        kept = np.zeros(900, bool)
        for b, e in segs[r].tolist():
            if e - b >= 24:
                kept[b:e] = True
        assert not (covered & ~kept).any()
        if shift <= window:
            assert np.array_equal(covered, kept)  # every speech frame of a kept segment is covered
        else:
            assert (kept & ~covered).any()        # the stated rule leaves gaps


def test_uniform_windows_by_hand():
    W = lambda segs, window, shift: [w[2:] for w in dz.uniform_windows([np.array(segs)], window, shift)[0].tolist()]  # noqa: E731
    got, dropped = dz.uniform_windows([np.array([[10, 33]])], 48, 12)   # 23 frames: dropped and reported
    assert got.shape == (0, 4) and dropped == [(0, 0, 23)]
    assert W([[10, 34]], 48, 12) == [[10, 34]]                       # 24 frames: one window
    assert W([[10, 58]], 48, 12) == [[10, 58]]                       # exactly the window
    assert W([[10, 59]], 48, 12) == [[10, 58], [11, 59]]             # window + 1: the end-aligned tail
    assert W([[0, 100]], 48, 12) == [[0, 48], [12, 60], [24, 72], [36, 84], [48, 96], [52, 100]]
    assert W([[0, 96]], 48, 12) == [[0, 48], [12, 60], [24, 72], [36, 84], [48, 96]]
    assert W([[0, 96]], 48, 48) == [[0, 48], [48, 96]]               # shift == window
    assert W([[0, 97]], 48, 48) == [[0, 48], [48, 96], [49, 97]]
    assert W([[0, 130]], 30, 50) == [[0, 30], [50, 80], [100, 130]]  # shift > window: [30, 50) and [80, 100) uncovered
    assert W([[0, 120]], 30, 50) == [[0, 30], [50, 80], [90, 120]]
    # segments out of order come back in time order with their own indices
    got, dropped = dz.uniform_windows([np.array([[200, 230], [0, 10], [50, 80]])], 40, 20)
    assert got.tolist() == [[0, 2, 50, 80], [0, 0, 200, 230]] and dropped == [(0, 1, 10)]
    with pytest.raises(ValueError):
        dz.uniform_windows([np.array([[0, 50], [40, 90]])], 40, 20)   # overlapping segments
    with pytest.raises(ValueError):
        dz.uniform_windows([np.array([[0, 50]])], 40, 20, min_frames=23)
    with pytest.raises(ValueError):
        dz.uniform_windows([np.array([[0, 50]])], 40, 0)


# ---- frame_labels / turns -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window,shift", [(48, 12), (30, 30), (31, 10), (40, 55), (25, 3)])
def test_turns_against_the_twin(window, shift):
    rng = np.random.default_rng(window * 7 + shift)
    segs = random_segments(rng, 3, 500)
    win, _ = dz.uniform_windows(segs, window, shift)
    labels = rng.integers(0, 3, win.shape[0])
    got = dz.turns(win, labels)
    assert got.dtype == np.int64 and np.array_equal(got, twin_turns(win, labels))
    # turns tile the covered frames exactly once, inside one segment, and neighbours in a segment differ in label
    for r in range(3):
        count = np.zeros(500, np.int64)
        for _, b, e, _ in got[got[:, 0] == r].tolist():
            count[b:e] += 1
            assert any(sb <= b and e <= se for sb, se in segs[r].tolist())
        covered = np.zeros(500, np.int64)
        for _, _, b, e in win[win[:, 0] == r].tolist():
            covered[b:e] = 1
        assert np.array_equal(count, covered)
    for (r, s, b0, fl) in dz.frame_labels(win, labels):
        for f in range(b0, b0 + fl.size, 7):
            assert fl[f - b0] == twin_frame_label(win, labels, r, s, f)


def test_turns_by_hand():
    # one segment [0, 100), windows 48 / 12: centres 24, 36, 48, 60, 72, 76
    win, _ = dz.uniform_windows([np.array([[0, 100]])], 48, 12)
    lab = np.array([5, 5, 7, 7, 5, 7])
    # frame f (centre f + 1/2) goes to the nearest centre: [0, 30) -> 24, [30, 42) -> 36, [42, 54) -> 48, [54, 66) -> 60,
    # [66, 74) -> 72, [74, 100) -> 76
    assert dz.turns(win, lab).tolist() == [[0, 0, 42, 5], [0, 42, 66, 7], [0, 66, 74, 5], [0, 74, 100, 7]]
    # a tie: [0, 24) and [2, 26) have centres 12 and 13, frame 12 (centre 12.5) is as near to both -> the earlier window
    win = np.array([[0, 0, 0, 24], [0, 0, 2, 26]])
    assert dz.turns(win, [1, 2]).tolist() == [[0, 0, 13, 1], [0, 13, 26, 2]]
    assert dz.turns(win, [3, 3]).tolist() == [[0, 0, 26, 3]]
    # two abutting segments with one label: two turns; and shift > window: the uncovered frames belong to no turn
    win, _ = dz.uniform_windows([np.array([[0, 30], [30, 60]]), np.array([[0, 130]])], 30, 50)
    assert dz.turns(win, [4, 4, 0, 0, 1]).tolist() == [[0, 0, 30, 4], [0, 30, 60, 4], [1, 0, 30, 0], [1, 50, 80, 0],
                                                        [1, 100, 130, 1]]
    assert dz.turns(np.zeros((0, 4), np.int64), []).shape == (0, 4)


# ---- files ----------------------------------------------------------------------------------------------------------

def test_write_rttm_text(tmp_path):
    t = np.array([[1, 0, 250, 3], [0, 1234, 1300, 0], [0, 5, 105, 2], [1, 250, 251, 4]])
    want = ("SPEAKER recA 1 0.050 1.000 <NA> <NA> 2 <NA> <NA>\n"
            "SPEAKER recA 1 12.340 0.660 <NA> <NA> 0 <NA> <NA>\n"
            "SPEAKER recB 1 0.000 2.500 <NA> <NA> 3 <NA> <NA>\n"
            "SPEAKER recB 1 2.500 0.010 <NA> <NA> 4 <NA> <NA>\n")
    fh = io.StringIO()
    dz.write_rttm(fh, ["recA", "recB"], t, 0.01)
    assert fh.getvalue() == want
    p = tmp_path / "out.rttm"
    dz.write_rttm(str(p), ["recA", "recB"], t)
    assert p.read_text() == want
    dz.write_rttm(str(p), ["recA"], np.zeros((0, 4), np.int64))
    assert p.read_text() == ""


def test_read_segments(tmp_path):
    p = tmp_path / "segments"
    p.write_text("recB-0001 recB 0.00 1.50\nrecA-0002 recA 12.345 13.004\n\nrecA-0001 recA 0.5 2.25\nrecB-0002 recB 2 3.1\n")
    recs, segs = dz.read_segments(str(p), 0.01)
    assert recs == ["recB", "recA"]
    assert [s.tolist() for s in segs] == [[[0, 150], [200, 310]], [[50, 225], [1234, 1300]]]
    assert all(s.dtype == np.int64 for s in segs)
    p.write_text("seg rec 1.0\n")
    with pytest.raises(ValueError):
        dz.read_segments(str(p))


# ---- the chunk planner of extract_windows ---------------------------------------------------------------------------

def planner_tables():
    rng = np.random.default_rng(3)
    dense = np.stack([np.arange(0, 3000, 7), np.arange(0, 3000, 7) + 60], axis=1)
    gap = np.concatenate([dense[:40], dense[:40] + 100_000])                        # a large uncovered gap
    mixed = np.stack([rng.integers(0, 5000, 300), np.zeros(300, np.int64)], axis=1)
    mixed[:, 1] = mixed[:, 0] + rng.integers(23, 400, 300)
    nested = np.array([[0, 2000], [10, 40], [500, 530], [1990, 2100], [5000, 5030], [5030, 5060], [5061, 5090]])
    return {"dense": dense, "gap": gap, "mixed": rng.permutation(mixed), "nested": nested,
            "repeat": np.array([[5, 50]] * 4)}


@pytest.mark.parametrize("name", ["dense", "gap", "mixed", "nested", "repeat"])
@pytest.mark.parametrize("limit", [1, 3 << 20, 6 << 20, 1 << 30])
def test_plan_windows(name, limit):
    win = planner_tables()[name]
    chunks = xvector.plan_windows(win, limit)
    seen = np.concatenate([c.windows for c in chunks])
    assert np.array_equal(np.sort(seen), np.arange(win.shape[0]))                   # every window in exactly one chunk
    assert (np.diff(win[seen, 0]) >= 0).all()                                       # in order of begin
    for c in chunks:
        assert len(c.windows) == 1 or xvector._ws_bytes(c.rows, len(c.windows)) <= limit
        src = np.concatenate([np.arange(b, e) for b, e in c.intervals])             # the caller's row of each input row
        assert src.size == c.rows and (np.diff(src) > 0).all()                      # disjoint, ascending
        want = np.unique(np.concatenate([np.arange(b, e) for b, e in win[c.windows].tolist()]))
        assert np.array_equal(src, want)                                            # exactly the union of the windows' rows
        assert all(b1 > e0 for (_, e0), (b1, _) in zip(c.intervals, c.intervals[1:]))  # a real gap between intervals
        for w, lb, le in zip(c.windows.tolist(), c.begin.tolist(), c.end.tolist()):
            assert np.array_equal(src[lb:le], np.arange(win[w, 0], win[w, 1]))      # the window's own rows, consecutive
    if limit == 1:
        assert len(chunks) == win.shape[0] and all(c.rows == e - b for c, (b, e) in zip(chunks, win[seen].tolist()))
    if limit == 1 << 30:
        assert len(chunks) == 1
    if limit == 3 << 20 and name in ("dense", "mixed"):
        # (a cut recomputes only rows that windows on both sides of it cover: each input is exactly its windows' union)
        assert len(chunks) >= 3


def test_plan_windows_skips_the_gap():
    chunks = xvector.plan_windows(planner_tables()["gap"], 1 << 30)
    assert len(chunks) == 1 and chunks[0].rows == 2 * (39 * 7 + 60) and len(chunks[0].intervals) == 2
    assert xvector.plan_windows(np.zeros((0, 2), np.int64), 1 << 30) == []


# ---- C ABI ----------------------------------------------------------------------------------------------------------

def test_windows_workspace_bytes(hip_lib):
    f = hip_lib.nplda_xvec_windows_workspace_bytes
    for R, W in [(0, 0), (0, 1), (1, 1), (128, 128), (129, 129), (407, 35), (60000, 2495), (3_840_000, 160_000)]:
        assert f(R, W) == xvector._ws_bytes(R, W) == hip_lib.nplda_xvec_workspace_bytes(R, W)
    assert f(-1, 4) == 0 and f(4, -1) == 0
    vals = [[f(R, W) for W in (0, 1, 128, 129, 5000)] for R in (0, 1, 127, 128, 129, 10_000)]
    assert all(a <= b for row in vals for a, b in zip(row, row[1:]))                # monotone in the windows
    assert all(a <= b for c0, c1 in zip(vals, vals[1:]) for a, b in zip(c0, c1))    # and in the frames
    assert f(10_000, 5000) > f(0, 5000) > f(0, 0)


def test_extract_windows_argument_checks(hip_lib):
    """Every check returns before anything is launched, so host memory stands in for the device pointers."""
    f = hip_lib.nplda_xvec_extract_windows_f32
    EINVAL, ENOSPC = -22, -28
    buf = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(buf) + 15) & ~15                                          # 16-byte aligned, not null
    R, W = 400, 10
    need = hip_lib.nplda_xvec_windows_workspace_bytes(R, W)

    def call(x=p, ld_in=30, R=R, b=p, e=p, W=W, pooling=0, packed=p, out=p, ldx=512, ws=p, ws_bytes=need - 1):
        return f(x, ld_in, R, b, e, W, pooling, packed, out, ldx, ws, ws_bytes, None)

    assert f(None, 30, 0, None, None, 0, 0, None, None, 512, None, 0, None) == 0    # no windows: OK, nothing touched
    assert f(None, 30, R, None, None, 0, 1, None, None, 512, None, 0, None) == 0
    assert call() == ENOSPC                                                         # everything valid but the workspace
    assert call(ws_bytes=0) == ENOSPC
    assert call(W=-1) == EINVAL and call(R=-1) == EINVAL
    assert call(pooling=2) == EINVAL and call(pooling=-1) == EINVAL
    assert f(None, 30, R, None, None, 0, 2, None, None, 512, None, 0, None) == EINVAL  # bad pooling even with no windows
    for null in ("x", "b", "e", "packed", "out", "ws"):
        assert call(**{null: None}) == EINVAL, null
    assert call(packed=p + 4) == EINVAL and call(ws=p + 8) == EINVAL and call(out=p + 4) == EINVAL
    assert call(ldx=508) == EINVAL and call(ldx=511) == EINVAL and call(ldx=514) == EINVAL
    assert call(ldx=516) == ENOSPC
    assert call(ld_in=29) == EINVAL and call(ld_in=32) == ENOSPC
