"""Speaker diarization with sliding-window x-vectors: the host logic around the device steps, and the whole chain.

    speech_segments(mask, lengths)        VAD decisions -> per recording (S, 2) [begin, end) runs of speech
    read_segments(path, frame_shift)      a Kaldi `segments` file -> the same structure
    uniform_windows(segments, window, shift)   -> (W, 4) rows (recording, segment, begin, end)
    frame_labels / turns(windows, labels) window labels -> per-frame labels -> (recording, begin, end, label) turns
    write_rttm(path_or_fh, reco_ids, turns, frame_shift)
    diarize(model, extractor, frames, lengths, reco_ids, ...)   MFCC -> VAD -> CMN -> windows -> x-vectors
                                          (XVectorNet_ETDNN_12Layer.extract_windows) -> cluster.cluster ->
                                          cluster.vb_refine -> turns

Everything here counts in frames, local to a recording; seconds appear only where a file holds them (frame_shift,
0.01 s by default).  A recording's segments do not overlap.  No DER scoring, no overlap detection, no RTTM reader
(design/k23_sliding_windows.md).
"""
import numpy as np
import torch

from . import cluster, features
from .xvector import CONTEXT

__all__ = ["speech_segments", "read_segments", "uniform_windows", "frame_labels", "turns", "write_rttm", "diarize",
           "Diarization"]

FRAME_SHIFT = 0.01


def _runs(m):
    """(n, 2) [begin, end) runs of True in a bool vector."""
    d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
    return np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1)], axis=1).astype(np.int64)


def speech_segments(mask, lengths, min_speech=50, max_gap=30):
    """The uint8 decisions of features.energy_vad (one per frame of the batch; a tensor costs one host copy) and the
    recordings' lengths -> a list with one (S, 2) int64 array of [begin, end) speech runs per recording, in frames of
    that recording.  Gaps of at most max_gap frames between two runs are closed first; runs shorter than min_speech
    frames are then dropped."""
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).reshape(-1) != 0
    lengths = [int(T) for T in lengths]
    if sum(lengths) != m.size:
        raise ValueError(f"lengths sum to {sum(lengths)}, mask has {m.size} decisions")
    if int(min_speech) < 1 or int(max_gap) < 0:
        raise ValueError("min_speech must be positive and max_gap must not be negative")
    out, r0 = [], 0
    for T in lengths:
        runs = _runs(m[r0:r0 + T])
        r0 += T
        if runs.shape[0] > 1:
            keep = (runs[1:, 0] - runs[:-1, 1]) > int(max_gap)  # the gaps that stay
            runs = np.stack([runs[np.concatenate([[True], keep]), 0], runs[np.concatenate([keep, [True]]), 1]], axis=1)
        out.append(runs[(runs[:, 1] - runs[:, 0]) >= int(min_speech)])
    return out


def read_segments(path, frame_shift=FRAME_SHIFT):
    """A Kaldi `segments` file (`<segment> <recording> <start> <end>`, seconds) -> (reco_ids in order of first
    appearance, the structure of speech_segments: per recording an (S, 2) array sorted by begin, times as
    round(t / frame_shift) frames)."""
    recs, rows = [], {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) < 4:
                raise ValueError(f"{path}:{ln}: expected `<segment> <recording> <start> <end>`")
            b, e = int(round(float(p[2]) / frame_shift)), int(round(float(p[3]) / frame_shift))
            if b < 0 or e < b:
                raise ValueError(f"{path}:{ln}: segment {p[0]} runs from {p[2]} to {p[3]}")
            if p[1] not in rows:
                recs.append(p[1])
                rows[p[1]] = []
            rows[p[1]].append((b, e))
    return recs, [np.array(sorted(rows[r]), np.int64).reshape(-1, 2) for r in recs]


def uniform_windows(segments, window, shift, min_frames=CONTEXT + 2):
    """Cut segments (the structure of speech_segments) into windows for x-vector extraction -> (windows, dropped).
    The rule, per segment [begin, end):
      * shorter than min_frames (at least 24: the extractor's context plus two): no window; it is reported in `dropped`
        as (recording, segment, frames);
      * at most `window` frames: the segment is one window;
      * otherwise windows of exactly `window` frames at begin + k shift, k = 0, 1, ..., while they fit in the segment;
        if the last of them ends before the segment does, one more window [end - window, end).
    With shift > window the rule leaves frames between windows that no window covers.  windows: (W, 4) int64 rows
    (recording index, segment index, begin, end), a recording's windows together and in time order (its segments are
    taken in order of begin and must not overlap)."""
    window, shift, min_frames = int(window), int(shift), int(min_frames)
    if min_frames < CONTEXT + 2:
        raise ValueError(f"min_frames = {min_frames}: the extractor needs {CONTEXT + 2} frames at least")
    if window < min_frames or shift < 1:
        raise ValueError("window must be at least min_frames and shift must be positive")
    out, dropped = [], []
    for r, segs in enumerate(segments):
        segs = np.asarray(segs, np.int64).reshape(-1, 2)
        prev = None
        for s in np.argsort(segs[:, 0], kind="stable").tolist():
            b, e = int(segs[s, 0]), int(segs[s, 1])
            if e < b or b < 0:
                raise ValueError(f"recording {r}, segment {s}: [{b}, {e})")
            if prev is not None and b < prev:
                raise ValueError(f"recording {r}: segment {s} begins at {b}, inside the segment before it")
            prev = e
            if e - b < min_frames:
                dropped.append((r, s, e - b))
                continue
            if e - b <= window:
                out.append(np.array([[r, s, b, e]], np.int64))
                continue
            wb = np.arange(b, e - window + 1, shift, dtype=np.int64)
            if wb[-1] + window < e:
                wb = np.concatenate([wb, [e - window]])
            out.append(np.stack([np.full_like(wb, r), np.full_like(wb, s), wb, wb + window], axis=1))
    return (np.concatenate(out) if out else np.zeros((0, 4), np.int64)), dropped


def frame_labels(windows, labels):
    """Per-frame labels of every segment that has windows: [(recording, segment, begin, labels)] in the order of the
    windows table, `labels` an int64 vector over the frames [begin, begin + len) from the segment's first window's begin
    to its windows' last end.  A frame takes the label of the window covering it whose centre is nearest to the frame's
    (ties: the earlier window in the table); a frame that no window covers gets -1."""
    win = np.asarray(windows, np.int64).reshape(-1, 4)
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64).reshape(-1)
    if lab.size != win.shape[0]:
        raise ValueError(f"{win.shape[0]} windows, {lab.size} labels")
    if lab.size and lab.min() < 0:
        raise ValueError("labels must not be negative")
    out = []
    cut = np.flatnonzero(np.any(win[1:, :2] != win[:-1, :2], axis=1)) + 1 if win.shape[0] else np.zeros(0, np.int64)
    for w0, w1 in zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [win.shape[0]]]).tolist()):
        if w1 == w0:
            continue
        b0, e1 = int(win[w0:w1, 2].min()), int(win[w0:w1, 3].max())
        fl = np.full(e1 - b0, -1, np.int64)
        best = np.full(e1 - b0, np.iinfo(np.int64).max)
        for w in range(w0, w1):
            b, e = int(win[w, 2]), int(win[w, 3])
            # twice the distance between the frame's centre f + 1/2 and the window's centre (b + e) / 2
            d = np.abs(2 * np.arange(b, e, dtype=np.int64) + 1 - (b + e))
            sl = slice(b - b0, e - b0)
            take = d < best[sl]
            best[sl] = np.where(take, d, best[sl])
            fl[sl] = np.where(take, lab[w], fl[sl])
        out.append((int(win[w0, 0]), int(win[w0, 1]), b0, fl))
    return out


def turns(windows, labels):
    """Window labels -> speaker turns: (N, 4) int64 rows (recording, begin, end, label), sorted by recording, then begin.
    A turn is a run of frames with one label (frame_labels) inside one segment: turns do not join across segments, and
    frames that no window covers belong to no turn."""
    out = []
    for r, _, b0, fl in frame_labels(windows, labels):
        edges = np.flatnonzero(np.diff(fl) != 0) + 1
        for a, z in zip(np.concatenate([[0], edges]).tolist(), np.concatenate([edges, [fl.size]]).tolist()):
            if z > a and fl[a] >= 0:
                out.append((r, b0 + a, b0 + z, int(fl[a])))
    out.sort(key=lambda t: (t[0], t[1], t[2]))
    return np.array(out, np.int64).reshape(-1, 4)


def write_rttm(path_or_fh, reco_ids, turns, frame_shift=FRAME_SHIFT):
    """One `SPEAKER <recording> 1 <start> <duration> <NA> <NA> <label> <NA> <NA>` line per turn (rows of turns():
    recording index into reco_ids, begin, end, label), start and duration in seconds with three decimals, sorted by
    recording (the order of reco_ids), then by start."""
    rows = sorted((tuple(int(v) for v in t) for t in np.asarray(turns, np.int64).reshape(-1, 4)),
                  key=lambda t: (t[0], t[1], t[2]))
    text = "".join(f"SPEAKER {reco_ids[r]} 1 {b * frame_shift:.3f} {(e - b) * frame_shift:.3f} <NA> <NA> {lab} <NA> <NA>\n"
                   for r, b, e, lab in rows)
    if hasattr(path_or_fh, "write"):
        path_or_fh.write(text)
    else:
        with open(path_or_fh, "w") as f:
            f.write(text)


class Diarization:
    """The result of diarize(): `reco_ids`, `segments` (as speech_segments), `windows` ((W, 4): recording, segment,
    begin, end), `dropped` (segments too short for a window), `xvectors` ((W, 512) on the device), `labels` ((W,) int64,
    unique over the whole call), `turns` ((N, 4): recording, begin, end, label), and the `clustering` (cluster.Clustering)
    and `refined` (cluster.Refined or None) they came from."""

    def __init__(self, reco_ids, segments, windows, dropped, xvectors, labels, turns, clustering, refined):
        self.reco_ids, self.segments, self.windows, self.dropped = reco_ids, segments, windows, dropped
        self.xvectors, self.labels, self.turns, self.clustering, self.refined = xvectors, labels, turns, clustering, refined

    def write_rttm(self, path_or_fh, frame_shift=FRAME_SHIFT):
        write_rttm(path_or_fh, self.reco_ids, self.turns, frame_shift)


def diarize(model, extractor, frames, lengths, reco_ids, segments=None, vad=features.VadOptions(), min_speech=50,
            max_gap=30, cmn_window=300, window=144, shift=24, min_frames=CONTEXT + 2, threshold=0.0, min_clusters=1,
            linkage="average", vb_psi=None, vb=None, workspace_bytes=None):
    """Diarize whole recordings -> Diarization.  frames: (sum T_r, 30) raw MFCC rows on the device, recording r being the
    next lengths[r] rows; reco_ids: their names.  The steps, all on the device but the window bookkeeping:
      1. segments: the given ones (the structure of speech_segments), or features.energy_vad(vad) through
         speech_segments(min_speech, max_gap);
      2. features.cmn_select(mask=None, cmn_window): sliding-window mean subtraction with every frame kept, so that rows
         stay aligned with time;
      3. uniform_windows(window, shift, min_frames);
      4. extractor.extract_windows over the windows' rows (an XVectorNet_ETDNN_12Layer);
      5. cluster.cluster(model, x-vectors, groups=recording, threshold, min_clusters, linkage);
      6. with vb_psi (the PLDA between-class variances): cluster.vb_refine(model, x-vectors, that clustering, vb_psi,
         groups=recording, **vb); a recording's windows are in time order already;
      7. turns()."""
    lengths = [int(T) for T in lengths]
    reco_ids = list(reco_ids)
    if len(reco_ids) != len(lengths):
        raise ValueError(f"{len(reco_ids)} recording names, {len(lengths)} lengths")
    if segments is None:
        segments = speech_segments(features.energy_vad(frames, lengths, vad), lengths, min_speech, max_gap)
    elif len(segments) != len(lengths):
        raise ValueError(f"{len(segments)} segment lists, {len(lengths)} recordings")
    for r, (segs, T) in enumerate(zip(segments, lengths)):
        segs = np.asarray(segs, np.int64).reshape(-1, 2)
        if segs.size and (segs.min() < 0 or segs.max() > T):
            raise ValueError(f"recording {reco_ids[r]}: a segment lies outside its {T} frames")
    rows, _ = features.cmn_select(frames, lengths, None, cmn_window, 0)
    windows, dropped = uniform_windows(segments, window, shift, min_frames)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    table = windows[:, 2:4] + starts[windows[:, 0]][:, None]
    with torch.no_grad():
        x = extractor.extract_windows(rows, table, workspace_bytes=workspace_bytes)
    clus = refined = None
    labels = np.zeros(0, np.int64)
    if windows.shape[0]:
        groups = windows[:, 0]
        clus = cluster.cluster(model, x, groups=groups, threshold=threshold, min_clusters=min_clusters, linkage=linkage)
        labels = clus.labels
        if vb_psi is not None:
            refined = cluster.vb_refine(model, x, clus, vb_psi, groups=groups, **(vb or {}))
            labels = refined.labels
    return Diarization(reco_ids, segments, windows, dropped, x, labels, turns(windows, labels), clus, refined)
