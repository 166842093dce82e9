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
0.01 s by default).  A recording's segments do not overlap.  No overlap detection (design/k23_sliding_windows.md).

Scoring (design/k24_der.md; the rate itself is metrics.der):

    read_rttm(path, frame_shift)          the SPEAKER lines of an RTTM file -> (reco_ids, (N, 4) turns, speaker names)
    read_uem(path, frame_shift)           a UEM file -> (reco_ids, per recording (n, 2) regions)
    Diarization.der(ref_turns, ...)       the DER of the result's own turns
    sweep_thresholds(diarization, ref_turns, thresholds, ...)   the DER of every cut of the recorded dendrogram, all
                                          (threshold, recording) cells in ONE device call
"""
import numpy as np
import torch

from . import cluster, features
from .xvector import CONTEXT

__all__ = ["speech_segments", "read_segments", "uniform_windows", "frame_labels", "turns", "write_rttm", "diarize",
           "Diarization", "read_rttm", "read_uem", "sweep_thresholds", "SweepResult"]

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


def read_rttm(path, frame_shift=FRAME_SHIFT):
    """The `SPEAKER <recording> <channel> <start> <duration> <NA> <NA> <speaker> ...` lines of an RTTM file (other line
    types and `;` comments are passed over) -> (reco_ids in order of first appearance, turns: (N, 4) int64 rows (recording
    index, begin, end, label) in the order of turns(): by recording, begin, end, speaker_names: per recording the names in
    order of first appearance in the file; a label indexes its recording's names).  Times are round(t / frame_shift)
    frames, begin from <start> and end from <start> + <duration>."""
    recs, index, names, rows = [], {}, [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p or p[0].startswith(";") or p[0] != "SPEAKER":
                continue
            if len(p) < 8:
                raise ValueError(f"{path}:{ln}: expected `SPEAKER <recording> <channel> <start> <duration> <NA> <NA> <speaker>`")
            try:
                start, dur = float(p[3]), float(p[4])
            except ValueError:
                raise ValueError(f"{path}:{ln}: start {p[3]!r} and duration {p[4]!r} must be numbers") from None
            b, e = int(round(start / frame_shift)), int(round((start + dur) / frame_shift))
            if not (start >= 0.0 and dur >= 0.0) or e < b:
                raise ValueError(f"{path}:{ln}: a turn of {p[7]} starts at {p[3]} and lasts {p[4]}")
            if p[1] not in index:
                index[p[1]] = len(recs)
                recs.append(p[1])
                names.append([])
            r = index[p[1]]
            if p[7] not in names[r]:
                names[r].append(p[7])
            rows.append((r, b, e, names[r].index(p[7])))
    rows.sort(key=lambda t: (t[0], t[1], t[2]))
    return recs, np.array(rows, np.int64).reshape(-1, 4), names


def read_uem(path, frame_shift=FRAME_SHIFT):
    """A UEM file (`<recording> <channel> <start> <end>`, seconds; `;` comments) -> (reco_ids in order of first
    appearance, per recording an (n, 2) int64 array of [begin, end) regions sorted by begin, times as
    round(t / frame_shift) frames)."""
    recs, rows = [], {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p or p[0].startswith(";"):
                continue
            try:
                if len(p) < 4:
                    raise ValueError
                start, end = float(p[2]), float(p[3])
            except ValueError:
                raise ValueError(f"{path}:{ln}: expected `<recording> <channel> <start> <end>`") from None
            b, e = int(round(start / frame_shift)), int(round(end / frame_shift))
            if not start >= 0.0 or e < b:
                raise ValueError(f"{path}:{ln}: a region of {p[0]} runs from {p[2]} to {p[3]}")
            if p[0] not in rows:
                recs.append(p[0])
                rows[p[0]] = []
            rows[p[0]].append((b, e))
    return recs, [np.array(sorted(rows[r]), np.int64).reshape(-1, 2) for r in recs]


class Diarization:
    """The result of diarize(): `reco_ids`, `segments` (as speech_segments), `windows` ((W, 4): recording, segment,
    begin, end), `dropped` (segments too short for a window), `xvectors` ((W, 512) on the device), `labels` ((W,) int64,
    unique over the whole call), `turns` ((N, 4): recording, begin, end, label), and the `clustering` (cluster.Clustering, or
    cluster.SpectralClustering under clusterer="spectral") and `refined` (cluster.Refined or None) they came from."""

    def __init__(self, reco_ids, segments, windows, dropped, xvectors, labels, turns, clustering, refined):
        self.reco_ids, self.segments, self.windows, self.dropped = reco_ids, segments, windows, dropped
        self.xvectors, self.labels, self.turns, self.clustering, self.refined = xvectors, labels, turns, clustering, refined

    def write_rttm(self, path_or_fh, frame_shift=FRAME_SHIFT):
        write_rttm(path_or_fh, self.reco_ids, self.turns, frame_shift)

    def der(self, ref_turns, **kw):
        """metrics.der of the result's own turns against ref_turns (whatever metrics.der takes as `ref`; the recording index of
        bare turns names self.reco_ids); **kw: lengths, uem, collar, skip_overlap, frame_shift."""
        from . import metrics
        return metrics.der(ref_turns, self.turns, reco_ids=self.reco_ids, **kw)


class SweepResult:
    """What sweep_thresholds returns: `thresholds` (K,), `reco_ids` (R), `der` (K,) the pooled rate per threshold,
    `per_recording` (K, R) (NaN: no reference speech, or the cell was not scored), `n_pooled` (K,) the recordings whose
    counts `der` pools, `counts` (K, R, 6) int64 in the order of ops.DER_COUNTS (zeros where not scored) and
    `best_threshold`: the one with the lowest pooled rate (the first of equal ones; None when every rate is NaN)."""

    def __init__(self, thresholds, reco_ids, counts, scored):
        from .derscore import rates
        self.thresholds, self.reco_ids, self.counts = np.asarray(thresholds, np.float64), reco_ids, counts
        conf = counts[..., 4] - counts[..., 5]
        self.per_recording = rates(counts[..., 2], counts[..., 3], conf, counts[..., 1])
        self.per_recording[~scored] = np.nan
        self.n_pooled = scored.sum(axis=1).astype(np.int64)
        self.der = rates(counts[..., 2].sum(axis=1), counts[..., 3].sum(axis=1), conf.sum(axis=1), counts[..., 1].sum(axis=1))
        ok = ~np.isnan(self.der)
        self.best_threshold = float(self.thresholds[np.flatnonzero(ok)[np.argmin(self.der[ok])]]) if ok.any() else None


def sweep_thresholds(diarization, ref_turns, thresholds, reco_ids=None, lengths=None, uem=None, collar=0.25, skip_overlap=False,
                     frame_shift=FRAME_SHIFT):
    """The DER of every cut of a diarization's dendrogram -> SweepResult.  For each threshold t,
    diarization.clustering.cut(t) (on the host) labels the windows; a cell (t, recording) is then exactly
    metrics.der(ref_turns, turns(windows, those labels)) for that recording, but no turns are built: the device is given, once
    per recording, the window that owns each frame (frame_labels' rule does not depend on the labels) and, per cell, one label
    per window, and scores all K x R cells in ONE call.  ref_turns, lengths, uem, collar, skip_overlap: as metrics.der;
    reco_ids: the names that the recording index of a bare ref_turns table refers to (default: the diarization's)
    (recordings of the reference that the diarization does not have are scored against nothing, at every threshold).
    A cell whose cut leaves the recording with more than 64 clusters is not scored: NaN, and its recording is left out of that
    threshold's pool (SweepResult.n_pooled says how many went in); so is a recording with more than 64 reference speakers.
    Raises where the recorded dendrogram does not reach a threshold: a recording whose clustering stopped early (threshold or
    min_clusters of diarize()) must have recorded a merge below the lowest threshold asked for.  The VB-HMM is not part of the
    sweep: the cells score the clustering's cuts, not `refined`."""
    from . import derscore, ops
    clus = diarization.clustering
    if clus is not None and not hasattr(clus, "cut"):
        raise ValueError("this diarization was clustered spectrally: there is no dendrogram to cut (diarize with "
                         'clusterer="ahc" to sweep thresholds)')
    thresholds = [float(t) for t in np.asarray(thresholds, np.float64).reshape(-1)]
    if not thresholds or any(t != t for t in thresholds):
        raise ValueError("give at least one threshold, none of them NaN")
    win = np.asarray(diarization.windows, np.int64).reshape(-1, 4)
    if win.shape[0] and (clus is None or len(clus) != win.shape[0]):
        raise ValueError("the diarization carries no clustering of its windows")
    if clus is not None:
        n, mo = np.diff(clus.offsets), clus._moffs()
        for p in np.flatnonzero(np.asarray(clus.n_merges) < np.maximum(n - 1, 0)).tolist():
            done = clus.merges[mo[p]:mo[p] + int(clus.n_merges[p])]
            if done.size == 0 or not float(done["value"].min()) < min(thresholds):
                raise ValueError(f"the dendrogram of group {p} was recorded down to "
                                 f"{float(done['value'].min()) if done.size else float('inf')}: it does not reach the threshold "
                                 f"{min(thresholds)} (diarize with threshold=-inf, min_clusters=1 to record all of it)")
    dev = derscore._device()
    own = list(diarization.reco_ids)
    rside, rorder = derscore._side(ref_turns, own if reco_ids is None else reco_ids, frame_shift, "ref_turns")
    ids = derscore._recordings(own, rorder)
    extent = {own[r]: int(win[win[:, 0] == r, 3].max()) for r in np.unique(win[:, 0]).tolist()}
    R = derscore.Reference(rside, ids, derscore._lengths(lengths, own if reco_ids is None else reco_ids),
                           derscore._uem(uem, frame_shift), collar, skip_overlap, frame_shift, extent, dev)
    # the window that owns each frame, as an index into its recording's windows
    rows_of = {r: np.flatnonzero(win[:, 0] == r) for r in np.unique(win[:, 0]).tolist()}
    local = np.zeros(win.shape[0], np.int64)
    for idx in rows_of.values():
        local[idx] = np.arange(idx.size)
    frame_item = np.full(R.frame_offsets.rows, -1, np.int32)
    for r, _, b0, fl in frame_labels(win, np.arange(win.shape[0])):
        if own[r] in R.index:
            k = R.index[own[r]]
            f0, T = int(R.frame_offsets.host[k]), int(R.frame_offsets.host[k + 1] - R.frame_offsets.host[k])
            e = min(b0 + fl.size, T)  # (a given length may cut a recording short)
            frame_item[f0 + b0:f0 + e] = np.where(fl[:e - b0] >= 0, local[np.maximum(fl[:e - b0], 0)], -1)
    K, limit = len(thresholds), R.limit
    counts = np.zeros((K, len(ids), len(ops.DER_COUNTS)), np.int64)
    scored = np.zeros((K, len(ids)), bool)
    prob, cells, labels, ioffs = [], [], [], [0]
    cuts = [clus.cut(t).labels if clus is not None else np.zeros(0, np.int64) for t in thresholds]
    for r, rid in enumerate(ids):  # a recording's cells side by side: their workgroups read the same reference masks
        if rid not in R.index:
            continue
        idx = rows_of.get(r, np.zeros(0, np.int64)) if r < len(own) else np.zeros(0, np.int64)
        for k in range(K):
            u, inv = np.unique(cuts[k][idx], return_inverse=True)
            if u.size > limit:
                continue
            prob.append(R.index[rid])
            cells.append((k, r))
            labels.append(inv.astype(np.int32).reshape(-1))
            ioffs.append(ioffs[-1] + idx.size)
    if prob:
        got, _ = R.score(prob, frame_item=torch.from_numpy(frame_item).to(dev),
                         item_offsets=ops.RaggedOffsets(ioffs, dev, max_rows=ops.DER_MAX_FRAMES),
                         item_labels=torch.from_numpy(np.concatenate(labels)).to(dev))
        kk, rr = np.array(cells).T
        counts[kk, rr] = got
        scored[kk, rr] = True
    return SweepResult(thresholds, ids, counts, scored)


def diarize(model, extractor, frames, lengths, reco_ids, segments=None, vad=features.VadOptions(), min_speech=50,
            max_gap=30, cmn_window=300, window=144, shift=24, min_frames=CONTEXT + 2, threshold=0.0, min_clusters=1,
            linkage="average", vb_psi=None, vb=None, workspace_bytes=None, clusterer="ahc", spectral=None):
    """Diarize whole recordings -> Diarization.  frames: (sum T_r, 30) raw MFCC rows on the device, recording r being the
    next lengths[r] rows; reco_ids: their names.  The steps, all on the device but the window bookkeeping:
      1. segments: the given ones (the structure of speech_segments), or features.energy_vad(vad) through
         speech_segments(min_speech, max_gap);
      2. features.cmn_select(mask=None, cmn_window): sliding-window mean subtraction with every frame kept, so that rows
         stay aligned with time;
      3. uniform_windows(window, shift, min_frames);
      4. extractor.extract_windows over the windows' rows (an XVectorNet_ETDNN_12Layer);
      5. cluster.cluster(model, x-vectors, groups=recording, threshold, min_clusters, linkage); or, with
         clusterer="spectral", cluster.spectral_cluster(model, x-vectors, groups=recording, **spectral) (spectral: a dict of
         its neighbours, min_clusters, max_clusters, workspace_bytes; threshold, min_clusters and linkage are not used);
      6. with vb_psi (the PLDA between-class variances): cluster.vb_refine(model, x-vectors, that clustering, vb_psi,
         groups=recording, **vb); a recording's windows are in time order already;
      7. turns()."""
    lengths = [int(T) for T in lengths]
    reco_ids = list(reco_ids)
    if len(reco_ids) != len(lengths):
        raise ValueError(f"{len(reco_ids)} recording names, {len(lengths)} lengths")
    if clusterer not in ("ahc", "spectral"):
        raise ValueError('clusterer must be "ahc" or "spectral"')
    if spectral is not None and clusterer != "spectral":
        raise ValueError('spectral= holds the options of clusterer="spectral"')
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
        if clusterer == "spectral":
            clus = cluster.spectral_cluster(model, x, groups=groups, **(spectral or {}))
        else:
            clus = cluster.cluster(model, x, groups=groups, threshold=threshold, min_clusters=min_clusters, linkage=linkage)
        labels = clus.labels
        if vb_psi is not None:
            refined = cluster.vb_refine(model, x, clus, vb_psi, groups=groups, **(vb or {}))
            labels = refined.labels
    return Diarization(reco_ids, segments, windows, dropped, x, labels, turns(windows, labels), clus, refined)
