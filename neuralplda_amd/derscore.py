"""Diarization error rate in integer frames with the optimal speaker mapping (csrc/nplda_der.hip, design/k24_der.md): the
host side of metrics.der and diarize.sweep_thresholds.  Names become indices here, the tables of ops.der are laid out, and
the integers that come back are turned into rates in float64.  What NIST md-eval computes, on a frame grid."""
import os

import numpy as np
import torch

from . import _lib, ops

__all__ = ["der", "DerResult", "Reference"]

COLLAR = 0.25
FRAME_SHIFT = 0.01


def _device():
    if not torch.cuda.is_available():
        raise _lib.NpldaHipError("DER scoring needs a HIP device (there is no CPU implementation)")
    return torch.device("cuda", torch.cuda.current_device())


def _side(x, reco_ids, frame_shift, what):
    """One side of a scoring -> {recording id: [(begin, end, speaker name), ...]} and the ids in order of appearance.
    x: an RTTM path, what diarize.read_rttm returns, or (N, 4) rows (recording index, begin, end, label) as diarize.turns
    gives them, the index naming reco_ids[index] (or itself without reco_ids)."""
    from . import diarize
    if isinstance(x, (str, os.PathLike)):
        x = diarize.read_rttm(x, frame_shift)
    names = None
    if isinstance(x, tuple) and len(x) == 3:
        ids, rows, names = x
    else:
        ids, rows = reco_ids, x
    rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows, dtype=np.int64).reshape(-1, 4)
    if rows.size and (rows[:, 0].min() < 0 or (ids is not None and rows[:, 0].max() >= len(ids))):
        raise ValueError(f"{what}: a turn names a recording outside the {len(ids) if ids is not None else 0} given")
    if rows.size and (rows[:, 1].min() < 0 or (rows[:, 2] < rows[:, 1]).any()):
        raise ValueError(f"{what}: a turn needs 0 <= begin <= end")
    out, order = {}, []
    for r, b, e, lab in rows.tolist():
        rid = ids[r] if ids is not None else r
        if rid not in out:
            out[rid] = []
            order.append(rid)
        out[rid].append((b, e, names[r][lab] if names is not None else str(lab)))
    return out, order


def _uem(uem, frame_shift):
    from . import diarize
    if uem is None:
        return None
    if isinstance(uem, (str, os.PathLike)):
        uem = diarize.read_uem(uem, frame_shift)
    if isinstance(uem, dict):
        return {k: np.asarray(v, np.int64).reshape(-1, 2) for k, v in uem.items()}
    ids, regions = uem
    return {k: np.asarray(v, np.int64).reshape(-1, 2) for k, v in zip(ids, regions)}


def _index(turns):
    """[(begin, end, name)] -> ((n, 3) int32 rows with the names as indices in order of first appearance, the names)."""
    names, idx = [], {}
    rows = np.zeros((len(turns), 3), np.int32)
    for k, (b, e, name) in enumerate(turns):
        if name not in idx:
            idx[name] = len(names)
            names.append(name)
        rows[k] = (b, e, idx[name])
    return rows, names


class Reference:
    """The reference side of a scoring, laid out for ops.der: `reco_ids`, `lengths` (frames), `ref_names` (speaker names per
    recording), `skipped` (recordings with more speakers than the kernel takes: not on the device), `index` (recording id ->
    row of the device tables, kept recordings only) and the device tables themselves.  hyp_extent: {recording id: largest
    end of the hypothesis}, which counts towards a length that is not given."""

    def __init__(self, ref, ids, lengths, uem, collar, skip_overlap, frame_shift, hyp_extent, dev):
        self.limit = int(_lib.load().nplda_der_max_speakers())
        self.collar = int(round(float(collar) / frame_shift))
        if self.collar < 0:
            raise ValueError("the collar must not be negative")
        self.skip_overlap, self.dev = bool(skip_overlap), dev
        self.reco_ids = list(ids)
        self.lengths, self.ref_names, self.skipped, self.index = [], [], [], {}
        tables, regions, offs, roffs, uoffs = [], [], [0], [0], [0]
        for rid in self.reco_ids:
            rows, names = _index(ref.get(rid, []))
            own = uem.get(rid) if uem is not None else None
            if lengths is not None and rid in lengths:
                T = int(lengths[rid])
            else:
                T = max([int(rows[:, 1].max()) if rows.size else 0, int(hyp_extent.get(rid, 0)),
                         int(own[:, 1].max()) if own is not None and own.size else 0])
            if T < 0 or T > ops.DER_MAX_FRAMES:
                raise ValueError(f"recording {rid}: {T} frames")
            self.lengths.append(T)
            self.ref_names.append(names)
            if len(names) > self.limit:
                self.skipped.append(rid)
                continue
            self.index[rid] = len(offs) - 1
            tables.append(rows)
            offs.append(offs[-1] + T)
            roffs.append(roffs[-1] + rows.shape[0])
            if uem is not None:  # a recording the UEM does not list is evaluated whole
                reg = np.clip(own, 0, T).astype(np.int32) if own is not None else np.array([[0, T]], np.int32)
                regions.append(reg)
                uoffs.append(uoffs[-1] + reg.shape[0])
        big = ops.DER_MAX_FRAMES
        self.frame_offsets = ops.RaggedOffsets(offs, dev, max_rows=big)
        self.ref_offsets = ops.RaggedOffsets(roffs, dev, max_rows=big)
        self.ref_turns = torch.from_numpy(np.concatenate(tables) if tables else np.zeros((0, 3), np.int32)).to(dev)
        self.uem_offsets = self.uem = None
        if uem is not None:
            self.uem_offsets = ops.RaggedOffsets(uoffs, dev, max_rows=big)
            self.uem = torch.from_numpy(np.concatenate(regions) if regions else np.zeros((0, 2), np.int32)).to(dev)

    def score(self, prob_reco, **hyp):
        """ops.der for problems over the kept recordings -> (counts (P, 6), map_ref (P, 64)) as numpy arrays."""
        counts, map_ref, _ = ops.der(self.frame_offsets, self.ref_offsets, self.ref_turns, ops.der_problems(prob_reco, self.dev),
                                     uem_offsets=self.uem_offsets, uem=self.uem, collar=self.collar,
                                     skip_overlap=self.skip_overlap, **hyp)
        return counts.cpu().numpy(), map_ref.cpu().numpy()


def rates(miss, fa, conf, total):
    """(miss + fa + conf) / total in float64, NaN where total == 0."""
    err, total = np.asarray(miss + fa + conf, np.float64), np.asarray(total, np.float64)
    return np.divide(err, total, out=np.full(err.shape, np.nan), where=total > 0)


class DerResult:
    """What metrics.der returns.  Per recording, in the order of `reco_ids`: the int64 arrays `scored`, `total`, `miss`, `fa`,
    `conf` and `matched` (frames; zeros for a skipped recording), `lengths`, `mappings` (a dict reference speaker name ->
    hypothesis speaker name per recording, under one optimal mapping; speakers without a partner are absent) and
    `per_recording` (float64 DER, NaN where total == 0 or the recording was skipped).  `skipped`: the recordings with more
    speakers on a side than the kernel takes.  `der`: the POOLED rate, the sum of the errors over the sum of the totals of
    the recordings that were scored (not the mean of the ratios); NaN without any reference speech."""

    def __init__(self, reco_ids, lengths, counts, mappings, skipped):
        self.reco_ids, self.lengths, self.mappings, self.skipped = reco_ids, np.asarray(lengths, np.int64), mappings, skipped
        self.scored, self.total, self.miss, self.fa = (counts[:, k].copy() for k in range(4))
        self.matched = counts[:, 5].copy()
        self.conf = counts[:, 4] - counts[:, 5]
        self.per_recording = rates(self.miss, self.fa, self.conf, self.total)
        gone = np.array([r in set(skipped) for r in reco_ids], bool)
        self.per_recording[gone] = np.nan
        self.der = float(rates(self.miss.sum(), self.fa.sum(), self.conf.sum(), self.total.sum()))

    def lines(self):
        """One line per recording and the overall line, as tools/score_rttm.py prints them."""
        out = []
        for r, rid in enumerate(self.reco_ids):
            if rid in self.skipped:
                out.append(f"{rid} skipped: more speakers on a side than the scorer takes")
                continue
            out.append(f"{rid} DER {100.0 * self.per_recording[r]:.2f}% scored {self.scored[r]} total {self.total[r]} "
                       f"miss {self.miss[r]} fa {self.fa[r]} conf {self.conf[r]}")
        out.append(f"OVERALL DER {100.0 * self.der:.2f}% scored {self.scored.sum()} total {self.total.sum()} "
                   f"miss {self.miss.sum()} fa {self.fa.sum()} conf {self.conf.sum()} "
                   f"({len(self.reco_ids) - len(self.skipped)} of {len(self.reco_ids)} recordings)")
        return out


def _lengths(lengths, reco_ids):
    """lengths as a dict by recording id: a dict already, or a sequence along reco_ids."""
    if lengths is None or isinstance(lengths, dict):
        return lengths
    lengths = [int(T) for T in lengths]
    if reco_ids is None or len(lengths) != len(reco_ids):
        raise ValueError("lengths must be a dict by recording id, or one length per entry of reco_ids")
    return dict(zip(reco_ids, lengths))


def _recordings(reco_ids, *orders):
    ids, seen = [], set()
    for order in ([] if reco_ids is None else [list(reco_ids)]) + list(orders):
        for rid in order:
            if rid not in seen:
                seen.add(rid)
                ids.append(rid)
    return ids


def der(ref, hyp, reco_ids=None, lengths=None, uem=None, collar=COLLAR, skip_overlap=False, frame_shift=FRAME_SHIFT):
    """The diarization error rate of `hyp` against `ref` -> DerResult.  ref, hyp: an RTTM path, what diarize.read_rttm returns
    ((reco_ids, turns, speaker names)), or (N, 4) turns (recording index, begin, end, label) as diarize.turns gives them,
    whose index names reco_ids[index].  Recordings are matched by id; one that a side does not have is scored against an
    empty side.  The result lists reco_ids first (when given), then the other recordings of ref, then of hyp.
    lengths: frames per recording, a dict by id or a sequence along reco_ids; a recording without one is as long as the
    largest end over its reference, hypothesis and UEM.  uem: a UEM path, what diarize.read_uem returns or a dict id ->
    (n, 2) regions; None: every frame is evaluated, and so is a recording that a given UEM does not list.  collar: seconds
    on either side of every reference boundary that are not scored (round(collar / frame_shift) frames); skip_overlap: frames
    with more than one reference speaker are not scored.  A recording with more than 64 speakers on a side is not scored: NaN,
    and named in DerResult.skipped."""
    dev = _device()
    rside, rorder = _side(ref, reco_ids, frame_shift, "ref")
    hside, horder = _side(hyp, reco_ids, frame_shift, "hyp")
    ids = _recordings(reco_ids, rorder, horder)
    regions = _uem(uem, frame_shift)
    extent = {rid: max(e for _, e, _ in t) for rid, t in hside.items() if t}
    R = Reference(rside, ids, _lengths(lengths, reco_ids), regions, collar, skip_overlap, frame_shift, extent, dev)
    prob, tables, hoffs, hnames, skipped = [], [], [0], {}, list(R.skipped)
    for rid in ids:
        rows, names = _index(hside.get(rid, []))
        hnames[rid] = names
        if rid not in R.index:
            continue
        if len(names) > R.limit:
            skipped.append(rid)
            continue
        prob.append(R.index[rid])
        tables.append(rows)
        hoffs.append(hoffs[-1] + rows.shape[0])
    counts = np.zeros((len(ids), len(ops.DER_COUNTS)), np.int64)
    mappings = [{} for _ in ids]
    if prob:
        turns = torch.from_numpy(np.concatenate(tables)).to(dev)
        got, maps = R.score(prob, hyp_offsets=ops.RaggedOffsets(hoffs, dev, max_rows=ops.DER_MAX_FRAMES), hyp_turns=turns)
        k = 0
        for r, rid in enumerate(ids):
            if rid in R.index and rid not in skipped:
                counts[r] = got[k]
                mappings[r] = {R.ref_names[r][i]: hnames[rid][j] for i, j in enumerate(maps[k][:len(R.ref_names[r])]) if j >= 0}
                k += 1
    return DerResult(ids, R.lengths, counts, mappings, [rid for rid in ids if rid in set(skipped)])
