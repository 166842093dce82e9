"""ops.der (csrc/nplda_der.hip), metrics.der, diarize.sweep_thresholds and tools/score_rttm.py on the GPU against the numpy
twin of tests/der_ref.py.  Every comparison is equality of integers.  The returned mapping is not compared with scipy's
(optima may tie): it must be one-to-one, within range and reach the twin's `matched`."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import der_ref as dr
from tests.test_der_cpu import HAND

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES_T = [1, 2, 63, 64, 65, 300, 4097]             # 4097: one frame into a second chunk of the counting kernel
SHAPES_S = [(1, 1), (1, 64), (64, 1), (64, 64), (3, 5), (5, 3), (0, 3), (3, 0), (0, 0)]
RAGGED = [0, 0, 17, 1, 0, 65, 300, 0, 64, 2, 0]      # empty recordings first, in the middle and last


def _cat(tables, cols):
    tables = [np.asarray(t, np.int64).reshape(-1, cols) for t in tables]
    offs = np.concatenate([[0], np.cumsum([t.shape[0] for t in tables])]).astype(np.int64)
    return offs, (np.concatenate(tables) if tables else np.zeros((0, cols), np.int64)).astype(np.int32)


def run(lengths, refs, problems, uems=None, collar=0, skip_overlap=False, items=None, **kw):
    """lengths, refs (turn tables), uems per recording; problems: [(recording, hypothesis)], the hypothesis a turn table or,
    with `items` (frame_item per recording), a label vector -> (counts, map_ref, C) as numpy arrays."""
    from neuralplda_amd import ops
    dev = torch.device(DEV)
    fo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ro, rt = _cat(refs, 3)
    args = dict(collar=collar, skip_overlap=skip_overlap, want_matrix=True, **kw)
    if uems is not None:
        uo, ut = _cat(uems, 2)
        args.update(uem_offsets=uo, uem=torch.from_numpy(ut).to(dev))
    if items is None:
        ho, ht = _cat([h for _, h in problems], 3)
        args.update(hyp_offsets=ho, hyp_turns=torch.from_numpy(ht).to(dev))
    else:
        labs = [np.asarray(h, np.int32).reshape(-1) for _, h in problems]
        io = np.concatenate([[0], np.cumsum([v.size for v in labs])]).astype(np.int64)
        fi = np.concatenate([np.asarray(v, np.int32).reshape(-1) for v in items] + [np.zeros(0, np.int32)])
        args.update(frame_item=torch.from_numpy(fi).to(dev), item_offsets=io,
                    item_labels=torch.from_numpy(np.concatenate(labs + [np.zeros(0, np.int32)])).to(dev))
    out = ops.der(fo, ro, torch.from_numpy(rt).to(dev), [r for r, _ in problems], **args)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check(got, k, want, Sr=64, Sh=64, what=""):
    """Problem k of a call against the twin's counts."""
    counts, maps, C = got
    names = ("scored", "total", "miss", "fa", "summin", "matched")
    assert counts[k].tolist() == [want[n] for n in names], (what, dict(zip(names, counts[k].tolist())), {n: want[n] for n in names})
    full = np.zeros((64, 64), np.int64)
    full[:Sr, :Sh] = want.C
    assert np.array_equal(C[k], full), what
    m = maps[k]
    pairs = [(i, int(j)) for i, j in enumerate(m) if j >= 0]
    assert all(i < Sr and j < Sh for i, j in pairs) and (m >= -1).all(), what
    assert len({j for _, j in pairs}) == len(pairs), what                          # one to one
    assert all(full[i, j] > 0 for i, j in pairs), what
    assert sum(int(full[i, j]) for i, j in pairs) == want.matched, what
    if Sr <= dr.MAX_BRUTE and Sh <= dr.MAX_BRUTE:
        assert dr.best_mapping_brute(want.C)[0] == want.matched, what


def make_uem(T):
    return np.array([[0, T // 3], [T // 2, T - T // 8], [T - T // 16, T]], np.int64)


@pytest.mark.parametrize("T", SHAPES_T)
def test_shapes_collars_overlap_and_uem(T):
    """A recording per speaker-count pair, each with its own hypothesis, for every collar, with and without skip_overlap;
    the calls with collar 1 carry three UEM regions.  Up to four speakers at once on either side; turns shorter than the
    collar, collars past both ends (T <= 25 all of them) and overlapping collars all occur in the random turns."""
    rng = np.random.default_rng(1000 + T)
    refs = [dr.random_turns(rng, T, Sr, 2 * Sr + 3, max(T // 3, 1)) for Sr, _ in SHAPES_S]
    hyps = [dr.random_turns(rng, T, Sh, 2 * Sh + 3, max(T // 3, 1)) for _, Sh in SHAPES_S]
    if T >= 63:
        assert max(dr.activity(refs[3], 64, T).sum(axis=0).max(), dr.activity(hyps[3], 64, T).sum(axis=0).max()) >= 3
    n = len(SHAPES_S)
    for collar in (0, 1, 25):
        uem = make_uem(T) if collar == 1 else None
        for skip in (False, True):
            got = run([T] * n, refs, list(enumerate(hyps)), [uem] * n if uem is not None else None, collar, skip)
            for k, (Sr, Sh) in enumerate(SHAPES_S):
                want = dr.der_counts(refs[k], hyps[k], T, Sr, Sh, uem, collar, skip)
                check(got, k, want, Sr, Sh, f"T {T} S {Sr, Sh} collar {collar} skip {skip}")


def test_collar_edges():
    cases = [(30, [(10, 12, 0)], 25),                                  # wider than the turn, past both ends: nothing is scored
             (40, [(10, 12, 0), (30, 31, 1)], 1),
             (300, [(100, 110, 0), (112, 130, 1), (129, 131, 0)], 5),  # the collars of neighbouring turns overlap
             (300, [(0, 300, 0), (150, 150, 1)], 25),                  # an empty turn has a collar too; the ends of the recording
             (64, [(0, 64, 0)], 1)]
    for T, ref, collar in cases:
        hyp = [(0, T, 0), (T // 2, T, 1)]
        got = run([T], [ref], [(0, hyp)], collar=collar)
        want = dr.der_counts(ref, hyp, T, 2, 2, collar=collar)
        check(got, 0, want, 2, 2, (T, ref, collar))
    assert run([30], [cases[0][1]], [(0, [(0, 30, 0)])], collar=25)[0][0].tolist() == [0] * 6


def test_ragged_call_with_shared_recordings():
    rng = np.random.default_rng(7)
    S = [0, 3, 5, 1, 0, 64, 7, 2, 12, 2, 4]
    refs = [dr.random_turns(rng, T, s, 2 * s + 2, max(T // 2, 1)) for T, s in zip(RAGGED, S)]
    uems = [make_uem(T) if r % 2 else np.array([[0, T]]) for r, T in enumerate(RAGGED)]
    uems[6] = np.zeros((0, 2), np.int64)                                 # a recording without a region: nothing is scored
    reco = [0, 6, 6, 5, 10, 2, 6, 4, 5, 3, 8, 9, 1, 7, 6, 0]             # empty recordings first, in the middle and last
    problems = []
    for k, r in enumerate(reco):
        Sh = [0, 3, 64, 5][k % 4]
        problems.append((r, dr.random_turns(rng, RAGGED[r], Sh, 0 if k in (1, 8, 15) else 2 * Sh + 2, max(RAGGED[r] // 2, 1))))
    for uem_on in (False, True):
        got = run(RAGGED, refs, problems, uems if uem_on else None, collar=2, skip_overlap=uem_on)
        for k, (r, hyp) in enumerate(problems):
            want = dr.der_counts(refs[r], hyp, RAGGED[r], 64, 64, uems[r] if uem_on else None, 2, uem_on)
            check(got, k, want, what=f"problem {k} of recording {r}")
        if uem_on:
            assert all(got[0][k].tolist() == [0] * 6 for k, r in enumerate(reco) if r == 6)
        one = run(RAGGED, refs, problems[3:4], uems if uem_on else None, collar=2, skip_overlap=uem_on)
        assert all(np.array_equal(a[0], b[3]) for a, b in zip(one, got))   # a problem does not depend on its neighbours


def test_ties_and_repeatability():
    T = 200
    ref = [(0, 100, 0), (100, 200, 1), (50, 150, 2)]
    twins = [(0, 200, 0), (0, 200, 1), (0, 200, 5)]                      # identical hypothesis speakers: every mapping ties
    apart = [(150, 200, 0), (160, 200, 3)]
    problems = [(0, twins), (1, apart), (0, []), (0, twins)]
    refs = [ref, [(0, 100, 0), (20, 90, 1)]]
    got = run([T, T], refs, problems)
    for k, (r, hyp) in enumerate(problems):
        check(got, k, dr.der_counts(refs[r], hyp, T), what=f"problem {k}")
    assert got[0][0, 5] == 300 and got[0][1, 5] == 0 and (got[1][1] == -1).all() and (got[1][2] == -1).all()
    assert np.array_equal(got[1][0], got[1][3])
    again = run([T, T], refs, problems)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))     # the tie rule is fixed: the same bits


def test_both_hypothesis_forms_agree():
    """Hypotheses with one speaker at a time, once as turns and once as frame_item + labels; items without a speaker (label
    -1) and frames without an item (frame_item -1) included, and labels / items outside the limits count as absent."""
    rng = np.random.default_rng(11)
    lengths, refs, items, bounds = [], [], [], []
    for T in (1, 64, 300, 4097, 0, 5000):
        cuts = np.unique(np.concatenate([[0, T], rng.integers(0, T + 1, max(T // 40, 1))]))
        fi = np.full(T, -1, np.int32)
        for w, (b, e) in enumerate(zip(cuts[:-1], cuts[1:])):
            fi[b:e] = w
        fi[rng.random(T) < 0.1] = -1
        if T >= 300:
            fi[7] = cuts.size + 5                                        # an item the problem does not have
        lengths.append(T)
        items.append(fi)
        bounds.append(cuts)
        refs.append(dr.random_turns(rng, T, 6, 14, max(T // 4, 1)))
    problems_l, problems_t = [], []
    for r in (0, 1, 2, 3, 3, 4, 5, 5, 5):
        W = bounds[r].size - 1
        lab = rng.integers(-1, 9, W).astype(np.int32)
        if W > 3:
            lab[1] = 70                                                  # outside the limit: no speaker
        problems_l.append((r, lab))
        A = dr.items_activity(items[r], lab, 64, lengths[r])
        turns = [(int(t), int(t) + 1, int(s)) for s, t in zip(*np.nonzero(A))]   # a turn per frame: also many turns
        problems_t.append((r, turns))
    for collar, skip in ((0, False), (3, True)):
        a = run(lengths, refs, problems_l, collar=collar, skip_overlap=skip, items=items)
        b = run(lengths, refs, problems_t, collar=collar, skip_overlap=skip)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        for k, (r, lab) in enumerate(problems_l):
            want = dr.der_counts_items(refs[r], items[r], lab, lengths[r], collar=collar, skip_overlap=skip)
            check(a, k, want, what=f"problem {k}")
    # a lower speaker limit drops the labels and turns above it
    a = run(lengths, refs, problems_l, items=items, n_hyp_speakers=4, n_ref_speakers=3)
    for k, (r, lab) in enumerate(problems_l):
        check(a, k, dr.der_counts_items(refs[r], items[r], lab, lengths[r], 3, 4), 3, 4, what=f"limits, problem {k}")


def test_one_long_problem():
    T, S = 70_000, 64
    rng = np.random.default_rng(5)
    ref, hyp = dr.random_turns(rng, T, S, 3000, 1500, 8), dr.random_turns(rng, T, S, 3000, 1500, 8)   # up to eight at once
    got = run([T], [ref], [(0, hyp)], collar=5)
    want = dr.der_counts(ref, hyp, T, collar=5)
    assert want.total > 2 * T and (want.C > 0).sum() > 3000 and want.C.max() > 1000      # (the inputs are what they are meant to be)
    check(got, 0, want)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def _write_case(tmp_path, cases, frame_shift=0.01):
    from neuralplda_amd import diarize
    ids = [c[0] for c in cases]
    ref = np.array([(r, b, e, s) for r, c in enumerate(cases) for b, e, s in c[1]], np.int64).reshape(-1, 4)
    hyp = np.array([(r, b, e, s + 10) for r, c in enumerate(cases) for b, e, s in c[2]], np.int64).reshape(-1, 4)
    diarize.write_rttm(str(tmp_path / "ref.rttm"), ids, ref, frame_shift)
    diarize.write_rttm(str(tmp_path / "hyp.rttm"), ids, hyp, frame_shift)
    return ids, ref, hyp


def test_metrics_der_and_the_tool_on_the_hand_worked_cases(tmp_path, capsys):
    from neuralplda_amd import metrics
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import score_rttm
    for name, ref, hyp, T, opt, (scored, total, miss, fa, conf, rate) in HAND:
        ids, rt, ht = _write_case(tmp_path, [(name, ref, hyp)])
        kw = dict(collar=opt["collar"] * 0.01, skip_overlap=opt.get("skip_overlap", False))
        argv = ["--ref", str(tmp_path / "ref.rttm"), "--hyp", str(tmp_path / "hyp.rttm"), "--collar", str(kw["collar"])]
        if "uem" in opt:
            (tmp_path / "x.uem").write_text("".join(f"{name} 1 {b * 0.01:.2f} {e * 0.01:.2f}\n" for b, e in opt["uem"]))
            kw["uem"] = str(tmp_path / "x.uem")
            argv += ["--uem", kw["uem"]]
        if kw["skip_overlap"]:
            argv.append("--skip-overlap")
        for res in (metrics.der(str(tmp_path / "ref.rttm"), str(tmp_path / "hyp.rttm"), lengths={name: T}, **kw),
                    metrics.der(rt, ht, reco_ids=ids, lengths=[T], **{**kw, "uem": {name: opt["uem"]} if "uem" in opt else None})):
            assert (res.scored[0], res.total[0], res.miss[0], res.fa[0], res.conf[0]) == (scored, total, miss, fa, conf), name
            assert res.der == rate and res.per_recording[0] == rate and res.skipped == []
        if name == "plain":
            assert res.mappings == [{"0": "10", "1": "11"}]
        score_rttm.main(argv)                                            # (no lengths: T is the largest end, 20 or 15)
        out = capsys.readouterr().out.splitlines()
        assert len(out) == 2 and out[1].startswith(f"OVERALL DER {100 * rate:.2f}% ") and out[0].startswith(f"{name} DER {100 * rate:.2f}% ")
        assert f"total {total} miss {miss} fa {fa} conf {conf}" in out[1]


def test_metrics_der_pools_counts_and_skips_crowded_recordings(tmp_path):
    from neuralplda_amd import metrics
    rng = np.random.default_rng(2)
    T = 900
    cases = [("a", dr.random_turns(rng, T, 4, 12, 300), dr.random_turns(rng, T, 5, 12, 300)),
             ("crowd", [(k, k + 5, k) for k in range(65)], [(0, 300, 0)]),           # 65 reference speakers
             ("b", dr.random_turns(rng, T, 3, 9, 300), dr.random_turns(rng, T, 2, 9, 300)),
             ("crowd2", [(0, 300, 0)], [(k, k + 5, k) for k in range(65)])]
    ids, rt, ht = _write_case(tmp_path, cases)
    ref_only = np.array([[4, 10, 200, 0]], np.int64)                                # a recording the hypothesis lacks
    hyp_only = np.array([[5, 0, 50, 3]], np.int64)
    ids6 = ids + ["ref-only", "hyp-only"]
    res = metrics.der(np.concatenate([rt, ref_only]), np.concatenate([ht, hyp_only]), reco_ids=ids6, collar=0.05,
                      lengths={"a": T, "b": T})
    assert res.reco_ids == ids6 and res.skipped == ["crowd", "crowd2"]
    assert np.isnan(res.per_recording[[1, 3, 5]]).all() and res.per_recording[4] == 1.0
    tot = np.zeros(5, np.int64)
    for r in (0, 2):
        want = dr.der_counts(cases[r][1], cases[r][2], T, collar=5)
        assert [res.scored[r], res.total[r], res.miss[r], res.fa[r], res.conf[r]] == [want.scored, want.total, want.miss, want.fa, want.conf]
        assert res.per_recording[r] == dr.der_value(want)
        m = res.mappings[r]
        assert sum(want.C[int(i), int(j) - 10] for i, j in m.items()) == want.matched and len(set(m.values())) == len(m)
        tot += [want.total, want.miss, want.fa, want.conf, 0]
    # ref-only: [10, 200) less the collar 5 at both ends: 180 frames, all missed; hyp-only: 50 frames of false alarm
    assert (res.total[4], res.miss[4], res.fa[5], res.total[5]) == (180, 180, 50, 0)
    assert res.der == (tot[1] + tot[2] + tot[3] + 180 + 50) / (tot[0] + 180)
    files = metrics.der(str(tmp_path / "ref.rttm"), str(tmp_path / "hyp.rttm"), collar=0.05, lengths={"a": T, "b": T})
    assert files.skipped == ["crowd", "crowd2"] and np.array_equal(files.total[:4], res.total[:4]) and np.array_equal(files.conf[:4], res.conf[:4])


def _dendrogram(rng, n):
    """A full random dendrogram over n rows as cluster.Clustering records it: values decrease, a < b are smallest members."""
    from neuralplda_amd import ops
    rec = np.zeros(max(n - 1, 0), ops.AHC_MERGE_DTYPE)
    live, size = list(range(n)), [1] * n
    vals = np.sort(rng.normal(0.0, 1.0, max(n - 1, 0)))[::-1]
    for k in range(n - 1):
        a, b = sorted(rng.choice(len(live), 2, replace=False).tolist())
        a, b = live[a], live[b]
        size[a] += size[b]
        live.remove(b)
        rec[k] = (a, b, vals[k], size[a], 0)
    return rec


def synthetic_diarization(seed=0):
    from neuralplda_amd import cluster, diarize
    rng = np.random.default_rng(seed)
    segments = [np.array([[0, 2000], [2100, 3000]]), np.array([[10, 700], [800, 1200]]), np.zeros((0, 2), np.int64),
                np.array([[0, 800]])]
    windows, dropped = diarize.uniform_windows(segments, 144, 24)
    counts = np.bincount(windows[:, 0], minlength=4)
    assert counts[0] > 100 and counts[2] == 0
    present = [r for r in range(4) if counts[r]]
    offsets = np.concatenate([[0], np.cumsum(counts[present])]).astype(np.int64)
    merges = np.concatenate([_dendrogram(rng, int(counts[r])) for r in present])
    W = windows.shape[0]
    labels = np.repeat(np.arange(len(present)), counts[present]).astype(np.int64)
    clus = cluster.Clustering(labels, np.ones(len(present), np.int32), merges, offsets, np.arange(W, dtype=np.int64),
                              np.maximum(counts[present] - 1, 0).astype(np.int32))
    ids = ["r0", "r1", "r2", "r3"]
    d = diarize.Diarization(ids, segments, windows, dropped, None, labels, diarize.turns(windows, labels), clus, None)
    ref = np.concatenate([np.concatenate([np.full((t.shape[0], 1), r), t], axis=1) for r, t in
                          enumerate([dr.random_turns(rng, 3000, 4, 30, 400), dr.random_turns(rng, 1200, 3, 14, 300),
                                     dr.random_turns(rng, 500, 2, 4, 200), dr.random_turns(rng, 800, 2, 8, 300)])]).astype(np.int64)
    return d, ref


def test_sweep_thresholds_equals_metrics_der_on_every_cut():
    """Six thresholds over four recordings (one without windows).  The two highest leave recording r0 (more than 100 windows)
    with more than 64 clusters: NaN there, and r0 is left out of those thresholds' pools; 22 of the 24 cells are scored."""
    from neuralplda_amd import diarize, metrics
    d, ref = synthetic_diarization()
    thresholds = [3.0, 0.9, -0.3, -0.7, -1.2, -4.0]
    n0 = [int(np.unique(d.clustering.cut(t).labels[d.windows[:, 0] == 0]).size) for t in thresholds]
    assert [n > 64 for n in n0] == [True, True, False, False, False, False] and n0[-1] == 1
    kw = dict(collar=0.1, skip_overlap=True)
    sw = diarize.sweep_thresholds(d, ref, thresholds, **kw)
    assert sw.reco_ids == d.reco_ids and sw.per_recording.shape == (6, 4) and sw.n_pooled.tolist() == [3, 3, 4, 4, 4, 4]
    assert np.isnan(sw.per_recording[:2, 0]).all() and not np.isnan(sw.per_recording[2:]).any()
    assert (~np.isnan(sw.per_recording)).sum() * 4 >= 3 * sw.per_recording.size
    for k, t in enumerate(thresholds):
        res = metrics.der(ref, diarize.turns(d.windows, d.clustering.cut(t).labels), reco_ids=d.reco_ids, **kw)
        assert res.skipped == (["r0"] if k < 2 else [])
        want = np.stack([res.scored, res.total, res.miss, res.fa, res.conf + res.matched, res.matched], axis=1)
        keep = [r for r in range(4) if d.reco_ids[r] not in res.skipped]
        assert np.array_equal(sw.counts[k][keep], want[keep]) and (not sw.counts[k, 0].any()) == (k < 2)
        assert np.array_equal(sw.per_recording[k], res.per_recording, equal_nan=True) and sw.der[k] == res.der
    assert sw.best_threshold == thresholds[int(np.nanargmin(sw.der))]
    own = d.der(ref, **kw)
    full = metrics.der(ref, d.turns, reco_ids=d.reco_ids, **kw)
    assert own.der == full.der == sw.der[-1] and np.array_equal(own.conf, full.conf)
    # the twin on one cell, so that the chain does not only agree with itself
    t = thresholds[3]
    lab = d.clustering.cut(t).labels
    hyp = [(b, e, s) for r, b, e, s in diarize.turns(d.windows, lab).tolist() if r == 1]
    _, inv = np.unique([s for _, _, s in hyp], return_inverse=True)
    want = dr.der_counts(ref[ref[:, 0] == 1][:, 1:], [(b, e, int(s)) for (b, e, _), s in zip(hyp, inv)], int(full.lengths[1]),
                         collar=10, skip_overlap=True)
    assert sw.counts[3, 1].tolist() == [want.scored, want.total, want.miss, want.fa, want.summin, want.matched]


def test_sweep_needs_a_dendrogram_that_reaches_its_thresholds():
    from neuralplda_amd import diarize
    d, ref = synthetic_diarization(1)
    short = d.clustering.cut(0.0)                                         # recorded down to 0.0 only
    d.clustering = short
    with pytest.raises(ValueError, match="does not reach"):
        diarize.sweep_thresholds(d, ref, [0.5, -0.5])
    assert diarize.sweep_thresholds(d, ref, [1.5, 1.0]).der.shape == (2,)


def test_capture_and_replay():
    from neuralplda_amd import ops
    dev = torch.device(DEV)
    rng = np.random.default_rng(9)
    lengths = [300, 0, 4097]
    refs = [dr.random_turns(rng, T, 5, 12, max(T // 3, 1)) for T in lengths]
    reco = [2, 0, 1, 2]
    hyps = [dr.random_turns(rng, lengths[r], 7, 12, max(lengths[r] // 3, 1)) for r in reco]
    big = ops.DER_MAX_FRAMES
    fo = ops.RaggedOffsets(np.concatenate([[0], np.cumsum(lengths)]), dev, max_rows=big)
    ro_h, rt = _cat(refs, 3)
    ho_h, ht = _cat(hyps, 3)
    ro, ho = ops.RaggedOffsets(ro_h, dev, max_rows=big), ops.RaggedOffsets(ho_h, dev, max_rows=big)
    rt, ht, prob = torch.from_numpy(rt).to(dev), torch.from_numpy(ht).to(dev), ops.der_problems(reco, dev)

    def call():
        return ops.der(fo, ro, rt, prob, hyp_offsets=ho, hyp_turns=ht, collar=3, want_matrix=True)

    eager = [t.cpu().numpy().tobytes() for t in call()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert [t.cpu().numpy().tobytes() for t in out] == eager
    got = tuple(t.cpu().numpy() for t in out)
    for k, r in enumerate(reco):
        check(got, k, dr.der_counts(refs[r], hyps[k], lengths[r], collar=3), what=f"problem {k}")


def test_degenerate_arguments_raise():
    from neuralplda_amd import ops
    dev = torch.device(DEV)
    rt = torch.tensor([[0, 5, 0]], dtype=torch.int32, device=dev)
    ok = dict(hyp_offsets=[0, 1], hyp_turns=rt)
    out = ops.der([0, 10], [0, 1], rt, [0], **ok)
    assert out[0].tolist() == [[10, 5, 0, 0, 5, 5]] and out[1][0, 0].item() == 0 and out[2] is None
    empty = ops.der([0, 10], [0, 1], rt, [], hyp_offsets=[0], hyp_turns=rt[:0])
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 64)
    for bad in (dict(collar=-1), dict(n_ref_speakers=65), dict(n_hyp_speakers=-1), dict(uem_offsets=[0, 0])):
        with pytest.raises(ValueError):
            ops.der([0, 10], [0, 1], rt, [0], **ok, **bad)
    for args, kw in ((([0, 10], [0, 1], rt, [1]), ok), (([0, 10], [0, 2], rt, [0]), ok), (([0, 10], [0, 1, 1], rt, [0]), ok),
                     (([0, 10], [0, 1], rt, [0]), dict(hyp_offsets=[0, 1, 1], hyp_turns=rt)),
                     (([0, 10], [0, 1], rt, [0]), dict()), (([0, 10], [0, 1], rt, [0]), dict(item_offsets=[0, 0], **ok)),
                     (([0, 10], [0, 1], rt, [0]), dict(item_offsets=[0, 1], item_labels=rt[0, :1])),
                     (([0, 10], [0, 1], rt, [0]), dict(item_offsets=[0, 1], item_labels=rt[0, :1], frame_item=rt[0, :2]))):
        with pytest.raises(ValueError):
            ops.der(*args, **kw)
    with pytest.raises(TypeError):
        ops.der([0, 10], [0, 1], rt.float(), [0], **ok)
