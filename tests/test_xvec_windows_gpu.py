"""Sliding-window x-vector extraction (nplda_xvec_extract_windows_f32, XVectorNet_ETDNN_12Layer.extract_windows) and the
diarization chain on top of it (neuralplda_amd/diarize.py) on the MI355X.  The contract is bit identity with the cut-out
route: extract_ragged on a copy of each window's rows."""
import io

import numpy as np
import pytest
import torch

from tests import fp32_units, xvec_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


@pytest.fixture(scope="module")
def params():
    return xvec_ref.make_params()


@pytest.fixture(scope="module")
def extractors(params):
    from neuralplda_amd import models
    out = {}
    for name, fn in (("std", torch.std), ("var", torch.var)):
        m = models.XVectorNet_ETDNN_12Layer(pooling_function=fn)
        out[name] = xvec_ref.load_into(m, params).to(DEV).eval().requires_grad_(False)
    return out


def frames_of(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 30)).astype(np.float32)).to(DEV)


def table_407():
    """407 frames: window 48 / shift 12 over [0, 300), a 24- and a 23-frame window, one across the 128-row tile edge, one
    ending at the last row, one listed twice, the whole shuffled."""
    win = [(b, b + 48) for b in range(0, 300 - 48 + 1, 12)]
    win += [(310, 334), (350, 373), (100, 180), (340, 407), (100, 180)]
    win = np.array(win, np.int64)
    return win[np.random.default_rng(11).permutation(win.shape[0])]


def cutouts(m, frames, win, **kw):
    """The parent route: extract_ragged on a copy of every window's rows."""
    cut = torch.cat([frames[b:e] for b, e in win.tolist()])
    return m.extract_ragged(cut, win[:, 1] - win[:, 0], **kw)


def same(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


@pytest.fixture(scope="module")
def case_407(extractors):
    frames, win = frames_of(407, 1), table_407()
    return frames, win, {k: cutouts(m, frames, win) for k, m in extractors.items()}


@pytest.mark.parametrize("pooling", ["std", "var"])
def test_bit_identity_with_the_cutouts(extractors, case_407, pooling):
    frames, win, ref = case_407
    got = extractors[pooling].extract_windows(frames, win)
    assert got.shape == (win.shape[0], 512) and got.device == frames.device
    short = (win[:, 1] - win[:, 0]) == 23
    assert short.sum() == 1 and torch.isnan(got[np.flatnonzero(short)]).all()   # one pooled row: NaN, as an utterance
    assert torch.isfinite(got[np.flatnonzero(~short)]).all()
    assert same(got, ref[pooling])
    # the table as a tensor and as a list, and frames on the host
    assert same(extractors[pooling].extract_windows(frames, torch.from_numpy(win)), got)
    assert same(extractors[pooling].extract_windows(frames.cpu(), win.tolist()).to(DEV), got)


def test_more_than_one_lin11_tile(extractors):
    m = extractors["std"]
    frames = frames_of(400, 2)
    b = np.arange(0, 400 - 40 + 1, 2, dtype=np.int64)
    win = np.stack([b, b + 40], axis=1)
    assert win.shape[0] == 181
    got = m.extract_windows(frames, win)
    assert torch.isfinite(got).all() and same(got, cutouts(m, frames, win))
    assert torch.equal(got, m.extract_windows(frames, win))


def test_chunking_keeps_the_bits(extractors, case_407):
    from neuralplda_amd import xvector
    frames, win, ref = case_407
    m = extractors["std"]
    for limit, least in ((3 << 20, 3), (1, win.shape[0])):
        chunks = xvector.plan_windows(win, limit)
        assert len(chunks) >= least
        assert same(m.extract_windows(frames, win, workspace_bytes=limit), ref["std"])


def test_uncovered_gap_is_not_run(extractors):
    from neuralplda_amd import xvector
    m = extractors["std"]
    frames = frames_of(400, 4)
    b = np.concatenate([np.arange(0, 60 - 30 + 1, 10), np.arange(340, 400 - 30 + 1, 10)]).astype(np.int64)
    win = np.stack([b, b + 30], axis=1)
    chunks = xvector.plan_windows(win, xvector.MAX_WORKSPACE_BYTES)
    assert sum(c.rows for c in chunks) == 120 and chunks[0].intervals == [(0, 60), (340, 400)]
    got = m.extract_windows(frames, win)
    assert torch.isfinite(got).all() and same(got, cutouts(m, frames, win))


@pytest.mark.parametrize("pooling", ["std", "var"])
def test_windows_in_fp32_units(extractors, params, pooling):
    # gates 3 / 5 (rms / max) of test_xvec_gpu.py, which the values inherit through the bit identity above; measured on
    # MI355X: std 1.68 / 1.59, var 1.71 / 1.80
    frames = frames_of(200, 5)
    win = np.array([(0, 24), (10, 90), (60, 200), (100, 148), (0, 200)], np.int64)
    got = extractors[pooling].extract_windows(frames, win).cpu().numpy()
    f = frames.cpu().numpy()
    cut = np.concatenate([f[b:e] for b, e in win.tolist()])
    lengths = win[:, 1] - win[:, 0]
    ref64 = xvec_ref.extract_ragged(cut, lengths, params, pooling, np.float64)
    ref32 = xvec_ref.extract_ragged(cut.astype(np.float32), lengths, params, pooling, np.float32)
    r = fp32_units.measure(got, ref64, ref32)
    print(f"extract_windows {pooling}: fp32 units {r}")
    fp32_units.assert_fp32_level(got, ref64, ref32, f"extract_windows {pooling}", rms_max=3.0, max_max=5.0)


def test_host_errors(extractors):
    m = extractors["std"]
    frames = frames_of(100, 6)
    with pytest.raises(ValueError, match=r"window 1 = \[60, 101\)"):
        m.extract_windows(frames, [(0, 40), (60, 101)])
    with pytest.raises(ValueError, match=r"window 0 = \[-1, 40\)"):
        m.extract_windows(frames, [(-1, 40)])
    with pytest.raises(ValueError, match=r"window 2 = \[10, 32\) has 22 frames"):
        m.extract_windows(frames, [(0, 40), (5, 28), (10, 32)])
    with pytest.raises(ValueError):
        m.extract_windows(frames, np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError):
        m.extract_windows(frames, np.array([[0.0, 40.0]]))
    with pytest.raises(ValueError):
        m.extract_windows(frames[:, :29], [(0, 40)])
    for empty in ([], np.zeros((0, 2), np.int64)):
        e = m.extract_windows(frames, empty)
        assert e.shape == (0, 512) and e.device == frames.device


def test_diarize_tool_writes_rttm(extractors, tmp_path):
    """tools/diarize.py over a two-line feats.scp, one recording per call, with a segments file and with the VAD: the RTTM
    text is what diarize() gives for each recording, the second recording's speakers counted on from the first's."""
    import importlib
    import os
    import pickle
    import sys
    from neuralplda_amd import diarize, kaldi_format, models
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    tool = importlib.import_module("diarize")
    ext = extractors["std"]
    head = xvec_ref.load_into(models.NeuralPlda(NC()), xvec_ref.make_head()).to(DEV)
    rng = np.random.default_rng(12)
    mats = []
    for T in (400, 300):
        m = np.repeat(rng.standard_normal((4, 30)), 100, axis=0)[:T] + rng.standard_normal((T, 30))
        m[:, 0] += 20.0                 # c0: loud, but for a silence in the middle
        m[T // 2:T // 2 + 60, 0] -= 30.0
        mats.append(m.astype(np.float32))
    kaldi_format.write_feature_ark(str(tmp_path / "f.ark"), ["recA", "recB"], mats, scp_path=str(tmp_path / "feats.scp"))
    (tmp_path / "segments").write_text("recA-1 recA 0.10 1.90\nrecA-2 recA 2.50 3.95\nrecB-1 recB 0.00 2.80\n")
    for name, obj in (("ext.pt", ext), ("head.pt", head)):
        with open(tmp_path / name, "wb") as fh:
            pickle.dump(obj, fh)
    common = ["--feats-scp", str(tmp_path / "feats.scp"), "--xvector-model", str(tmp_path / "ext.pt"), "--model",
              str(tmp_path / "head.pt"), "--window", "60", "--shift", "30", "--min-clusters", "2", "--recordings-per-call", "1"]
    kw = dict(window=60, shift=30, threshold=float("-inf"), min_clusters=2)
    for extra, segs in ((["--segments", str(tmp_path / "segments")], [np.array([[10, 190], [250, 395]]), np.array([[0, 280]])]),
                        (["--min-speech", "30", "--max-gap", "5"], None)):
        tool.main(common + extra + ["--rttm", str(tmp_path / "out.rttm")])
        want, base = io.StringIO(), 0
        for r, name in enumerate(["recA", "recB"]):
            f = torch.from_numpy(mats[r]).to(DEV)
            res = diarize.diarize(head, ext, f, [mats[r].shape[0]], [name], segments=None if segs is None else [segs[r]],
                                  min_speech=30, max_gap=5, **kw)
            assert res.windows.shape[0] >= 5 and res.turns.shape[0] >= 2
            t = res.turns.copy()
            t[:, 3] += base
            base += int(res.labels.max()) + 1
            diarize.write_rttm(want, [name], t)
        got = (tmp_path / "out.rttm").read_text()
        assert got == want.getvalue() and got.count("\n") >= 4 and base == 4
        assert all(ln.split()[0] == "SPEAKER" and len(ln.split()) == 10 for ln in got.splitlines())


def test_diarize_pipeline(extractors, params):
    """Two recordings, a hand-placed VAD mask with a gap, window 60 / shift 30: diarize() against the same chain composed
    by hand from uniform_windows, extract_ragged on cut-outs, cluster.cluster (and vb_refine) and the twin of turns."""
    from neuralplda_amd import cluster, diarize, features, models
    from tests.test_diarize_cpu import twin_turns
    ext = extractors["std"]
    head = xvec_ref.load_into(models.NeuralPlda(NC()), xvec_ref.make_head()).to(DEV)
    lengths = [600, 580]
    rng = np.random.default_rng(8)
    # raw "MFCC" rows with a level that changes every 150 frames, so that windows differ by more than noise
    level = np.repeat(rng.standard_normal((8, 30)), 150, axis=0)[:sum(lengths)]
    frames = torch.from_numpy((level + rng.standard_normal((sum(lengths), 30))).astype(np.float32)).to(DEV)
    mask = np.zeros(sum(lengths), np.uint8)
    mask[20:280] = 1        # recording 0: [20, 280), a 3-frame dip at 100 that closes, a real gap, then [330, 590)
    mask[100:103] = 0
    mask[330:590] = 1
    mask[600 + 0:600 + 15] = 1      # recording 1: a run too short to keep, then [50, 575)
    mask[600 + 50:600 + 575] = 1
    segs = diarize.speech_segments(mask, lengths, min_speech=30, max_gap=5)
    assert [s.tolist() for s in segs] == [[[20, 280], [330, 590]], [[50, 575]]]
    psi = np.random.default_rng(9).uniform(0.5, 4.0, 150)
    kw = dict(segments=segs, window=60, shift=30, threshold=float("-inf"), min_clusters=3)
    res = diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], **kw)
    # by hand
    rows, _ = features.cmn_select(frames, lengths, None, 300, 0)
    assert rows.shape == frames.shape
    win, dropped = diarize.uniform_windows(segs, 60, 30)
    assert dropped == [] and np.array_equal(res.windows, win) and win.shape[0] == 2 * 8 + 17
    starts = np.array([0, 600])
    tab = win[:, 2:4] + starts[win[:, 0]][:, None]
    x = cutouts(ext, rows, tab)
    assert same(res.xvectors, x) and torch.isfinite(x).all()
    c = cluster.cluster(head, x, groups=win[:, 0], threshold=float("-inf"), min_clusters=3)
    assert c.n_clusters.tolist() == [3, 3]
    assert np.array_equal(res.labels, c.labels) and res.refined is None
    want = twin_turns(win, c.labels)
    assert want.shape[0] >= 5 and np.array_equal(res.turns, want)
    # turns tile the segments: every frame of a segment in exactly one turn
    count = np.zeros(sum(lengths), np.int64)
    for r, b, e, _ in res.turns.tolist():
        count[starts[r] + b:starts[r] + e] += 1
    inside = np.zeros(sum(lengths), np.int64)
    for r, s in enumerate(segs):
        for b, e in s.tolist():
            inside[starts[r] + b:starts[r] + e] = 1
    assert np.array_equal(count, inside)
    fh = io.StringIO()
    res.write_rttm(fh)
    lines = fh.getvalue().splitlines()
    assert len(lines) == want.shape[0] and lines[0].startswith("SPEAKER recA 1 0.200 ")
    # with the VB-HMM on
    vb = dict(Fa=0.5, Fb=5.0, loop_prob=0.9, max_iters=10)
    res2 = diarize.diarize(head, ext, frames, lengths, ["recA", "recB"], vb_psi=psi, vb=vb, **kw)
    r = cluster.vb_refine(head, x, c, psi, groups=win[:, 0], **vb)
    assert np.array_equal(res2.labels, r.labels) and np.array_equal(res2.turns, twin_turns(win, r.labels))
    assert same(res2.xvectors, x)
