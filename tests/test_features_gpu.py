"""The feature front end on the MI355X (csrc/nplda_feat.hip through neuralplda_amd/features.py) against the fp64 restatement
tests/feat_ref.py: decode, energy VAD, sliding CMN + select, their composition with the extractor, and the extraction CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from neuralplda_amd import features, kaldi_format as kf
from tests import feat_ref, fp32_units, xvec_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
VAD_SEED = 0        # seeds for which the *_clear_of_the_threshold conditions hold (searched on the CPU)
COMPOSE_SEED = 0
MARGIN = 1e-3


def _mfcc_like(rng, T):
    """c0 near 10 - 20, the high cepstra near 0."""
    x = rng.standard_normal((T, 30)) * np.linspace(3.0, 0.3, 30)
    x[:, 0] += 14.0
    return x


def _speech_silence(rng, T, start=None):
    """c0 in runs of 5 .. 200 frames, silence N(2, 1) and speech N(13, 1) in turn."""
    c0 = np.empty(T)
    t, speech = 0, bool(rng.integers(2)) if start is None else start
    while t < T:
        n = min(int(rng.integers(5, 201)), T - t)
        c0[t:t + n] = rng.normal(13.0 if speech else 2.0, 1.0, n)
        t, speech = t + n, not speech
    return c0


def _archive(tmp_path, items, order=None, name="feats"):
    ark, scp = str(tmp_path / f"{name}.ark"), str(tmp_path / f"{name}.scp")
    offs = feat_ref.write_ark(ark, items)
    feat_ref.write_scp(scp, ark, offs, order or [k for k, _, _ in items])
    return scp


def _extractor(params):
    from neuralplda_amd import models
    m = models.XVectorNet_ETDNN_12Layer()
    xvec_ref.load_into(m, params)
    return m.to(DEV).eval().requires_grad_(False)


# ---- 6. decode ----------------------------------------------------------------------------------------------------------

def test_decode_every_value(tmp_path):
    rng = np.random.default_rng(6)
    fmts = ["CM", "FM", "CM2", "CM3", "DM"]
    plan = [(1, "CM"), (63, "CM"), (64, "CM"), (65, "CM"), (0, "CM"), (2000, "CM"), (1, "FM"), (0, "FM"), (65, "CM2"),
            (63, "CM3"), (64, "DM"), (1999, "FM")]
    plan += [(int(t), fmts[i % 5]) for i, t in enumerate(rng.integers(1, 2001, 52))]
    Ts = [T for T, _ in plan]
    items = [(f"u{i:02d}", _mfcc_like(rng, T), f) for i, (T, f) in enumerate(plan)]
    assert len(items) == 64 and {f for _, _, f in items} == set(fmts)
    feats = kf.load_feature_scp(_archive(tmp_path, items))
    frames, lengths = features.decode_features(feats, DEV)
    assert lengths == Ts and frames.shape == (sum(Ts), 30) and frames.dtype == torch.float32
    got = frames.cpu().numpy()
    assert np.isfinite(got).all()
    off = np.concatenate([[0], np.cumsum(Ts)])
    worst = 0.0
    for i, (key, mat, fmt) in enumerate(items):
        ref, bound = feat_ref.decode(feat_ref.encode(mat, fmt))
        g = got[off[i]:off[i + 1]]
        assert g.shape == ref.shape, key
        if ref.size:
            err = float(np.abs(g - ref).max())
            worst = max(worst, err / bound)
            assert err <= bound, (key, fmt, err, bound)
            if fmt == "FM":
                assert np.array_equal(g, ref.astype(np.float32)), key
    print(f"decode: worst error {worst:.3f} of the 4-ulp bound")  # measured on MI355X: 0.125
    again, _ = features.decode_features(feats, DEV)
    assert torch.equal(frames, again)


# ---- 7. energy VAD ------------------------------------------------------------------------------------------------------

def _vad_utterances(seed):
    rng = np.random.default_rng(seed)
    c0s = [_speech_silence(rng, int(T)) for T in list(rng.integers(5, 3000, 36)) + [1, 2, 3, 5, 700]]
    c0s.append(rng.normal(2.0, 1.0, 400))    # all silence
    c0s.append(rng.normal(13.0, 1.0, 400))   # all speech
    return [c.astype(np.float32) for c in c0s], rng


VAD_SETTINGS = [features.VadOptions(), features.VadOptions(5.0, 0.4, 0.5, 3), features.VadOptions(5.5, 0.5, 0.12, 0)]


def test_vad_inputs_are_clear_of_the_threshold():
    """A condition on the committed seed's inputs (no frame is excluded): no c0 lies within 1e-3 of its utterance's
    threshold, so that an fp32-vs-fp64 difference of the mean (< 1e-5 at these magnitudes) cannot move a decision."""
    c0s, _ = _vad_utterances(VAD_SEED)
    for o in VAD_SETTINGS:
        for c0 in c0s:
            thr = feat_ref.vad_threshold(c0, o.energy_threshold, o.energy_mean_scale)
            assert np.abs(c0.astype(np.float64) - thr).min() > MARGIN


@pytest.mark.parametrize("opts", VAD_SETTINGS, ids=["vad.conf", "half-of-7", "no-context"])
def test_vad_equals_the_restatement(opts):
    c0s, rng = _vad_utterances(VAD_SEED)
    for c0 in c0s:
        thr = feat_ref.vad_threshold(c0, opts.energy_threshold, opts.energy_mean_scale)
        assert np.abs(c0.astype(np.float64) - thr).min() > MARGIN
    lengths = [len(c) for c in c0s]
    x = rng.standard_normal((sum(lengths), 30)).astype(np.float32)
    x[:, 0] = np.concatenate(c0s)
    mask = features.energy_vad(torch.from_numpy(x).to(DEV), lengths, opts).cpu().numpy()
    ref = np.concatenate([feat_ref.vad_energy(c0, *opts) for c0 in c0s])
    assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    bad = np.nonzero(mask.astype(bool) != ref)[0]
    assert bad.size == 0, (bad[:10], len(bad))
    off = np.concatenate([[0], np.cumsum(lengths)])
    assert mask[off[-3]:off[-2]].sum() == 0 and mask[off[-2]:].mean() > 0.5  # the all-silence and the all-speech utterance
    assert 0.2 < ref.mean() < 0.9


# ---- 8. sliding CMN + select ------------------------------------------------------------------------------------------------

EDGE_T = [1, 2, 149, 150, 151, 299, 300, 301, 302, 1000, 5000]


def _cmn_case(tmp_path, Ts, seed, with_mask, name):
    rng = np.random.default_rng(seed)
    mats = [_mfcc_like(rng, T).astype(np.float32) for T in Ts]
    keys = [f"{name}{i:03d}" for i in range(len(Ts))]
    masks = None
    if with_mask:
        masks = [_speech_silence(rng, T) > 7.5 for T in Ts]
        masks[0] = np.ones(Ts[0], bool)
    scp = _archive(tmp_path, [(k, m, "FM") for k, m in zip(keys, mats)], name=name)
    return kf.load_feature_scp(scp), keys, mats, masks


@pytest.mark.parametrize("W", [300, 7])
@pytest.mark.parametrize("batch", ["edges", "ragged256"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["all-frames", "masked"])
def test_cmn_select_in_fp32_units(tmp_path, W, batch, with_mask):
    # gates 3 / 5 (rms / max) of tests/fp32_units; measured on MI355X: rms 0.42 - 0.43, max 0.50 - 0.56 over the sixteen
    # cases (W = 300 edges 0.427 / 0.546, masked 0.427 / 0.559; every W = 7 and ragged case 0.42 / 0.50).  Below 1: the
    # device subtracts in fp64 and rounds once, the unit is an fp32 subtraction of a rounded mean.
    Ts = EDGE_T if batch == "edges" else [int(t) for t in np.random.default_rng(256).integers(1, 700, 256)]
    feats, keys, mats, masks = _cmn_case(tmp_path, Ts, 80 + W + len(Ts), with_mask, batch)
    vad = None if masks is None else {k: m.astype(np.float32) for k, m in zip(keys, masks)}
    prep = features.prepare_features(feats, vad=vad, cmn_window=W, min_frames=1, device=DEV)
    r64, r32, lengths, counts = feat_ref.prepare(mats, masks, W, 1)
    assert prep.lengths == lengths                                        # per-utterance counts, exact
    assert prep.keys == [k for k, c in zip(keys, counts) if c >= 1]
    assert prep.dropped == [(k, c) for k, c in zip(keys, counts) if c < 1]
    got = prep.frames.cpu().numpy()
    assert got.shape == r64.shape
    off = np.concatenate([[0], np.cumsum(lengths)])
    for u in range(len(lengths)):                                         # row order: every utterance on its own
        a = got[off[u]:off[u + 1]]
        assert np.abs(a - r64[off[u]:off[u + 1]]).max() <= 1e-4, (prep.keys[u], lengths[u])
    r = fp32_units.assert_fp32_level(got, r64, r32, f"cmn W={W} {batch} mask={with_mask}")
    print(f"cmn W={W} {batch} mask={with_mask}: rms / max ratio {r['all'][0]:.3f} / {r['all'][1]:.3f}")
    again = features.prepare_features(feats, vad=vad, cmn_window=W, min_frames=1, device=DEV)
    assert torch.equal(prep.frames, again.frames) and again.lengths == prep.lengths      # two calls, the same bits
    # an utterance's rows do not depend on the batch it is in
    one = kf.FeatureArchive(feats.keys[-1:], feats.desc[-1:], feats.payload)
    solo = features.prepare_features(one, vad=vad, cmn_window=W, min_frames=1, device=DEV)
    if solo.lengths:
        assert torch.equal(solo.frames, prep.frames[off[-2]:])


def test_cmn_window_zero_and_min_frames(tmp_path):
    feats, keys, mats, masks = _cmn_case(tmp_path, [40, 10, 24, 25, 0, 300], 5, True, "mf")
    masks[1][:] = True
    vad = {k: m.astype(np.float32) for k, m in zip(keys, masks)}
    prep = features.prepare_features(feats, vad=vad, cmn_window=0, min_frames=25, device=DEV)
    counts = [int(m.sum()) for m in masks]
    assert prep.dropped == [(k, c) for k, c in zip(keys, counts) if c < 25] and ("mf001", 10) in prep.dropped
    assert prep.lengths == [c for c in counts if c >= 25]
    want = np.concatenate([m[k] for m, k, c in zip(mats, masks, counts) if c >= 25])
    assert np.array_equal(prep.frames.cpu().numpy(), want)                # no normalisation: the selected rows themselves
    # given decisions from a vad.scp are the same as the dict (write_vector_ark writes rows of one length: a file each)
    nz = [i for i, m in enumerate(masks) if m.shape[0] > 0]
    sub = kf.FeatureArchive([keys[i] for i in nz], feats.desc[nz], feats.payload)
    vscp, lines = str(tmp_path / "vad.scp"), []
    for i in nz:
        p = str(tmp_path / f"vad{i}.ark")
        offs = kf.write_vector_ark(p, [keys[i]], masks[i][None, :].astype(np.float32))
        lines.append(f"{keys[i]} {p}:{offs[0]}\n")
    with open(vscp, "w") as fh:
        fh.write("".join(lines))
    a = features.prepare_features(sub, vad=vscp, cmn_window=300, min_frames=1, device=DEV)
    b = features.prepare_features(sub, vad={k: vad[k] for k in sub.keys}, cmn_window=300, min_frames=1, device=DEV)
    assert torch.equal(a.frames, b.frames) and a.lengths == b.lengths and a.keys == b.keys
    with pytest.raises(ValueError, match="mf000"):
        features.prepare_features(sub, vad={**vad, "mf000": np.ones(7)}, device=DEV)
    with pytest.raises(KeyError, match="mf003"):
        features.prepare_features(sub, vad={k: v for k, v in vad.items() if k != "mf003"}, device=DEV)


# ---- 9. composition with the extractor --------------------------------------------------------------------------------------

def _compose_items(seed):
    rng = np.random.default_rng(seed)
    fmts = ["CM", "CM", "CM2", "FM", "CM3", "DM"]
    items = []
    for i in range(40):
        T = int(rng.integers(120, 520))
        x = _mfcc_like(rng, T)
        x[:, 0] = _speech_silence(rng, T)
        items.append((f"spk{i % 7}-utt{i:02d}", x, fmts[i % 6]))
    x = _mfcc_like(rng, 200)
    x[:, 0] = rng.normal(2.0, 1.0, 200)
    x[97:103, 0] = rng.normal(20.0, 0.5, 6)    # six frames above the threshold: with +-2 frames of context, 10 voiced
    items[17] = ("short-utt17", x, "CM")
    return items


def _compose_reference(items, opts):
    """The restatement on the DECODED matrices; asserts that the decisions cannot depend on fp32-vs-fp64 decoding."""
    mats, masks = [], []
    for key, mat, fmt in items:
        dec, bound = feat_ref.decode(feat_ref.encode(mat, fmt))
        thr = feat_ref.vad_threshold(dec[:, 0].astype(np.float32), opts.energy_threshold, opts.energy_mean_scale)
        assert np.abs(dec[:, 0] - thr).min() > MARGIN + bound, key
        mats.append(dec)
        masks.append(feat_ref.vad_energy(dec[:, 0], *opts))
    return mats, masks


def test_compose_inputs_are_clear_of_the_threshold():
    _compose_reference(_compose_items(COMPOSE_SEED), features.VadOptions())


def test_extract_from_scp_equals_the_restatement_then_extract_ragged(tmp_path):
    params = xvec_ref.make_params()
    m = _extractor(params)
    items = _compose_items(COMPOSE_SEED)
    opts = features.VadOptions()
    order = [items[i][0] for i in np.random.default_rng(1).permutation(40)]
    scp = _archive(tmp_path, items, order)
    by_key = {k: (k, x, f) for k, x, f in items}
    ordered = [by_key[k] for k in order]
    mats, masks = _compose_reference(ordered, opts)
    r64, _, lengths, counts = feat_ref.prepare(mats, masks, 300, 25)
    want_keys = [k for k, c in zip(order, counts) if c >= 25]
    want_dropped = [(k, c) for k, c in zip(order, counts) if c < 25]
    assert ("short-utt17", 10) in want_dropped and ("spk5-utt12", 0) in want_dropped   # ten voiced frames; none at all
    outs = {}
    for n in (1, 7, 40):
        keys, xv, dropped = m.extract_from_scp(scp, vad=opts, utts_per_call=n)
        assert keys == want_keys and dropped == want_dropped
        assert "short-utt17" not in keys and xv.shape == (len(want_keys), 512) and xv.device == DEV
        outs[n] = xv
    assert torch.equal(outs[1], outs[7]) and torch.equal(outs[1], outs[40])       # piece boundaries do not matter
    # extract_ragged on the frames the restatement prepares, uploaded as float32
    rows32 = r64.astype(np.float32)
    direct = m.extract_ragged(torch.from_numpy(rows32).to(DEV), lengths).cpu().numpy()
    ref64 = xvec_ref.extract_ragged(rows32.astype(np.float64), lengths, params, "std", np.float64)
    ref32 = xvec_ref.extract_ragged(rows32, lengths, params, "std", np.float32)
    # gates 3 / 5; measured on MI355X: extract_from_scp 1.72 / 1.54, extract_ragged on the restated frames 1.74 / 1.54
    ra = fp32_units.assert_fp32_level(outs[40].cpu().numpy(), ref64, ref32, "extract_from_scp")
    rb = fp32_units.assert_fp32_level(direct, ref64, ref32, "extract_ragged on the restatement's frames")
    print(f"composition: extract_from_scp {ra['all']}, extract_ragged on restated frames {rb['all']}")
    # given decisions instead of the energy VAD: the same x-vectors
    keys2, xv2, dropped2 = m.extract_from_scp(scp, vad={k: mk.astype(np.float32) for k, mk in zip(order, masks)},
                                              utts_per_call=16)
    assert keys2 == want_keys and dropped2 == want_dropped and torch.equal(xv2, outs[40])
    # an empty scp
    empty = str(tmp_path / "empty.scp")
    open(empty, "w").close()
    k0, x0, d0 = m.extract_from_scp(empty)
    assert k0 == [] and d0 == [] and tuple(x0.shape) == (0, 512)
    with pytest.raises(ValueError, match="min_frames"):
        m.extract_from_scp(scp, min_frames=10)


# ---- 10. the extraction CLI -------------------------------------------------------------------------------------------------

def test_extract_xvectors_cli(tmp_path):
    params = xvec_ref.make_params()
    m = _extractor(params)
    items = _compose_items(COMPOSE_SEED)
    scp = _archive(tmp_path, items)
    model = str(tmp_path / "extractor.pt")
    torch.save({k: v.cpu() for k, v in m.state_dict().items()}, model)
    conf = str(tmp_path / "vad.conf")
    with open(conf, "w") as fh:
        fh.write("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n"
                 "--vad-frames-context=2\n")
    ark, oscp = str(tmp_path / "xvector.ark"), str(tmp_path / "xvector.scp")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_xvectors.py"), scp, "--vad-conf", conf,
                        "--model", model, "--out-ark", ark, "--out-scp", oscp, "--utts-per-call", "16"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "dropped short-utt17: 10 voiced frames" in r.stderr
    keys, xv, dropped = m.extract_from_scp(scp, vad=features.VadOptions.from_conf(conf))
    lk, lx = kf.load_vector_scp(oscp)
    assert lk == keys and lx.dtype == np.float32
    assert np.array_equal(lx, xv.cpu().numpy())                           # bit for bit
    assert ("short-utt17", 10) in dropped
