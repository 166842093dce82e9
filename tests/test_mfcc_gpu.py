"""The MFCC kernel on the MI355X (csrc/nplda_mfcc.hip through neuralplda_amd/mfcc.py) against the restatement
tests/mfcc_ref.py: `got` against mfcc64 in units of mfcc32's error (tests/fp32_units, gates 3 rms / 5 max), over the first
frame tile, the last full tile, the ragged last tile and the rest; batch independence, bounds, the unsupported geometries,
the composition with VAD, CMN and the extractor, and prepare_features after its split."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from neuralplda_amd import _lib, features, kaldi_format as kf, mfcc
from tests import feat_ref, fp32_units, mfcc_ref, xvec_ref
from tests.test_mfcc_cpu import opts_16k, opts_8k, test_inputs as make_audio

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TM = mfcc.FRAME_TILE
EPS = mfcc_ref.FLT_EPSILON
MARGIN = 1e-3
COMPOSE_SEED = 0     # a seed for which the composition's c0 stay clear of the VAD threshold (searched on the CPU)


def _samples_for(T, o):
    """A number of samples that gives exactly T frames."""
    n = o.frame_size + (T - 1) * o.shift if o.snip_edges else T * o.shift
    assert int(mfcc.num_frames(n, o)) == T
    return n


def _reference(samples, offsets, o, check_energies=True):
    r64, r32 = [], []
    for u in range(len(offsets) - 1):
        x = samples[offsets[u]:offsets[u + 1]]
        a, en = mfcc_ref.mfcc64(x, o, with_energies=True)
        if check_energies and en.size:   # a condition on the inputs: the floor is not in play, log amplifies no vanishing bin
            assert en.min() >= 1e6 * EPS, (u, float(en.min()))
        r64.append(a)
        r32.append(mfcc_ref.mfcc32(x, o))
    return np.concatenate(r64), np.concatenate(r32)


def _check(got, r64, r32, what):
    reg = fp32_units.Regions(got.shape[0], TM)
    r = fp32_units.assert_fp32_level(got[reg.idx], r64[reg.idx], r32[reg.idx], what, reg)
    print(f"{what}: " + ", ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in r.items()))
    return r


def _concat(parts):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts) if parts else np.zeros(0, np.int16), offsets


RAGGED_SAMPLES = [0, 1, 79, 80, 399, 400, 401, 560]


@functools.lru_cache(maxsize=None)
def _ragged(rate, seed=40):
    """40 utterances: the edge lengths, then up to 2 s; several share a tile, several yield no frame."""
    rng = np.random.default_rng(seed)
    ns = RAGGED_SAMPLES + [int(n) for n in rng.integers(int(rate), 2 * int(rate) + 1, 26)] + \
        [int(n) for n in rng.integers(40, int(rate), 4)] + [2 * int(rate), 39]
    assert len(ns) == 40
    order = rng.permutation(40)
    return _concat([make_audio(rng, ns[i], rate=rate) for i in order])


CONFIGS = {"8k": opts_8k, "16k": opts_16k}


# ---- accuracy -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("snip", [False, True], ids=["reflect", "snip"])
@pytest.mark.parametrize("cfg", ["8k", "16k"])
def test_single_utterances_in_fp32_units(cfg, snip):
    # gates 3 / 5 (rms / max); measured on MI355X: 8 kHz 0.39 - 0.47 / 0.38 - 0.79, 16 kHz 0.58 - 0.69 / 0.52 - 0.79
    # (every case: design/k14_mfcc.md)
    o = CONFIGS[cfg](snip_edges=snip)
    rng = np.random.default_rng(7)
    for T in (TM - 1, TM, TM + 1, 3 * TM + 5):
        x = make_audio(rng, _samples_for(T, o), rate=o.sample_frequency)
        frames, lengths = mfcc.compute_mfcc(x, [0, len(x)], o, DEV)
        assert lengths == [T] and frames.shape == (T, o.num_ceps) and frames.dtype == torch.float32 and frames.device == DEV
        r64, r32 = _reference(x, [0, len(x)], o)
        _check(frames.cpu().numpy(), r64, r32, f"{cfg} snip={snip} T={T}")


@pytest.mark.parametrize("snip", [False, True], ids=["reflect", "snip"])
@pytest.mark.parametrize("cfg", ["8k", "16k"])
def test_ragged_batch_in_fp32_units_and_alone(cfg, snip):
    o = CONFIGS[cfg](snip_edges=snip)
    samples, offsets = _ragged(o.sample_frequency)
    frames, lengths = mfcc.compute_mfcc(samples, offsets, o, DEV)
    want = [int(t) for t in mfcc.num_frames(np.diff(offsets), o)]
    assert lengths == want and frames.shape == (sum(want), o.num_ceps)
    assert sum(1 for t in want if t == 0) >= 3 and sum(1 for t in want if 0 < t < TM // 2) >= 3 and 4000 <= sum(want) <= 6000
    got = frames.cpu().numpy()
    r64, r32 = _reference(samples, offsets, o)
    _check(got, r64, r32, f"{cfg} snip={snip} ragged")
    again, _ = mfcc.compute_mfcc(samples, offsets, o, DEV)
    assert torch.equal(frames, again)                                        # two calls, the same bits
    # an utterance's rows are the same bits alone and inside the batch
    foff = np.concatenate([[0], np.cumsum(want)])
    for u in (0, 7, 19, 38, 39):
        solo, sl = mfcc.compute_mfcc(samples[offsets[u]:offsets[u + 1]], [0, offsets[u + 1] - offsets[u]], o, DEV)
        assert sl == [want[u]] and torch.equal(solo, frames[foff[u]:foff[u + 1]]), u
    # a device tensor is taken as it is
    dsamp = torch.from_numpy(samples).to(DEV)
    assert torch.equal(mfcc.compute_mfcc(dsamp, offsets, o)[0], frames)


OPTION_CASES = {"raw_energy=false": dict(raw_energy=False), "use_energy=false": dict(use_energy=False),
                "remove_dc_offset=false": dict(remove_dc_offset=False), "cepstral_lifter=0": dict(cepstral_lifter=0.0),
                "hamming": dict(window_type="hamming"), "energy_floor": dict(energy_floor=1e3)}


@pytest.mark.parametrize("case", list(OPTION_CASES))
def test_options_in_fp32_units(case):
    o = opts_16k(**OPTION_CASES[case])
    rng = np.random.default_rng(11)
    if case == "energy_floor":   # quiet audio: the log energy of about half of the frames lies below log(1e3)
        n = 3 * 16000 // 2
        gain = np.where((np.arange(n) // 1600) % 2 == 0, 0.9, 3.0)
        x = np.clip(np.rint(rng.standard_normal(n) * gain + 2.0), -32768, 32767).astype(np.int16)
    else:
        x = make_audio(rng, _samples_for(2 * TM + 9, o))
    frames, lengths = mfcc.compute_mfcc(x, [0, len(x)], o, DEV)
    got = frames.cpu().numpy()
    r64, r32 = _reference(x, [0, len(x)], o, check_energies=case != "energy_floor")
    if case == "energy_floor":
        at = r64[:, 0] == np.log(1e3)
        assert 0.2 < at.mean() < 0.8 and np.array_equal(got[at, 0], r32[at, 0])
    _check(got, r64, r32, case)


@pytest.mark.parametrize("cfg", ["8k", "16k"])
def test_floors(cfg):
    """Digital silence and constant audio: both logarithms sit on their FLT_EPSILON floor."""
    o = CONFIGS[cfg]()
    n = _samples_for(TM + 3, o)
    for x in (np.zeros(n, np.int16), np.full(n, 1234, np.int16)):
        frames, _ = mfcc.compute_mfcc(x, [0, n], o, DEV)
        got = frames.cpu().numpy()
        r64, r32 = _reference(x, [0, n], o, check_energies=False)
        assert np.abs(r64 - mfcc_ref.floor_output(o)[None, :]).max() <= 1e-9
        assert np.abs(got[:, 0].astype(np.float64) - np.log(EPS)).max() <= 4e-6      # logf to 2 ulp at 16
        _check(got, r64, r32, f"{cfg} floor {int(x[0])}")


# ---- bounds and unsupported geometries --------------------------------------------------------------------------------------

def test_nothing_outside_the_utterances_is_read():
    """The samples in the middle of a larger allocation filled with 32767: a reflected index that left its utterance (or
    the buffer) would change the result."""
    o = opts_16k()
    samples, offsets = _ragged(o.sample_frequency)
    want, _ = mfcc.compute_mfcc(samples, offsets, o, DEV)
    pad = 4096
    big = torch.full((len(samples) + 2 * pad,), 32767, dtype=torch.int16, device=DEV)
    big[pad:pad + len(samples)] = torch.from_numpy(samples).to(DEV)
    got, _ = mfcc.compute_mfcc(big[pad:pad + len(samples)], offsets, o)
    assert torch.equal(got, want)
    # every utterance on its own, surrounded by the others' samples replaced by 32767
    for u in (3, 20):
        alone = torch.full_like(big, 32767)
        a, b = int(offsets[u]), int(offsets[u + 1])
        alone[pad + a:pad + b] = big[pad + a:pad + b]
        g, lengths = mfcc.compute_mfcc(alone[pad + a:pad + b], [0, b - a], o)
        foff = np.concatenate([[0], np.cumsum(mfcc.num_frames(np.diff(offsets), o))])
        assert torch.equal(g, want[foff[u]:foff[u + 1]])


def test_unsupported_geometry_launches_nothing():
    lib = _lib.load()
    o = mfcc.MfccOptions(sample_frequency=44100)                             # N = 1102
    g = mfcc.geometry_of(o)
    assert g.N == 1102
    plan = mfcc.MfccPlan.get(opts_16k(), DEV)
    x = torch.from_numpy(make_audio(np.random.default_rng(0), 44100, rate=44100.0)).to(DEV)
    soff = torch.tensor([0, 44100], dtype=torch.int64, device=DEV)
    R = int(mfcc.num_frames(44100, o))
    foff = torch.tensor([0, R], dtype=torch.int64, device=DEV)
    guard = 1024
    buf = torch.full((R * o.num_ceps + 2 * guard,), -7.25, dtype=torch.float32, device=DEV)
    out = buf[guard:guard + R * o.num_ceps]
    rc = lib.nplda_mfcc_frames_f32(x.data_ptr(), soff.data_ptr(), foff.data_ptr(), 1, R, ctypes.addressof(g),
                                   plan.window.data_ptr(), plan.dft.data_ptr(), plan.bank.data_ptr(), plan.dct.data_ptr(),
                                   out.data_ptr(), _lib.current_stream(DEV))
    assert rc == _lib.NPLDA_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == -7.25).all())                                        # sentinels and out untouched
    with pytest.raises(ValueError, match="1102"):
        mfcc.compute_mfcc(x, [0, 44100], o)
    with pytest.raises(ValueError, match="int16"):
        mfcc.compute_mfcc(np.zeros(1000, np.float32), [0, 1000], opts_16k(), DEV)
    with pytest.raises(ValueError, match="offsets"):
        mfcc.compute_mfcc(np.zeros(1000, np.int16), [0, 1001], opts_16k(), DEV)
    # nothing to do
    f0, l0 = mfcc.compute_mfcc(np.zeros(0, np.int16), [0], opts_16k(), DEV)
    f1, l1 = mfcc.compute_mfcc(np.zeros(100, np.int16), [0, 39, 39, 100], opts_16k(), DEV)
    assert tuple(f0.shape) == (0, 30) and l0 == [] and tuple(f1.shape) == (0, 30) and l1 == [0, 0, 0]


# ---- composition with VAD, CMN and the extractor ------------------------------------------------------------------------------

def _speech_like(rng, n):
    """Loud and quiet stretches of 0.1 - 0.6 s in turn (noise of standard deviation 3000 / 30 on an offset of 2000)."""
    x = np.empty(n)
    t, loud = 0, bool(rng.integers(2))
    while t < n:
        m = min(int(rng.integers(1600, 9600)), n - t)
        x[t:t + m] = rng.standard_normal(m) * (3000.0 if loud else 30.0)
        t, loud = t + m, not loud
    tt = np.arange(n) / 16000.0
    x += 2000.0 + 0.05 * np.abs(x) * np.sin(2 * np.pi * 440.0 * tt)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _compose_audio(seed):
    rng = np.random.default_rng(seed)
    secs = [0.2, 3.0, 0.9, 1.4, 2.2, 0.6, 1.1, 2.7, 0.75, 1.9, 1.25, 0.5]
    return [(f"spk{i % 4}-wav{i:02d}", _speech_like(rng, int(s * 16000))) for i, s in enumerate(secs)]


def _compose_reference(items, o, vad):
    mats, masks = [], []
    for key, x in items:
        m = mfcc_ref.mfcc64(x, o)
        thr = feat_ref.vad_threshold(m[:, 0].astype(np.float32), vad.energy_threshold, vad.energy_mean_scale)
        assert np.abs(m[:, 0] - thr).min() > MARGIN, key                    # no c0 within 1e-3 of its VAD threshold
        mats.append(m)
        masks.append(feat_ref.vad_energy(m[:, 0], *vad))
    return mats, masks


def test_extract_from_wav_scp_equals_the_restatement(tmp_path):
    from neuralplda_amd import models
    params = xvec_ref.make_params()
    m = xvec_ref.load_into(models.XVectorNet_ETDNN_12Layer(), params).to(DEV).eval().requires_grad_(False)
    o, vad = opts_16k(), features.VadOptions()
    items = _compose_audio(COMPOSE_SEED)
    scp = str(tmp_path / "wav.scp")
    with open(scp, "w") as fh:
        for key, x in items:
            p = str(tmp_path / f"{key}.wav")
            mfcc_ref.write_wav(p, x, 16000)
            fh.write(f"{key} {p}\n")
    mats, masks = _compose_reference(items, o, vad)
    r64, _, lengths, counts = feat_ref.prepare(mats, masks, 300, 25)
    keys_in = [k for k, _ in items]
    want_keys = [k for k, c in zip(keys_in, counts) if c >= 25]
    want_dropped = [(k, c) for k, c in zip(keys_in, counts) if c < 25]
    assert want_dropped and want_dropped[0][0] == "spk0-wav00" and len(want_keys) >= 9
    outs = {}
    for n in (1, 5, 12):
        keys, xv, dropped = m.extract_from_wav_scp(scp, mfcc=o, vad=vad, utts_per_call=n)
        assert keys == want_keys and dropped == want_dropped and xv.shape == (len(want_keys), 512) and xv.device == DEV
        outs[n] = xv
    assert torch.equal(outs[1], outs[5]) and torch.equal(outs[1], outs[12])    # piece boundaries do not matter
    rows32 = r64.astype(np.float32)
    ref64 = xvec_ref.extract_ragged(rows32.astype(np.float64), lengths, params, "std", np.float64)
    ref32 = xvec_ref.extract_ragged(rows32, lengths, params, "std", np.float32)
    # gates 3 / 5 of tests/test_features_gpu.py's composition case; measured on MI355X: 2.47 / 3.71, of which the MFCCs
    # through a float64 extractor account for 0.97 / 1.80 (design/k14_mfcc.md)
    r = fp32_units.measure(outs[12].cpu().numpy(), ref64, ref32)
    print(f"composition: extract_from_wav_scp {r['all']}")
    fp32_units.assert_fp32_level(outs[12].cpu().numpy(), ref64, ref32, "extract_from_wav_scp")
    with pytest.raises(ValueError, match="num_ceps"):
        m.extract_from_wav_scp(scp, mfcc=mfcc.MfccOptions())
    empty = str(tmp_path / "empty.scp")
    open(empty, "w").close()
    k0, x0, d0 = m.extract_from_wav_scp(empty, mfcc=o)
    assert k0 == [] and d0 == [] and tuple(x0.shape) == (0, 512)


def test_compose_inputs_are_clear_of_the_threshold():
    _compose_reference(_compose_audio(COMPOSE_SEED), opts_16k(), features.VadOptions())


def test_prepare_features_is_its_three_steps(tmp_path):
    """prepare_features after the prepare_frames split, on the feature tests' composition fixture: the same bits as
    decode_features + energy_vad + cmn_select."""
    from tests.test_features_gpu import _archive, _compose_items
    items = _compose_items(0)
    feats = kf.load_feature_scp(_archive(tmp_path, items))
    vad = features.VadOptions()
    prep = features.prepare_features(feats, vad=vad, cmn_window=300, min_frames=25, device=DEV)
    frames, lengths = features.decode_features(feats, DEV)
    mask = features.energy_vad(frames, lengths, vad)
    rows, cnt = features.cmn_select(frames, lengths, mask, 300, 25)
    keep = cnt >= 25
    assert torch.equal(prep.frames, rows) and prep.lengths == [int(c) for c in cnt[keep]]
    assert prep.keys == [k for (k, _, _), f in zip(items, keep) if f]
    assert prep.dropped == [(k, int(c)) for (k, _, _), c, f in zip(items, cnt, keep) if not f] and prep.dropped
    again = features.prepare_frames(feats.keys, frames, lengths, vad, 300, 25)
    assert torch.equal(again.frames, prep.frames) and again[1:] == prep[1:]
