"""The resampler on the MI355X (csrc/nplda_resample.hip through neuralplda_amd/resample.py) against the twin
tests/resample_ref.py: float output against resample64 in units of resample32's error (tests/fp32_units, gates 3 rms / 5 max,
regions over samples at the kernel's chunk of 1024 outputs), 16-bit output against rint(resample64), the copy path bit for bit,
saturation, determinism (two calls, alone / in a batch / permuted, a captured graph) and the composition with the
augmentation, the MFCCs and the extractor.  The inputs are defined in tests/resample_ref.py; tests/test_resample_cpu.py checks
their conditions without a device."""
import functools

import numpy as np
import pytest
import torch

from neuralplda_amd import augment as ag, features, kaldi_format as kf, mfcc, resample as rs
from tests import augment_ref, fp32_units, resample_ref as ref, xvec_ref
from tests.test_mfcc_cpu import opts_16k

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SR = 16000


def _concat(parts):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int16)).astype(np.int16), offsets


def _split(t, offsets):
    a = t.cpu().numpy()
    return [a[offsets[u]:offsets[u + 1]] for u in range(len(offsets) - 1)]


def _check(got, r64, r32, what):
    reg = fp32_units.Regions(len(got), rs.CHUNK)
    r = fp32_units.assert_fp32_level(got[reg.idx], r64[reg.idx], r32[reg.idx], what, reg)
    print(f"{what}: " + ", ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in r.items()))
    return r


def _run(cases, out_dtype=torch.float32, gain=1.0):
    samples, offsets = _concat([x for x, _, _ in cases])
    out, ooff, clipped = rs.resample(samples, offsets, [r for _, r, _ in cases], [r for _, _, r in cases], gain, out_dtype,
                                     device=DEV)
    assert out.dtype == out_dtype and out.device == DEV and clipped.dtype == torch.int32 and clipped.shape == (len(cases),)
    assert np.diff(ooff).tolist() == [ref.output_length(len(x), a, b) for x, a, b in cases]
    return out, ooff, clipped


@functools.lru_cache(maxsize=None)
def _grid():
    cases = ref.grid_case()
    out, ooff, clipped = _run(cases)
    return cases, out, ooff, clipped


@functools.lru_cache(maxsize=None)
def _mixed():
    cases = ref.mixed_case()
    out, ooff, clipped = _run(cases)
    return cases, out, ooff, clipped


# ---- float output in fp32 units --------------------------------------------------------------------------------------------

def test_grid_in_fp32_units():
    """ONE call of 42 utterances: every ratio of 9:10, 11:10, 2:1, 1:2, 441:160, 441:80 with n in {1, 2, taps - 1, taps, one
    input sample less / more than a chunk of 1024 outputs takes, 5000}.  Per ratio, its outputs together against the twins,
    and the two chunk-edge lengths on their own.  Gates 3 / 5 (rms / max).  Measured on MI355X, per ratio over all its
    outputs (worst region or edge length in brackets):
      9:10     0.933 / 0.912  (0.957 / 1.274)        1:2      0.924 / 0.869  (0.975 / 1.141)
      11:10    0.945 / 1.069  (0.959 / 1.199)        441:160  0.965 / 0.787  (0.981 / 1.000)
      2:1      0.967 / 0.997  (0.988 / 1.000)        441:80   1.007 / 1.246  (1.030 / 1.286)"""
    cases, out, ooff, clipped = _grid()
    assert int(clipped.sum()) == 0
    got = _split(out, ooff)
    for rin, rout in ref.RATES:
        mine = [u for u, c in enumerate(cases) if (c[1], c[2]) == (rin, rout)]
        assert [len(cases[u][0]) for u in mine] == list(ref.grid_lengths(rin, rout))
        r64 = [ref.resample64(*cases[u]) for u in mine]
        r32 = [ref.resample32(*cases[u]) for u in mine]
        _check(np.concatenate([got[u] for u in mine]), np.concatenate(r64), np.concatenate(r32), f"{rin}->{rout}")
        for j in (4, 5):   # the lengths at the chunk's edge
            _check(got[mine[j]], r64[j], r32[j], f"{rin}->{rout} n={len(cases[mine[j]][0])}")


def test_mixed_ratios_copies_and_empty_utterances_in_fp32_units():
    """14 utterances, each of another ratio than its neighbour (nine ratios, 19:20 and 21:20 and 3:1 among them), three copies
    and three empty utterances in between: one call.  The copies are exact.  Measured on MI355X over the resampled
    utterances: 0.950 / 1.341 (worst region 0.964 / 1.341)."""
    cases, out, ooff, clipped = _mixed()
    assert sum(1 for x, a, b in cases if a == b) == 3 and sum(1 for x, _, _ in cases if len(x) == 0) == 3
    assert all((cases[u][1], cases[u][2]) != (cases[u + 1][1], cases[u + 1][2]) for u in range(len(cases) - 1))
    got = _split(out, ooff)
    filt = [u for u, (x, a, b) in enumerate(cases) if a != b and len(x)]
    for u, (x, a, b) in enumerate(cases):
        if a == b:
            assert np.array_equal(got[u], x.astype(np.float32)), u
    _check(np.concatenate([got[u] for u in filt]), np.concatenate([ref.resample64(*cases[u]) for u in filt]),
           np.concatenate([ref.resample32(*cases[u]) for u in filt]), "mixed ratios")
    assert int(clipped.sum()) == 0


# ---- 16-bit output ------------------------------------------------------------------------------------------------------------

def test_int16_output_against_the_float64_twin():
    """20 000 samples per ratio: within 1 of rint(resample64) everywhere, differing in at most 0.5 % of the samples of each
    case (a cap: tests/test_resample_cpu.py holds the float32 twin alone to half of it on the same inputs, where it has
    0.000 - 0.055 %).  Measured on MI355X, per case: 0.000 - 0.069 % (0 of 3 629 at 441:80 to 5 of 7 257 at 441:160)."""
    cases = ref.big_cases()
    out, ooff, clipped = _run(cases, torch.int16)
    assert int(clipped.sum()) == 0
    for (x, a, b), got in zip(cases, _split(out, ooff)):
        want, _ = ref.round_int16(ref.resample64(x, a, b))
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print(f"{a}->{b}: {int((d > 0).sum())} of {d.size} differ ({100 * (d > 0).mean():.4f} %), max {int(d.max())}")
        assert d.max() <= 1 and (d > 0).mean() <= 0.005, (a, b, int(d.max()), float((d > 0).mean()))


# ---- exact paths ------------------------------------------------------------------------------------------------------------------

def test_equal_rates_are_a_copy_times_the_gain():
    rng = np.random.default_rng(3)
    audio = [ref.make_audio(rng, n) for n in (1, 1023, 1024, 1025, 5000, 0, 7)]
    samples, offsets = _concat(audio)
    out, ooff, clipped = rs.resample(samples, offsets, 16000, 16000, device=DEV)
    assert out.dtype == torch.int16 and np.array_equal(out.cpu().numpy(), samples) and np.array_equal(ooff, offsets)
    assert int(clipped.sum()) == 0
    half, hoff, _ = rs.resample(samples, offsets, 8000, 8000, gain=0.5, device=DEV)
    assert np.array_equal(half.cpu().numpy(), np.rint(0.5 * samples.astype(np.float64)).astype(np.int16))
    assert np.array_equal(hoff, offsets)
    one, _, _ = rs.speed_perturb(samples, offsets, 1.0, SR, device=DEV)
    assert np.array_equal(one.cpu().numpy(), samples)


def test_saturation_and_the_clipped_count():
    """A full-scale square wave with gain 2: the copy saturates everywhere; a filtered utterance is within 1 of the rounded
    float64 twin, and its count is the twin's up to the samples whose value lies within one step of the bound (where float32
    rounding may decide the other way)."""
    sq = np.where((np.arange(6000) // 40) % 2 == 0, 32767, -32768).astype(np.int16)
    cases = [(sq, 16000, 16000), (sq, 14400, 16000), (sq[:3001], 16000, 8000), (sq[:100], 8000, 16000)]
    out, ooff, clipped = _run(cases, torch.int16, gain=2.0)
    got_c = clipped.cpu().numpy()
    assert int(got_c[0]) == 6000 and np.array_equal(_split(out, ooff)[0], np.where(sq > 0, 32767, -32768))
    for u, (x, a, b) in enumerate(cases):
        v = ref.resample64(x, a, b, gain=2.0)
        want, n = ref.round_int16(v)
        near = int((np.abs(np.abs(v) - 32767.5) < 1.0).sum())       # values a rounding step could move across the bound
        got = _split(out, ooff)[u]
        assert np.abs(got.astype(np.int64) - want).max() <= 1 and abs(int(got_c[u]) - n) <= near, (u, int(got_c[u]), n, near)
        assert int(got_c[u]) > 0.5 * len(got) and (got == 32767).any() and (got == -32768).any()


# ---- determinism ------------------------------------------------------------------------------------------------------------------

def test_same_bits_alone_in_a_batch_and_permuted():
    cases, out, ooff, _ = _mixed()
    again, _, _ = _run(cases)
    assert torch.equal(out, again)                                                  # two calls, the same bits
    got = _split(out, ooff)
    for u in (0, 3, 7, 9, 11):                                                      # alone
        x, a, b = cases[u]
        solo, _, _ = rs.resample(x, [0, len(x)], a, b, out_dtype=torch.float32, device=DEV)
        assert np.array_equal(solo.cpu().numpy(), got[u]), u
    perm = np.random.default_rng(1).permutation(len(cases))                         # permuted
    pout, poo, _ = _run([cases[u] for u in perm])
    for k, g in enumerate(_split(pout, poo)):
        assert np.array_equal(g, got[perm[k]]), k
    x, a, b = cases[7]                                                              # behind a prefix of 3 samples: another
    shifted, so, _ = rs.resample(np.concatenate([x[:3], x]), [0, 3, 3 + len(x)], a, b, out_dtype=torch.float32, device=DEV)
    assert np.array_equal(_split(shifted, so)[1], got[7])                           # alignment of the 16-byte loads
    samples, offsets = _concat([c[0] for c in cases])                               # a device tensor is taken as it is
    dev_in = torch.from_numpy(samples).to(DEV)
    assert torch.equal(rs.resample(dev_in, offsets, [c[1] for c in cases], [c[2] for c in cases], out_dtype=torch.float32)[0], out)


def test_captured_graph_replays_the_same_bits():
    cases = ref.mixed_case()
    samples, offsets = _concat([c[0] for c in cases])
    rin, rout = [c[1] for c in cases], [c[2] for c in cases]
    want, woff, wclip = rs.resample(samples, offsets, rin, rout, gain=3.0, device=DEV)
    assert int(wclip.sum()) > 0
    prep = rs.prepare(samples, offsets, rin, rout, gain=3.0, device=DEV)
    prep.launch()                                                                   # warm
    torch.cuda.synchronize()
    assert torch.equal(prep.samples, want) and torch.equal(prep.clipped, wclip)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        prep.launch()
    for _ in range(2):
        prep.samples.zero_()
        prep.clipped.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(prep.samples, want) and torch.equal(prep.clipped, wclip) and np.array_equal(prep.offsets, woff)


# ---- composition ------------------------------------------------------------------------------------------------------------------

def test_resample_then_mfcc():
    rng = np.random.default_rng(5)
    audio = [ref.make_audio(rng, n, 8000) for n in (8000, 5000)]
    samples, offsets = _concat(audio)
    s2, o2, _ = rs.resample(samples, offsets, 8000, SR, device=DEV)
    frames, lengths = mfcc.compute_mfcc(s2, o2, opts_16k(), DEV)
    want, wl = mfcc.compute_mfcc(s2.cpu().numpy(), o2, opts_16k(), DEV)
    assert torch.equal(frames, want) and list(lengths) == list(wl) and int(sum(lengths)) > 150
    assert torch.isfinite(frames).all()


def test_recipe_speed_equals_speed_perturb_then_augment():
    rng = np.random.default_rng(6)
    audio = [ref.make_audio(rng, n) for n in (3000, 1, 4500, 0, 2600)]
    samples, offsets = _concat(audio)
    rirs = ag.RirTable([augment_ref.make_rir(rng, L, p) for L, p in ((400, 20), (900, 100))], SR)
    noises = ag.NoiseTable([ref.make_audio(rng, n, dc=0.0) for n in (3000, 800)], SR)
    speed = [0.9, 1.1, 1.0, 0.9, 1.1]
    additive = [[(0, 100, 10.0, True)], [], [(1, 4000, 5.0, False)], [], []]
    rec = ag.Recipe([0, 1, -1, 0, 1], additive, speed=speed)
    out, ooff, clipped = ag.augment(samples, offsets, rec, rirs, noises, device=DEV)
    s1, o1, _ = rs.speed_perturb(samples, offsets, speed, SR, device=DEV)
    assert np.diff(o1).tolist() == [ref.output_length(len(x), round(f * SR), SR) for x, f in zip(audio, speed)]
    want, woff, wclip = ag.augment(s1, o1, ag.Recipe([0, 1, -1, 0, 1], additive), rirs, noises, device=DEV)
    assert torch.equal(out, want) and np.array_equal(ooff, woff) and torch.equal(clipped, wclip)
    assert np.array_equal(ag.output_lengths(np.diff(offsets), rec, rirs, SR), np.diff(woff))
    plain, _, _ = ag.augment(samples, offsets, ag.Recipe([0, 1, -1, 0, 1], additive), rirs, noises, device=DEV)
    assert plain.shape != out.shape


def test_extract_from_wav_scp_resamples_an_8_khz_file(tmp_path):
    from neuralplda_amd import models
    m = xvec_ref.load_into(models.XVectorNet_ETDNN_12Layer(), xvec_ref.make_params()).to(DEV).eval().requires_grad_(False)
    o, vad = opts_16k(), features.VadOptions()
    rng = np.random.default_rng(12)
    scp, scp16 = str(tmp_path / "wav.scp"), str(tmp_path / "wav16.scp")
    rates = (8000, SR, 8000, 44100)
    audio = [ref.make_audio(rng, int(secs * r), r) for secs, r in zip((1.0, 0.8, 1.2, 0.9), rates)]
    s16, o16, _ = rs.resample(*_concat(audio), list(rates), SR, device=DEV)
    with open(scp, "w") as fa, open(scp16, "w") as fb:
        for i, (x, r, y) in enumerate(zip(audio, rates, _split(s16, o16))):
            pa, pb = str(tmp_path / f"utt{i}.wav"), str(tmp_path / f"utt{i}_16k.wav")
            kf.write_wav(pa, x, r)
            kf.write_wav(pb, y, SR)
            fa.write(f"utt{i} {pa}\n")
            fb.write(f"utt{i} {pb}\n")
    with pytest.raises(kf.KaldiFormatError, match="no resampling"):
        m.extract_from_wav_scp(scp, mfcc=o, vad=vad)
    for per_call in (4, 3):
        keys, xv, dropped = m.extract_from_wav_scp(scp, mfcc=o, vad=vad, utts_per_call=per_call, resample=True)
        k16, x16, d16 = m.extract_from_wav_scp(scp16, mfcc=o, vad=vad, utts_per_call=per_call)
        assert keys == k16 and len(keys) == 4 and dropped == d16 == [] and torch.equal(xv, x16)


def test_tables_resample_their_items_at_construction(tmp_path):
    rng = np.random.default_rng(13)
    noise8 = ref.make_audio(rng, 4000, 8000, dc=0.0)
    rir8 = np.rint(3000 * np.abs(augment_ref.make_rir(rng, 300, 10))).astype(np.int16)
    pn, pr = str(tmp_path / "n.wav"), str(tmp_path / "r.wav")
    kf.write_wav(pn, noise8, 8000)
    kf.write_wav(pr, rir8, 8000)
    with pytest.raises(ValueError, match="sample rate 8000"):
        ag.NoiseTable([pn], SR)
    with pytest.raises(ValueError, match="sample rate 8000"):
        ag.RirTable([pr], SR)
    n16, no, _ = rs.resample(noise8, [0, 4000], 8000, SR, device=DEV)
    table = ag.NoiseTable([pn, noise8[:100]], SR, resample=True)
    want = ag.NoiseTable([n16.cpu().numpy(), noise8[:100]], SR)
    assert np.array_equal(table.samples, want.samples) and np.array_equal(table.offsets, want.offsets)
    r16, _, _ = rs.resample(rir8, [0, 300], 8000, SR, gain=0.5, out_dtype=torch.float32, device=DEV)
    rt = ag.RirTable([pr], SR, resample=True)
    assert rt.taps.dtype == np.float32 and np.array_equal(rt.taps, r16.cpu().numpy()) and len(rt.taps) == 600
    assert abs(float(rt.taps.sum()) / float(rir8.sum()) - 1.0) < 2e-3             # the DC gain is kept


def test_tool_writes_the_speed_copies_and_the_resampled_files(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("resample_wav_scp", os.path.join(root, "tools", "resample_wav_scp.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(14)
    audio = {"spkA-u1": (ref.make_audio(rng, 1500), SR), "spkB-u1": (ref.make_audio(rng, 900, 8000), 8000)}
    scp, u2s = str(tmp_path / "wav.scp"), str(tmp_path / "utt2spk")
    with open(scp, "w") as fa, open(u2s, "w") as fb:
        for k, (x, r) in audio.items():
            kf.write_wav(str(tmp_path / f"{k}.wav"), x, r)
            fa.write(f"{k} {tmp_path / (k + '.wav')}\n")
            fb.write(f"{k} {k[:4]}\n")
    out = str(tmp_path / "sp")
    assert tool.main([scp, out, "--speeds", "0.9,1.0,1.1", "--utt2spk", u2s, "--utts-per-call", "4"]) == 0
    keys, offsets, samples, rates = kf.load_wav_scp(os.path.join(out, "wav.scp"), return_rates=True)
    assert keys == [f"sp{f}-{k}" for f in ("0.9", "1.0", "1.1") for k in audio]
    for i, key in enumerate(keys):
        f, src = float(key[2:5]), key[6:]
        x, r = audio[src]
        want, _, _ = rs.speed_perturb(x, [0, len(x)], f, r, device=DEV)
        assert rates[i] == r and np.array_equal(samples[offsets[i]:offsets[i + 1]], want.cpu().numpy()), key
    assert open(os.path.join(out, "utt2spk")).read().splitlines()[1] == "sp0.9-spkB-u1 sp0.9-spkB"
    assert len(open(os.path.join(out, "spk2utt")).read().splitlines()) == 6
    out16 = str(tmp_path / "r16")
    assert tool.main([scp, out16, "--rate", "16000"]) == 0
    keys, offsets, samples, rates = kf.load_wav_scp(os.path.join(out16, "wav.scp"), sample_frequency=SR, return_rates=True)
    assert keys == list(audio) and np.array_equal(samples[offsets[0]:offsets[1]], audio["spkA-u1"][0])
    want, _, _ = rs.resample(audio["spkB-u1"][0], [0, 900], 8000, SR, device=DEV)
    assert np.array_equal(samples[offsets[1]:offsets[2]], want.cpu().numpy()) and not os.path.exists(os.path.join(out16, "utt2spk"))
