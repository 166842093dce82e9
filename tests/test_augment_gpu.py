"""The augmentation on the MI355X (csrc/nplda_augment.hip through neuralplda_amd/augment.py) against the twin
tests/augment_ref.py: float output against augment64 in units of augment32's error (tests/fp32_units, gates 3 rms / 5 max,
regions over samples at tile 256), 16-bit output against round(augment64), the path without a RIR bit for bit, saturation,
determinism (two calls, alone / in a batch / permuted / split, a captured graph) and the composition with the MFCCs and the
extractor.  The inputs are defined in tests/test_augment_cpu.py, which checks their conditions without a device."""
import functools

import numpy as np
import pytest
import torch

from neuralplda_amd import augment as ag, features, kaldi_format as kf, mfcc
from tests import augment_ref as ref, fp32_units, xvec_ref
from tests.test_augment_cpu import FLAGS, GRID_L, GRID_N, SR, big_cases, grid_case, make_audio, mixed_case, ragged_case
from tests.test_mfcc_cpu import opts_16k

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _concat(parts):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int16)).astype(np.int16), offsets


def _split(t, offsets):
    a = t.cpu().numpy()
    return [a[offsets[u]:offsets[u + 1]] for u in range(len(offsets) - 1)]


def _check(got, r64, r32, what):
    reg = fp32_units.Regions(len(got), ag.BLOCK)
    r = fp32_units.assert_fp32_level(got[reg.idx], r64[reg.idx], r32[reg.idx], what, reg)
    print(f"{what}: " + ", ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in r.items()))
    return r


# ---- float output in fp32 units --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", GRID_L)
def test_grid_in_fp32_units(L):
    """n in {1, 255, 256, 257, 513, 5000} x this L, the peak at 0, in the middle and at L - 1, shift_output and
    normalize_output on and off: one call; per n, the outputs of its variants together against the twins.
    Gates 3 / 5 (rms / max); measured on MI355X, whole output of an (n, L), range over n (worst region in brackets):
      L = 1      0 (n = 1: exact), 0.85 - 1.08 / 0.58 - 1.50   (1.17 / 1.67)
      L = 2      0.84 - 1.07 / 0.79 - 1.43                      (1.12 / 1.51)
      L = 255    0.83 - 0.96 / 0.74 - 1.15                      (1.16 / 1.76)
      L = 256    0.76 - 0.98 / 0.60 - 1.33                      (1.07 / 1.41)
      L = 257    0.87 - 1.02 / 0.83 - 1.07                      (1.03 / 1.24)
      L = 1000   0.78 - 0.90 / 0.70 - 1.27                      (1.10 / 1.38)"""
    rirs, audio, cases = grid_case(L)
    samples, offsets = _concat([audio[a] for a, _, _, _ in cases])
    rec = ag.Recipe([r for _, r, _, _ in cases], shift_output=[s for _, _, s, _ in cases],
                    normalize_output=[m for _, _, _, m in cases])
    out, ooff, clipped = ag.augment(samples, offsets, rec, ag.RirTable(rirs, SR), out_dtype=torch.float32, device=DEV)
    assert out.dtype == torch.float32 and out.device == DEV and int(clipped.sum()) == 0
    want_len = [ref.output_length(len(audio[a]), L, s) for a, _, s, _ in cases]
    assert np.diff(ooff).tolist() == want_len
    got = _split(out, ooff)
    for a, n in enumerate(GRID_N):
        mine = [u for u, c in enumerate(cases) if c[0] == a]
        r64 = [ref.augment64(audio[a], rirs[cases[u][1]], shift_output=cases[u][2], normalize_output=cases[u][3]) for u in mine]
        r32 = [ref.augment32(audio[a], rirs[cases[u][1]], shift_output=cases[u][2], normalize_output=cases[u][3]) for u in mine]
        _check(np.concatenate([got[u] for u in mine]), np.concatenate(r64), np.concatenate(r32), f"n={n} L={L}")


@functools.lru_cache(maxsize=None)
def _ragged():
    rirs, audio, rir_of, shift = ragged_case()
    samples, offsets = _concat(audio)
    rec = ag.Recipe(rir_of, shift_output=shift)
    table = ag.RirTable(rirs, SR)
    out, ooff, _ = ag.augment(samples, offsets, rec, table, out_dtype=torch.float32, device=DEV)
    return samples, offsets, rec, table, out, ooff


def test_ragged_batch_in_fp32_units():
    """24 utterances of 0 - 6 000 samples over 5 impulse responses, a third without one: blocks of several utterances
    share the transform kernels' tiles.  Measured on MI355X: 0.92 / 1.05 (worst region 1.01 / 1.23)."""
    rirs, audio, rir_of, shift = ragged_case()
    samples, offsets, rec, table, out, ooff = _ragged()
    assert sorted(len(a) for a in audio)[0] == 0 and sum(1 for r in rir_of if r < 0) == 8
    blocks = ag._layout(np.diff(offsets), rec, table)["blocks"]
    assert (blocks[blocks > 0] % ag.TILE != 0).any() and blocks.sum() > 4 * ag.TILE
    got = _split(out, ooff)
    r64 = [ref.augment64(x, rirs[r] if r >= 0 else None, shift_output=s) for x, r, s in zip(audio, rir_of, shift)]
    r32 = [ref.augment32(x, rirs[r] if r >= 0 else None, shift_output=s) for x, r, s in zip(audio, rir_of, shift)]
    assert [len(g) for g in got] == [len(r) for r in r64]
    with_rir = [u for u, r in enumerate(rir_of) if r >= 0]
    _check(np.concatenate([got[u] for u in with_rir]), np.concatenate([r64[u] for u in with_rir]),
           np.concatenate([r32[u] for u in with_rir]), "ragged batch, reverberated")
    _check(np.concatenate(got), np.concatenate(r64), np.concatenate(r32), "ragged batch")


def test_rir_and_additive_entries_in_fp32_units():
    """A RIR and additive entries on the same utterance: the one place where the early window's power — the second
    multiply-accumulate, the synthesis to sums of squares, P_sig — reaches the output, as the entries' scale; with
    normalize_output on, P_mix is that of a mix with noise in it.  Early windows clamped at 0, at L, at both, at neither.  Every
    utterance on its own against the twins, gates 3 / 5.  Measured on MI355X: 0.78 - 1.01 / 0.75 - 1.06 over the eight
    utterances (worst region 1.11 / 1.49)."""
    rirs, noises, audio, recipe = mixed_case()
    samples, offsets = _concat(audio)
    rec = ag.Recipe([r for r, _, _, _ in recipe], [e for _, e, _, _ in recipe], [s for _, _, s, _ in recipe],
                    [m for _, _, _, m in recipe])
    out, ooff, _ = ag.augment(samples, offsets, rec, ag.RirTable(rirs, SR), ag.NoiseTable(noises, SR), out_dtype=torch.float32,
                              device=DEV)
    for u, (x, (r, additive, shift, norm), got) in enumerate(zip(audio, recipe, _split(out, ooff))):
        kw = dict(shift_output=shift, normalize_output=norm)
        r64, r32 = ref.augment64(x, rirs[r], additive, noises, **kw), ref.augment32(x, rirs[r], additive, noises, **kw)
        assert got.shape == r64.shape
        _check(got, r64, r32, f"mixed {u}: n={len(x)} L={len(rirs[r])} entries={len(additive)} shift={shift} normalize={norm}")
        bare = ref.augment64(x, rirs[r], (), noises, **kw)                        # the entries are a large part of the output
        assert np.sqrt(((r64 - bare) ** 2).mean()) > 0.05 * np.sqrt((r64 ** 2).mean()), u


# ---- 16-bit output ------------------------------------------------------------------------------------------------------------

def test_int16_output_against_the_float64_twin():
    """The inputs of at least 4 000 samples, default recipe: within 1 of round(augment64) everywhere, differing in at most
    0.5 % of the samples — twice the share tests/test_augment_cpu.py::test_condition_of_the_16_bit_cap allows augment32 on
    the same pooled samples.  Measured on MI355X: 174 of 100 766 (0.173 %)."""
    cases = big_cases()
    hs = []
    for _, h in cases:
        if not any(h is k for k in hs):
            hs.append(h)
    samples, offsets = _concat([x for x, _ in cases])
    rec = ag.Recipe([next(i for i, k in enumerate(hs) if k is h) for _, h in cases])
    out, ooff, clipped = ag.augment(samples, offsets, rec, ag.RirTable(hs, SR), device=DEV)
    assert out.dtype == torch.int16 and np.array_equal(ooff, offsets) and int(clipped.sum()) == 0
    total = differ = 0
    for (x, h), got in zip(cases, _split(out, ooff)):
        want, _ = ref.round_int16(ref.augment64(x, h))
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        # each case within 1 and, so that none hides in the pool, under twice the CPU test's per-case ceiling of 0.6 %
        assert d.max() <= 1 and (d > 0).mean() <= 0.012, (len(x), len(h), int(d.max()), float((d > 0).mean()))
        total, differ = total + d.size, differ + int((d > 0).sum())
    print(f"16-bit samples differing from round(augment64): {differ} of {total} ({100 * differ / total:.3f} %)")
    assert differ <= 0.005 * total


def test_identity():
    rng = np.random.default_rng(3)
    audio = [make_audio(rng, n) for n in (1, 256, 1000, 5000)]
    samples, offsets = _concat(audio)
    rec = ag.Recipe([0, 0, 0, 0], normalize_output=False)
    out, ooff, clipped = ag.augment(samples, offsets, rec, ag.RirTable([np.ones(1, np.float32)], SR), device=DEV)
    assert np.array_equal(out.cpu().numpy(), samples) and np.array_equal(ooff, offsets) and int(clipped.sum()) == 0
    clean, coff, _ = ag.augment(samples, offsets, ag.Recipe.clean(4), device=DEV)
    assert np.array_equal(clean.cpu().numpy(), samples) and np.array_equal(coff, offsets)


# ---- the path without a RIR: bit for bit ----------------------------------------------------------------------------------------

def _exact_case():
    rng = np.random.default_rng(9)
    noises = [make_audio(rng, 700, dc=0.0), make_audio(rng, 3000, dc=50.0), np.zeros(400, np.int16), make_audio(rng, 1, dc=900.0),
              make_audio(rng, 5000, dc=0.0)]
    audio = [make_audio(rng, n) for n in (2500, 2500, 4097, 2048, 300, 1, 2500)]
    additive = [[(0, 100, 10.0, True)],                                             # repeat: wraps around three times
                [(1, 1000, 5.0, False)],                                            # truncated by the end
                [(0, 4097, 0.0, True), (1, 5000, 0.0, False)],                      # starting at and past the end: no-ops
                [(2, 0, 10.0, True)],                                               # a silent item: a no-op
                [(0, 0, 15.0, True), (1, 17, 20.0, False), (3, 5, 13.0, True)],     # three entries, one of a single sample
                [(4, 0, 0.0, False)],
                [(4, 2047, 8.0, False), (0, 2049, 17.0, True)]]
    return audio, noises, additive


@pytest.mark.parametrize("gain", ["volume", "none"])
def test_exact_path_bit_for_bit(gain):
    audio, noises, additive = _exact_case()
    samples, offsets = _concat(audio)
    kw = dict(volume=0.5) if gain == "volume" else dict(normalize_output=False)
    rec = ag.Recipe([-1] * len(audio), additive, **kw)
    out, ooff, _ = ag.augment(samples, offsets, rec, None, ag.NoiseTable(noises, SR), out_dtype=torch.float32, device=DEV)
    assert np.array_equal(ooff, offsets)
    changed = 0
    for u, (x, got) in enumerate(zip(audio, _split(out, ooff))):
        want = ref.augment32(x, None, additive[u], noises, **kw)
        assert want.dtype == np.float32 and np.array_equal(got, want), (u, int((got != want).sum()))
        changed += int((want != ref.augment32(x, None, **kw)).sum())
    assert changed > 4000       # the entries did add something: 2 400 + 1 500 + 300 samples of utterances 0, 1 and 4 alone


def test_saturation():
    audio, noises, additive = _exact_case()
    samples, offsets = _concat(audio)
    rec = ag.Recipe([-1] * len(audio), additive, volume=6.0)
    out, ooff, clipped = ag.augment(samples, offsets, rec, None, ag.NoiseTable(noises, SR), device=DEV)
    assert out.dtype == torch.int16 and clipped.dtype == torch.int32 and clipped.device == DEV
    got_c = clipped.cpu().numpy()
    for u, (x, got) in enumerate(zip(audio, _split(out, ooff))):
        want, n = ref.round_int16(ref.augment32(x, None, additive[u], noises, volume=6.0))
        assert np.array_equal(got, want) and int(got_c[u]) == n, (u, int(got_c[u]), n)
    o = out.cpu().numpy()
    assert got_c.sum() > 1000 and (o == 32767).sum() > 100 and (o == -32768).sum() > 100


# ---- determinism ------------------------------------------------------------------------------------------------------------------

def test_same_bits_alone_in_a_batch_permuted_and_split():
    samples, offsets, rec, table, out, ooff = _ragged()
    again, _, _ = ag.augment(samples, offsets, rec, table, out_dtype=torch.float32, device=DEV)
    assert torch.equal(out, again)                                                  # two calls, the same bits
    got = _split(out, ooff)
    for u in (0, 4, 10, 17, 23):                                                    # alone
        x = samples[offsets[u]:offsets[u + 1]]
        solo, _, _ = ag.augment(x, [0, len(x)], rec.select([u]), table, out_dtype=torch.float32, device=DEV)
        assert np.array_equal(solo.cpu().numpy(), got[u]), u
    perm = np.random.default_rng(1).permutation(len(rec))                           # permuted
    ps, po = _concat([samples[offsets[u]:offsets[u + 1]] for u in perm])
    pout, poo, _ = ag.augment(ps, po, rec.select(perm), table, out_dtype=torch.float32, device=DEV)
    for k, g in enumerate(_split(pout, poo)):
        assert np.array_equal(g, got[perm[k]]), k
    lengths = np.diff(offsets)                                                      # split by a workspace limit
    limit = ag.workspace_bytes(lengths, rec, table) // 5
    assert len(ag._pieces(lengths, rec, table, limit)) >= 4
    prep = ag.prepare(samples, offsets, rec, table, out_dtype=torch.float32, device=DEV, workspace_limit=limit)
    assert len(prep.calls) >= 4 and prep.workspace_bytes == max(c.ws_bytes for c in prep.calls) <= limit
    assert prep.workspace.numel() == prep.workspace_bytes and all(c.ws is prep.workspace for c in prep.calls)  # one, shared
    sout, soo, _ = prep.launch()
    assert torch.equal(sout, out) and np.array_equal(soo, ooff)
    dev_in = torch.from_numpy(samples).to(DEV)                                      # a device tensor is taken as it is
    assert torch.equal(ag.augment(dev_in, offsets, rec, table, out_dtype=torch.float32)[0], out)


def test_captured_graph_replays_the_same_bits():
    """One capture of the whole call (transforms, multiply-accumulate, scalars, mix, store: the launch count depends on the
    shapes only and nothing is read back), two replays."""
    rirs, audio, rir_of, shift = ragged_case()
    rng = np.random.default_rng(5)
    noises = ag.NoiseTable([make_audio(rng, 900, dc=0.0), make_audio(rng, 2000, dc=0.0)], SR)
    samples, offsets, rec, table, _, _ = _ragged()
    rec = ag.Recipe(rec.rir, [[(u % 2, 10 * u, 10.0, bool(u % 3))] for u in range(len(rec))], rec.shift_output)
    want, woff, wclip = ag.augment(samples, offsets, rec, table, noises, device=DEV)
    prep = ag.prepare(samples, offsets, rec, table, noises, device=DEV)
    prep.launch()                                                                   # warm: tables and attributes are set
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


# ---- composition with the MFCCs and the extractor ------------------------------------------------------------------------------------

def test_extract_from_wav_scp_with_an_augmenter(tmp_path):
    from neuralplda_amd import models
    params = xvec_ref.make_params()
    m = xvec_ref.load_into(models.XVectorNet_ETDNN_12Layer(), params).to(DEV).eval().requires_grad_(False)
    o, vad = opts_16k(), features.VadOptions()
    rng = np.random.default_rng(12)
    scp = str(tmp_path / "wav.scp")
    with open(scp, "w") as fh:
        for i, secs in enumerate((1.0, 0.7, 1.3, 0.9, 1.1, 0.8)):
            p = str(tmp_path / f"utt{i}.wav")
            kf.write_wav(p, make_audio(rng, int(secs * SR)), SR)
            fh.write(f"utt{i} {p}\n")
    rirs = ag.RirTable([ref.make_rir(rng, L, p) for L, p in ((400, 20), (900, 100))], SR)
    noises = ag.NoiseTable([make_audio(rng, n, dc=0.0) for n in (3000, 8000, 12000)], SR)
    entries = kf.read_scp(scp)
    for per_call in (6, 4):
        keys, xv, dropped = m.extract_from_wav_scp(scp, mfcc=o, vad=vad, utts_per_call=per_call,
                                                   augmenter=ag.Augmenter(rirs, noises, seed=8))
        aug = ag.Augmenter(rirs, noises, seed=8)                                    # by hand, the same draws (seed 8: all five kinds)
        hk, parts, kinds = [], [], set()
        for lo in range(0, 6, per_call):
            pk, offsets, samples = kf.load_wav_scp(scp, entries=entries[lo:lo + per_call], sample_frequency=SR)
            rec = aug.draw(np.diff(offsets))
            kinds |= {(int(r) >= 0, len(e)) for r, e in zip(rec.rir, rec.additive)}
            s2, o2, _ = ag.augment(samples, offsets, rec, rirs, noises, device=DEV)
            frames, lengths = mfcc.compute_mfcc(s2, o2, o, DEV)
            prep = features.prepare_frames(pk, frames, lengths, vad, 300, 25)
            hk += prep.keys
            with torch.no_grad():
                parts.append(m.extract_ragged(prep.frames, prep.lengths))
        assert keys == hk and len(keys) == 6 and dropped == [] and len(kinds) >= 4
        assert torch.equal(xv, torch.cat(parts))
    k0, x0, d0 = m.extract_from_wav_scp(scp, mfcc=o, vad=vad, utts_per_call=4, augmenter=None)
    pk, offsets, samples = kf.load_wav_scp(scp, sample_frequency=SR)                # today's path, by hand
    frames, lengths = mfcc.compute_mfcc(samples, offsets, o, DEV)
    prep = features.prepare_frames(pk, frames, lengths, vad, 300, 25)
    with torch.no_grad():
        x1 = m.extract_ragged(prep.frames, prep.lengths)
    assert k0 == prep.keys and torch.equal(x0, x1)
    assert torch.equal(m.extract_from_wav_scp(scp, mfcc=o, vad=vad, utts_per_call=4)[1], x0)
    assert not torch.equal(xv, x0)                                                  # the augmenter did change the audio
