"""The augmentation without a GPU: the twin tests/augment_ref.py held to facts worked out by hand, the host code of
neuralplda_amd/augment.py (lengths, windows, tables, draws, validation), the wave writer, the C ABI's argument checks and the
transform kernels' resources.  The shapes and inputs of the GPU tests are defined here so that their conditions can be
checked without a device."""
import ctypes
import functools
import os

import numpy as np
import pytest

from neuralplda_amd import augment as ag, kaldi_format as kf
from tests import augment_ref as ref, fp32_units
from tests.test_mfcc_cpu import test_inputs as make_audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000

# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------------

GRID_N = (1, 255, 256, 257, 513, 5000)
GRID_L = (1, 2, 255, 256, 257, 1000)
FLAGS = ((True, True), (True, False), (False, True), (False, False))  # (shift_output, normalize_output)


def peaks_of(L):
    return sorted({0, L // 2, L - 1})


@functools.lru_cache(maxsize=None)
def grid_case(L):
    """For one RIR length: the impulse responses with the peak at 0, in the middle and at L - 1, and one utterance per
    (n, peak, shift_output, normalize_output) -> (rirs, audio, [(utterance, rir, shift, normalize)])."""
    rng = np.random.default_rng(1000 + L)
    rirs = [ref.make_rir(rng, L, p) for p in peaks_of(L)]
    audio = [make_audio(rng, n) for n in GRID_N]
    return rirs, audio, [(a, r, sh, nm) for a in range(len(GRID_N)) for r in range(len(rirs)) for sh, nm in FLAGS]


@functools.lru_cache(maxsize=None)
def ragged_case():
    """24 utterances of 0 - 6 000 samples (one of length 0) over 5 impulse responses; a third of them has none."""
    rng = np.random.default_rng(77)
    ns = [0, 1, 300, 4000, 6000] + [int(v) for v in rng.integers(2, 6001, 19)]
    order = rng.permutation(24)
    ns = [ns[i] for i in order]
    rirs = [ref.make_rir(rng, L, p) for L, p in ((1, 0), (200, 0), (700, 350), (1000, 999), (1800, 40))]
    audio = [make_audio(rng, n) for n in ns]
    rir_of = [int(rng.integers(5)) if u % 3 else -1 for u in range(24)]
    shift = [bool(u % 4 != 1) for u in range(24)]
    return rirs, audio, rir_of, shift


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Utterances with a RIR AND additive entries — the only place where the early-window power P_sig shows in the output (it
    scales the entries) — with normalize_output on and off, and responses whose early window [a, b) hits its clamps: peak at
    0 (a = 0), peak at L - 1 (b = L), a 10-tap response (both), and one with neither
    -> (rirs, noises, audio, [(rir, additive, shift_output, normalize_output)])."""
    rng = np.random.default_rng(2028)
    rirs = [ref.make_rir(rng, L, p) for L, p in ((600, 0), (600, 599), (1500, 400), (10, 5))]
    noises = [make_audio(rng, 900, dc=0.0), make_audio(rng, 2500, dc=30.0), make_audio(rng, 7000, dc=0.0, sigma=800.0)]
    ns = (3000, 4100, 700, 2049, 513, 5000, 2600, 1300)
    audio = [make_audio(rng, n) for n in ns]
    recipe = [(0, [(0, 0, 10.0, True)], True, True),
              (1, [(1, 500, 5.0, False)], True, False),
              (2, [(0, 0, 15.0, True), (1, 100, 0.0, False)], True, True),
              (3, [(2, 0, 8.0, True)], False, True),
              (0, [(1, 0, 13.0, True), (0, 7, 17.0, True), (2, 300, 20.0, True)], False, False),
              (1, [(2, 0, 0.0, True)], True, True),
              (2, [(0, 2000, 5.0, True)], False, True),
              (3, [(1, 0, 10.0, True)], True, False)]
    return rirs, noises, audio, recipe


def big_cases():
    """(x, h) of at least 4 000 samples with a RIR: what the 16-bit tests run on (default recipe: shift and normalise)."""
    out = []
    for L in GRID_L:
        rirs, audio, _ = grid_case(L)
        out += [(audio[-1], h) for h in rirs]
    rirs, audio, rir_of, _ = ragged_case()
    out += [(x, rirs[r]) for x, r in zip(audio, rir_of) if r >= 0 and len(x) >= 4000]
    return out


# ---- the twin ------------------------------------------------------------------------------------------------------------------

def test_block_convolution_is_a_convolution():
    rng = np.random.default_rng(0)
    for n, L in ((1, 1), (1, 2), (255, 257), (256, 256), (257, 255), (1000, 300), (700, 1000)):
        x, h = make_audio(rng, n), ref.make_rir(rng, L, L // 3)
        want = np.convolve(x.astype(np.float64), h.astype(np.float64))
        got = ref.block_convolve(x, h, np.float64)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    F, G = ref.tables(np.float64)
    assert np.abs(ag.forward_table() - F).max() <= 1e-15 and np.abs(ag.inverse_table() - G).max() <= 1e-15
    # the inverse table undoes the forward one on the last 256 samples
    assert np.abs(G @ F - np.eye(512)[256:]).max() <= 1e-12


def test_the_units_transform_does_not_depend_on_the_number_of_rows():
    """augment_ref._transform pads products of fewer than MIN_ROWS rows so that every case gets the arithmetic of a matrix
    product.  What that rests on: from MIN_ROWS rows up, the float32 error of numpy's product against the float64 one is the
    same statistic whatever the number of rows, padded into a larger product or not."""
    F32, _ = ref.tables(np.float32)
    F64, _ = ref.tables(np.float64)
    rng = np.random.default_rng(0)
    big = np.zeros((256, 512), np.float32)
    big[:, 256:] = (rng.standard_normal((256, 256)) * 3000).astype(np.float32)
    want = big.astype(np.float64) @ F64.T
    rel = lambda got, rows: float(np.sqrt(((got - want[:rows]) ** 2).mean()) / np.sqrt((want[:rows] ** 2).mean()))  # noqa: E731
    whole = rel(big @ F32.T, 256)
    assert 1e-7 < whole < 1e-6
    for rows in (ref.MIN_ROWS, 13, 32, 100):
        alone = rel(big[:rows] @ F32.T, rows)
        inside = rel((big @ F32.T)[:rows], rows)
        assert 0.8 * whole <= alone <= 1.25 * whole and 0.8 * whole <= inside <= 1.25 * whole, (rows, alone, inside, whole)
    for rows in (1, 2, 5):                                                     # below MIN_ROWS: the padded product's statistic
        assert 0.7 * whole <= rel(ref._transform(big[:rows], F32), rows) <= 1.4 * whole, rows


def test_twins_agree_and_give_usable_units():
    rng = np.random.default_rng(5)
    for n, L in ((1000, 300), (5000, 1000)):
        x, h = make_audio(rng, n), ref.make_rir(rng, L, L // 2)
        for kw in (dict(), dict(shift_output=False, normalize_output=False)):
            r64, r32 = ref.augment64(x, h, **kw), ref.augment32(x, h, **kw)
            assert r32.dtype == np.float32 and r64.shape == r32.shape == (ref.output_length(n, L, kw.get("shift_output", True)),)
            err = np.abs(r32 - r64)
            rel = np.sqrt((err ** 2).mean()) / np.sqrt((r64 ** 2).mean())
            assert np.isfinite(r32).all() and 1e-7 < rel < 2e-6, rel      # the issue's prototype: 5.0e-7 - 5.8e-7
            assert fp32_units.ratios(r32, r64, r32) == (1.0, 1.0)


def test_twins_agree_with_a_rir_and_additive_entries():
    """The mixed case: augment32 against augment64, and augment64's scale held to the definition by hand — the power of
    what an entry adds is 10^(-snr / 10) times the power of x * h[a:b]."""
    rirs, noises, audio, recipe = mixed_case()
    windows = [ref.early_window(h, SR) for h in rirs]
    assert [w[1] for w in windows] == [0, 583, 384, 0] and [w[2] for w in windows] == [600, 600, 1200, 10]
    for x, (r, additive, shift, norm) in zip(audio, recipe):
        kw = dict(shift_output=shift, normalize_output=norm)
        r64, r32 = ref.augment64(x, rirs[r], additive, noises, **kw), ref.augment32(x, rirs[r], additive, noises, **kw)
        assert r64.shape == r32.shape == (ref.output_length(len(x), len(rirs[r]), shift),) and r32.dtype == np.float32
        rel = np.sqrt(((r32 - r64) ** 2).mean()) / np.sqrt((r64 ** 2).mean())
        assert np.isfinite(r32).all() and 3e-8 < rel < 2e-6, rel
        if norm:
            assert abs((r64 ** 2).mean() / (x.astype(np.float64) ** 2).mean() - 1.0) < 1e-12
    # utterance 4: no normalisation; its first entry alone, from the start, periodic
    x, (r, additive, shift, norm) = audio[4], recipe[4]
    item, start, snr, repeat = additive[0]
    assert start == 0 and repeat and not norm
    h64 = rirs[r].astype(np.float64)
    peak, a, b = windows[r]
    e = np.convolve(x.astype(np.float64), h64[a:b])
    added = ref.augment64(x, rirs[r], additive[:1], noises, shift_output=shift, normalize_output=False) - \
        ref.augment64(x, rirs[r], (), noises, shift_output=shift, normalize_output=False)
    z = noises[item].astype(np.float64)
    tiled = z[np.arange(len(added)) % len(z)]
    s2 = (added ** 2).sum() / (tiled ** 2).sum()
    assert abs(s2 / (10.0 ** (-snr / 10.0) * (e ** 2).mean() / (z ** 2).mean()) - 1.0) < 1e-9
    # the early window's power is not the input's: a twin (or a kernel) that took P_in for P_sig would be off by this much
    assert abs((e ** 2).mean() / (x.astype(np.float64) ** 2).mean() - 1.0) > 0.05


def test_condition_of_the_16_bit_cap():
    """On the GPU tests' inputs of at least 4 000 samples, round(augment32) and round(augment64) differ by at most 1 in every
    case, and in at most 0.25 % of the samples of all cases together (the GPU test allows the kernel twice that).  The share
    is taken over the pooled samples: these inputs have an rms near 5 000 counts, so a twin's error of 5e-7 of it flips about
    0.2 % of the roundings — in one case of 5 000 samples that is 10 +- 3 samples, a draw next to a gate at 12.5; over the
    100 766 samples of the 20 cases it measured 192 (0.191 %; single cases 0 - 0.30 %).  So that no single case hides in the
    pool, each is also held to 0.6 %: at 0.2 % a case of 4 000 - 6 000 samples expects 8 - 12 differing samples with a
    standard deviation of 3 - 3.5, and 0.6 % (24 - 36 samples) is five deviations above that."""
    cases = big_cases()
    assert len(cases) >= 20
    total = differ = 0
    for x, h in cases:
        a, _ = ref.round_int16(ref.augment32(x, h))
        b, _ = ref.round_int16(ref.augment64(x, h))
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        assert d.max() <= 1 and (d > 0).mean() <= 0.006, (len(x), len(h), int(d.max()), float((d > 0).mean()))
        total, differ = total + d.size, differ + int((d > 0).sum())
    print(f"16-bit samples differing between the twins: {differ} of {total} ({100 * differ / total:.3f} %)")
    assert total >= 100000 and differ <= 0.0025 * total


def test_exact_path_by_hand():
    x = np.array([100, -200, 300, 400], np.int16)
    z = np.array([3, -4], np.int16)                                       # P_noise = 12.5
    p_in = (100 ** 2 + 200 ** 2 + 300 ** 2 + 400 ** 2) / 4.0            # 75 000
    s = np.float32(np.sqrt(10.0 ** -1.0 * p_in / 12.5))
    got = ref.augment32(x, None, [(0, 1, 10.0, True)], [z], normalize_output=False)
    want = x.astype(np.float32)
    want[1:] = want[1:] + s * np.array([3, -4, 3], np.float32)
    assert np.array_equal(got, want)
    once = ref.augment32(x, None, [(0, 1, 10.0, False)], [z], normalize_output=False)
    assert np.array_equal(once[:3], want[:3]) and once[3] == 400.0
    past = ref.augment32(x, None, [(0, 4, 10.0, True)], [z], normalize_output=False)
    silent = ref.augment32(x, None, [(0, 0, 10.0, True)], [np.zeros(5, np.int16)], normalize_output=False)
    assert np.array_equal(past, x.astype(np.float32)) and np.array_equal(silent, x.astype(np.float32))
    assert np.array_equal(ref.augment32(x, None, volume=0.5), np.float32(0.5) * x.astype(np.float32))
    assert np.allclose(ref.augment64(x, None, [(0, 1, 10.0, True)], [z], normalize_output=False), want, rtol=1e-6)
    # normalisation restores the input power
    rng = np.random.default_rng(2)
    xx, zz = make_audio(rng, 3000), make_audio(rng, 500, dc=0.0)
    out = ref.augment64(xx, None, [(0, 0, 5.0, True)], [zz])
    assert abs((out ** 2).mean() / (xx.astype(np.float64) ** 2).mean() - 1.0) < 1e-12
    v, clipped = ref.round_int16(np.array([0.5, 1.5, 2.5, -0.5, 32767.4, 32767.5, -32768.5, -32769.0, 1e9]))
    assert v.tolist() == [0, 2, 2, 0, 32767, 32767, -32768, -32768, 32767] and clipped == 3


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------

def test_peak_and_early_window_at_the_clamps():
    h = np.zeros(2000, np.float32)
    h[[5, 900]] = 0.7
    h[7] = -3.0                                                           # the largest VALUE, not the largest magnitude
    assert ref.early_window(h, SR) == (5, 0, 805) == ag.early_window(h, SR)          # a clamped at 0, first of two equal peaks
    h[1990] = 0.8
    assert ref.early_window(h, SR) == (1990, 1974, 2000) == ag.early_window(h, SR)   # b clamped at L
    h[1000] = 2.0
    assert ref.early_window(h, SR) == (1000, 984, 1800) == ag.early_window(h, SR)
    assert ag.early_window(np.ones(1, np.float32), 8000) == (0, 0, 1) == ref.early_window(np.ones(1), 8000)
    assert ag.early_window(h, 8000) == (1000, 992, 1400) == ref.early_window(h, 8000)
    t = ag.RirTable([h, np.ones(1, np.float32)], SR)
    assert t.peaks.tolist() == [1000, 0] and t.early_begin.tolist() == [984, 0] and t.early_lengths.tolist() == [816, 1]
    # partitions: 8 and 1 for the responses, then 4 and 1 for the early windows
    assert t.parts.tolist() == [[0, 8, 9, 4], [8, 1, 13, 1]] and t.spectra_bytes() == 14 * 2048


def test_output_lengths_offsets_and_workspace(hip_lib):
    rirs = ag.RirTable([np.ones(1, np.float32), ref.make_rir(np.random.default_rng(0), 300, 10)], SR)
    lengths = np.array([0, 1, 1000, 1000, 257, 5])
    rec = ag.Recipe([-1, 1, 1, 1, 0, -1], shift_output=[True, True, True, False, False, False])
    assert ag.output_lengths(lengths, rec, rirs).tolist() == [0, 1, 1000, 1299, 257, 5]
    assert ag.output_lengths(lengths, ag.Recipe.clean(6), None).tolist() == lengths.tolist()
    lay = ag._layout(lengths, rec, rirs)
    assert lay["conv"].tolist() == [0, 300, 1299, 1299, 257, 0] and lay["blocks"].tolist() == [0, 2, 6, 6, 2, 0]
    assert lay["groups"].tolist() == [0, 1, 1, 1, 1, 0]
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    want = 2 * up(16 * 2048) + up(16 * 1024) + up(16 * 8) + up(5 * 8) + up(6 * 8) + 2 * up(6 * 4) + up(0)
    assert ag.workspace_bytes(lengths, rec, rirs) == want == hip_lib.nplda_augment_workspace_bytes(6, 0, 16, 5)
    assert hip_lib.nplda_augment_workspace_bytes(-1, 0, 0, 0) == 0
    # the split by whole utterances
    assert ag._pieces(lengths, rec, rirs, 1 << 30) == [(0, 6)]
    pieces = ag._pieces(lengths, rec, rirs, 40000)
    assert pieces[0][0] == 0 and pieces[-1][1] == 6 and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and len(pieces) >= 3
    for lo, hi in pieces:
        assert hi - lo == 1 or ag.workspace_bytes(lengths[lo:hi], rec.select(np.arange(lo, hi)), rirs) <= 40000
    assert ag._pieces(lengths, rec, rirs, 1) == [(u, u + 1) for u in range(6)]       # never less than one utterance


def test_table_images_hold_the_tables():
    rng = np.random.default_rng(0)
    for table, NU in ((ag.forward_table(), 8), (ag.inverse_table(), 4)):
        img = ag.table_image(table)
        assert img.shape == (32, 4, NU, 64, 4) and img.dtype == np.float32
        t32 = table.astype(np.float32)
        for _ in range(400):
            kb, w, u, lane, i = (int(rng.integers(s)) for s in img.shape)
            assert img[kb, w, u, lane, i] == t32[16 * (NU * w + u) + (lane & 15), 16 * kb + 4 * (lane >> 4) + i]


def test_augmenter_draws_equal_the_restatement():
    rng = np.random.default_rng(4)
    rirs = ag.RirTable([ref.make_rir(rng, L, 3) for L in (50, 80, 120)], SR)
    lens = [4000, 9000, 30000, 2500, 16000, 700, 1200]
    labels = ["noise", "noise", "music", "babble", "babble", "babble", "music"]
    noises = ag.NoiseTable([make_audio(rng, n, dc=0.0) for n in lens], SR, labels=labels)
    lengths = [int(v) for v in rng.integers(1, 80000, 60)]
    items = {k: [i for i, s in enumerate(labels) if s == k] for k in ("noise", "music", "babble")}
    for seed, kinds in ((0, ag.KINDS), (7, ("noise", "babble")), (7, ("clean", "reverb"))):
        rec = ag.Augmenter(rirs, noises, kinds=kinds, seed=seed).draw(lengths)
        want = ref.draw(seed, lengths, kinds, 3, items, lens, SR)
        assert [int(r) for r in rec.rir] == [w[0] for w in want] and rec.additive == [w[1] for w in want]
        assert rec.shift_output.all() and rec.normalize_output.all() and (rec.volume == 0).all()
        rec.validate(lengths, rirs, noises)
    a, b = ag.Augmenter(rirs, noises, seed=3), ag.Augmenter(rirs, noises, seed=3)
    ra, rb = a.draw(lengths), b.draw(lengths)
    assert ra.additive == rb.additive and np.array_equal(ra.rir, rb.rir)              # a seed repeats a run
    assert a.draw(lengths).additive != ra.additive                                       # and the generator moves on
    kinds_seen = {("reverb" if r >= 0 else "clean") if not e else ("noise" if not e[0][3] else "music" if len(e) == 1 else
                                                                    "babble") for r, e in zip(ra.rir, ra.additive)}
    assert kinds_seen == set(ag.KINDS)
    noise_recipes = [e for e in ra.additive if e and not e[0][3]]
    for e in noise_recipes:                                                              # end to end with a 1 s gap
        for p, q in zip(e, e[1:]):
            assert q[1] == p[1] + lens[p[0]] + SR and labels[p[0]] == "noise"
    with pytest.raises(ValueError, match="music"):
        ag.Augmenter(rirs, ag.NoiseTable([np.zeros(4, np.int16)], SR, labels=["noise"]), seed=0)
    with pytest.raises(ValueError, match="reverb"):
        ag.Augmenter(None, noises, seed=0)
    with pytest.raises(ValueError, match="kinds"):
        ag.Augmenter(rirs, noises, kinds=("speed",))


def test_recipe_validation_names_the_utterance():
    rirs = ag.RirTable([np.ones(3, np.float32)], SR)
    noises = ag.NoiseTable([np.ones(10, np.int16)], SR)
    lengths = [100, 100, 100]
    ag.Recipe([-1, 0, -1], [[], [(0, 5, 10.0, True)], []]).validate(lengths, rirs, noises)
    for rec, what in ((ag.Recipe([-1, 1, -1]), "utterance 1: RIR 1"), (ag.Recipe([-1, -1, -2]), "utterance 2: RIR -2"),
                      (ag.Recipe([-1, -1, -1], [[], [], [(1, 0, 10.0, True)]]), "utterance 2: noise item 1"),
                      (ag.Recipe([-1, -1, -1], [[(0, -1, 10.0, True)], [], []]), "utterance 0: additive entry starting"),
                      (ag.Recipe([-1, -1, -1], [[], [(0, 0, float("nan"), True)], []]), "utterance 1: snr_db"),
                      (ag.Recipe([-1, -1, -1], [[], [(0, 0, 10.0)], []]), "utterance 1: an additive entry"),
                      (ag.Recipe([-1, -1, -1], volume=[0, np.inf, 0]), "utterance 1: volume")):
        with pytest.raises(ValueError, match=what):
            rec.validate(lengths, rirs, noises)
    with pytest.raises(ValueError, match="utterance 0: RIR 0"):
        ag.Recipe([0, -1, -1]).validate(lengths, None, None)
    with pytest.raises(ValueError, match="recipe of 3"):
        ag.Recipe.clean(3).validate([1, 2], rirs, noises)
    with pytest.raises(ValueError, match="2 additive lists"):
        ag.Recipe([-1, -1, -1], [[], []])
    with pytest.raises(ValueError, match="RIR 1: 32769 taps"):
        ag.RirTable([np.ones(2, np.float32), np.ones(32769, np.float32)], SR)
    with pytest.raises(ValueError, match="RIR 0: empty"):
        ag.RirTable([np.ones(0, np.float32)], SR)
    with pytest.raises(ValueError, match="noise item 0: expected int16"):
        ag.NoiseTable([np.ones(4, np.float32)], SR)
    c = ag.Recipe.clean(4)
    assert (c.rir == -1).all() and not c.normalize_output.any() and c.shift_output.all() and (c.volume == 0).all()
    assert ctypes.sizeof(ag._Call) == 19 * 8 + 7 * 8 + 8 and ag.UTT_DTYPE.itemsize == 64 and ag.ENTRY_DTYPE.itemsize == 32


# ---- the wave writer ------------------------------------------------------------------------------------------------------------

def test_write_wav_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    for n, rate in ((0, 16000), (1, 8000), (1001, 16000)):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        p = str(tmp_path / f"w{n}.wav")
        kf.write_wav(p, x, rate)
        r, y = kf.read_wav(p)
        assert r == rate and y.dtype == np.int16 and np.array_equal(x, y)
        assert os.path.getsize(p) == 44 + 2 * n
    with pytest.raises(ValueError, match="int16"):
        kf.write_wav(str(tmp_path / "f.wav"), np.zeros(4, np.float32), 16000)
    rirs = ag.RirTable([str(tmp_path / "w1001.wav")], 16000)                  # tables load wave files: counts, unscaled
    assert np.array_equal(rirs.taps, x.astype(np.float32))
    noises = ag.NoiseTable([str(tmp_path / "w1001.wav"), x[:7]], 16000)
    assert np.array_equal(noises.samples, np.concatenate([x, x[:7]])) and noises.offsets.tolist() == [0, 1001, 1008]
    with pytest.raises(ValueError, match="sample rate 8000"):
        ag.NoiseTable([str(tmp_path / "w1.wav")], 16000)


# ---- the C ABI and the kernels' resources --------------------------------------------------------------------------------------

def test_entry_points_check_their_arguments(hip_lib):
    from neuralplda_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    for name in ("nplda_augment_table_bytes", "nplda_augment_spectra_f32", "nplda_augment_power_i64",
                 "nplda_augment_workspace_bytes", "nplda_augment_batch"):
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None and f"{name}(" in hdr, name
    assert hip_lib.nplda_abi_version() == 4
    for k, v in (("BLOCK", ag.BLOCK), ("TILE", ag.TILE), ("GROUP", ag.GROUP), ("CHUNK", ag.CHUNK), ("MAX_RIR", ag.MAX_RIR)):
        assert f"#define NPLDA_AUGMENT_{k} {v}" in hdr
    assert [hip_lib.nplda_augment_table_bytes(w) for w in (0, 1, 2, -1)] == [1 << 20, 1 << 19, 0, 0]
    assert ag.table_image(ag.forward_table()).nbytes == 1 << 20 and ag.table_image(ag.inverse_table()).nbytes == 1 << 19
    EINVAL, ENOSPC, EUNSUPPORTED = -22, -28, _lib.NPLDA_EUNSUPPORTED
    spectra = lambda F, R, lo, hi, p=None: hip_lib.nplda_augment_spectra_f32(p, p, p, p, F, R, lo, hi, p, p, None)  # noqa: E731
    assert spectra(0, 0, 0, 0) == 0                                           # no filters: a no-op
    assert spectra(2, 2, 0, 5) == EINVAL                                      # L = 0
    assert spectra(2, 130, 1, 32769) == EUNSUPPORTED                          # L > 32 768: before the pointers are looked at
    assert spectra(2, 129, 1, 32768) == EINVAL                                # supported, null pointers
    assert spectra(-1, 0, 1, 1) == EINVAL and spectra(2, 1, 1, 1, 4096) == EINVAL     # fewer blocks than filters
    power = lambda n, c: hip_lib.nplda_augment_power_i64(None, None, None, n, c, None, None)  # noqa: E731
    assert power(0, 0) == 0 and power(3, 2) == EINVAL and power(-1, 0) == EINVAL
    assert hip_lib.nplda_augment_batch(None, None, 0, None) == EINVAL
    c = ag._Call()
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), None, 0, None) == 0          # no utterances: a no-op
    c.n_utts, c.total_blocks, c.total_groups, c.max_rir_len, c.max_conv_len = 1, 130, 17, 32769, 33000
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), None, 0, None) == EUNSUPPORTED
    c.max_rir_len, c.max_conv_len = 100, (1 << 31) - 512
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), None, 0, None) == EUNSUPPORTED   # beyond the int32 block indexing
    c.max_conv_len = 33000
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), None, 0, None) == EINVAL      # null pointers
    c.n_utts = -1
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), None, 0, None) == EINVAL
    # every required pointer given (never dereferenced: the workspace is too small, which is found before any launch)
    c = ag._Call()
    for k, _ in ag._Call._fields_[:19]:
        setattr(c, k, 4096)
    c.n_utts, c.total_in_chunks, c.total_out_chunks = 1, 1, 1
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), 4096, 16, None) == ENOSPC
    assert hip_lib.nplda_augment_batch(ctypes.addressof(c), 4097, 1 << 20, None) == EINVAL   # workspace not 256-aligned


def test_transform_kernels_use_no_scratch():
    from tests.test_kernel_resources_cpu import _resources
    res = _resources("nplda_augment.hip")
    dft = {k: v for k, v in res.items() if "aug_dft_kernel" in k}
    assert len(dft) == 4, sorted(res)            # signal and filter spectra, synthesis, synthesis to sums of squares
    for k, v in dft.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] + v["AGPRs"] <= 256 and v["Occupancy"] >= 2, (k, v)
    for k, v in res.items():                     # nor does any other kernel of the family
        assert v["ScratchSize"] == 0, (k, v)
    assert {n for n in ("aug_mac_kernel", "aug_power_kernel", "aug_mix_sum_kernel", "aug_store_kernel", "aug_scalars_kernel")
            if any(n in k for k in res)} == {"aug_mac_kernel", "aug_power_kernel", "aug_mix_sum_kernel", "aug_store_kernel",
                                             "aug_scalars_kernel"}
