"""The MFCC front end without a GPU: the restatement tests/mfcc_ref.py and the host code (neuralplda_amd/mfcc.py, the wave
readers of kaldi_format.py) held to facts worked out by hand, the C ABI's argument checks, and the kernel's resources."""
import ctypes
import os

import numpy as np
import pytest

from neuralplda_amd import kaldi_format as kf, mfcc
from tests import fp32_units, mfcc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)

CONF_8K = """--sample-frequency=8000
--frame-length=25 # the default is 25
--low-freq=20 # the default.
--high-freq=3700 # the default is zero meaning use the Nyquist (8k in this case).
--num-mel-bins=23
--num-ceps=23
--snip-edges=false
"""


def opts_8k(**kw):
    return mfcc.MfccOptions(**{**dict(sample_frequency=8000, low_freq=20, high_freq=3700, num_mel_bins=23, num_ceps=23,
                                      snip_edges=False), **kw})


def opts_16k(**kw):
    return mfcc.MfccOptions(**{**dict(sample_frequency=16000, low_freq=20, high_freq=7600, num_mel_bins=30, num_ceps=30,
                                      snip_edges=False), **kw})


def test_inputs(rng, n, dc=2000.0, sigma=3000.0, rate=16000.0):
    """Gaussian noise plus three sinusoids and a DC offset, clipped to int16 (the GPU tests' inputs)."""
    t = np.arange(n) / rate
    x = rng.standard_normal(n) * sigma + dc
    for f, a in ((220.0, 4000.0), (1330.0, 2500.0), (3100.0, 1500.0)):
        x += a * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


test_inputs.__test__ = False


# ---- framing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("snip, n, frames", [(True, 399, 0), (True, 400, 1), (True, 559, 1), (True, 560, 2), (False, 79, 0),
                                             (False, 80, 1), (False, 239, 1), (False, 240, 2)])
def test_frame_counts_at_16k(snip, n, frames):
    o = mfcc.MfccOptions(snip_edges=snip)
    assert (o.frame_size, o.shift, o.padded_size) == (400, 160, 512) == mfcc_ref.sizes(o)
    assert int(mfcc.num_frames(n, o)) == frames == mfcc_ref.num_frames(n, o)
    assert mfcc_ref.frame_indices(n, o).shape == (frames, 400)


def test_sizes_at_8k():
    o = opts_8k()
    assert (o.frame_size, o.shift, o.padded_size) == (200, 80, 256) == mfcc_ref.sizes(o)
    assert mfcc.num_frames(np.array([39, 40, 119, 120]), o).tolist() == [0, 1, 1, 2]


def test_reflection():
    o = mfcc.MfccOptions(snip_edges=False)
    idx = mfcc_ref.frame_indices(240, o)
    assert idx.shape == (2, 400)
    # frame 0 starts at 80 - 200 = -120: -120 .. -1 read 119 .. 0, then 0 .. 239, then 240 .. 279 read 239 .. 200
    assert idx[0, :5].tolist() == [119, 118, 117, 116, 115] and idx[0, -5:].tolist() == [204, 203, 202, 201, 200]
    assert idx[0, 119:122].tolist() == [0, 0, 1] and idx[0, 359:362].tolist() == [239, 239, 238]
    # frame 1 starts at 40: 40 .. 239, then 240 .. 439 read 239 .. 40
    assert idx[1, :5].tolist() == [40, 41, 42, 43, 44] and idx[1, -5:].tolist() == [44, 43, 42, 41, 40]
    # n = 80: one frame from -120; -120 reflects to 119, which is still outside and reflects to 40
    one = mfcc_ref.frame_indices(80, o)
    assert one.shape == (1, 400) and one.min() == 0 and one.max() == 79
    assert one[0, :5].tolist() == [40, 41, 42, 43, 44] and one[0, -5:].tolist() == [44, 43, 42, 41, 40]
    assert one[0, 39:42].tolist() == [79, 79, 78] and one[0, 119:122].tolist() == [0, 0, 1]
    assert mfcc_ref.reflect(-120, 80) == 40 and mfcc_ref.reflect(-81, 80) == 79 and mfcc_ref.reflect(279, 80) == 40
    # the kernel's closed form (period 2 n) is the same map
    for n in (80, 81, 240):
        for i in range(-3 * n, 4 * n):
            m = i % (2 * n)
            assert (m if m < n else 2 * n - 1 - m) == mfcc_ref.reflect(i, n)


# ---- tables -------------------------------------------------------------------------------------------------------------

def test_tables():
    for B in (23, 30):
        D = mfcc_ref.dct(B)
        assert np.abs(D @ D.T - np.eye(B)).max() <= 1e-12
    assert mfcc_ref.lifter(30, 22.0)[0] == 1.0 and np.all(mfcc_ref.lifter(13, 0.0) == 1.0)
    for o in (opts_8k(), opts_16k()):
        w = mfcc_ref.window(o)
        assert w[0] == 0.0 and abs(w[-1]) < 1e-12 and np.allclose(w, w[::-1], atol=1e-12)
        bk = mfcc_ref.banks(o)
        P = o.padded_size
        assert bk.shape == (o.num_mel_bins, P // 2 + 1) and (bk >= 0).all() and ((bk > 0).sum(axis=1) >= 1).all()
        assert (bk[:, P // 2] == 0).all()                         # no bank touches the Nyquist bin
        # the product's tables are the restatement's
        assert np.array_equal(mfcc.window_table(o), w)
        assert np.abs(mfcc.bank_table(o) - bk[:, :P // 2]).max() <= 1e-12
        want = mfcc_ref.dct(o.num_mel_bins)[:o.num_ceps] * mfcc_ref.lifter(o.num_ceps, o.cepstral_lifter)[:, None]
        assert np.abs(mfcc.dct_table(o) - want).max() <= 1e-12


def test_fragment_images_hold_the_tables():
    """The three images in the kernel's fragment order, read back element by element."""
    for o in (opts_8k(), opts_16k()):
        N, P, B, C = o.frame_size, o.padded_size, o.num_mel_bins, o.num_ceps
        KB, NBW, MB = (N + 15) // 16, P // 128, 2
        img = mfcc.dft_image(o)
        assert img.shape == (KB, 4, 2 * NBW, 64, 4) and img.dtype == np.float32
        rng = np.random.default_rng(0)
        for _ in range(300):
            kb, w, u, lane, i = (int(rng.integers(s)) for s in img.shape)
            n, k = 16 * kb + 4 * (lane >> 4) + i, 16 * (w * NBW + u % NBW) + (lane & 15)
            trig = np.cos if u < NBW else np.sin
            want = np.float32(trig(2 * np.pi * ((n * k) % P) / P)) if n < N else np.float32(0)
            assert img[kb, w, u, lane, i] == want
        bank = mfcc._frag(mfcc.bank_table(o), P // 32, MB)
        dct = mfcc._frag(mfcc.dct_table(o), MB, MB)
        assert bank.shape == (P // 32, MB, 64, 4) and dct.shape == (MB, MB, 64, 4)
        bt, dt = mfcc.bank_table(o).astype(np.float32), mfcc.dct_table(o).astype(np.float32)
        for _ in range(300):
            bb, mb, lane, i = (int(rng.integers(s)) for s in bank.shape)
            b, k = 16 * mb + (lane & 15), 16 * bb + 4 * (lane >> 4) + i
            assert bank[bb, mb, lane, i] == (bt[b, k] if b < B else 0)
            kb, cb, lane, i = (int(rng.integers(s)) for s in dct.shape)
            c, b = 16 * cb + (lane & 15), 16 * kb + 4 * (lane >> 4) + i
            assert dct[kb, cb, lane, i] == (dt[c, b] if c < C and b < B else 0)


# ---- the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", [opts_8k(), opts_16k(), opts_16k(use_energy=False), mfcc.MfccOptions()],
                         ids=["8k", "16k", "16k-no-energy", "defaults"])
def test_floor_output(o):
    want = mfcc_ref.floor_output(o)
    for x in (np.zeros(2000, np.int16), np.full(2000, 1234, np.int16)):
        got = mfcc_ref.mfcc64(x, o)
        assert got.shape[0] == int(mfcc.num_frames(2000, o)) > 0
        assert np.abs(got - want[None, :]).max() <= 1e-9
    assert want[0] == (np.log(EPS) if o.use_energy else want[0])
    D = mfcc_ref.dct(o.num_mel_bins)
    assert abs(want[1] - mfcc_ref.lifter(o.num_ceps, o.cepstral_lifter)[1] * np.log(EPS) * D[1].sum()) < 1e-12


def test_restatements_agree_and_give_usable_units():
    """mfcc32 against mfcc64 on the GPU tests' inputs: finite, non-degenerate units, and mel energies far above the floor."""
    rng = np.random.default_rng(3)
    for o in (opts_8k(), opts_16k(), opts_16k(snip_edges=True)):
        x = test_inputs(rng, 6000, rate=o.sample_frequency)
        r64, en = mfcc_ref.mfcc64(x, o, with_energies=True)
        r32 = mfcc_ref.mfcc32(x, o)
        assert r64.shape == r32.shape == (int(mfcc.num_frames(6000, o)), o.num_ceps) and r32.dtype == np.float32
        assert en.min() >= 1e6 * EPS
        err = np.abs(r32 - r64)
        assert np.isfinite(r32).all() and 1e-7 < err.max() < 1e-3 and np.sqrt((err ** 2).mean()) > 1e-8
        assert fp32_units.ratios(r32, r64, r32) == (1.0, 1.0)
        # a direct float64 DFT gives what rfft gives
        d64 = mfcc_ref._mfcc(x, o, np.float64, True)[0]
        assert np.abs(d64 - r64).max() < 1e-9


# ---- options ------------------------------------------------------------------------------------------------------------

def test_conf_files(tmp_path):
    p = str(tmp_path / "mfcc.conf")
    with open(p, "w") as fh:
        fh.write(CONF_8K)
    o = mfcc.MfccOptions.from_conf(p)
    assert (o.sample_frequency, o.frame_length, o.low_freq, o.high_freq, o.num_mel_bins, o.num_ceps, o.snip_edges) == \
        (8000, 25, 20, 3700, 23, 23, False)
    assert o == opts_8k() and o.frame_shift == 10 and o.dither == 0 and o.window_type == "povey" and o.use_energy
    for bad, name in (("--htk-compat=true\n", "htk-compat"), ("--vtln-low=100\n", "vtln-low"),
                      ("--round-to-power-of-two=false\n", "round-to-power-of-two"), ("--allow-downsample=true\n", "allow"),
                      ("--subtract-mean=true\n", "subtract-mean")):
        with open(p, "w") as fh:
            fh.write(CONF_8K + bad)
        with pytest.raises(ValueError, match=name):
            mfcc.MfccOptions.from_conf(p)
    with open(p, "w") as fh:
        fh.write(CONF_8K + "--dither=1\n")
    with pytest.raises(ValueError, match="dither"):
        mfcc.MfccOptions.from_conf(p)
    with open(p, "w") as fh:
        fh.write("--dither=0.0\n--use-energy=false\n--window-type=hamming\n")
    o = mfcc.MfccOptions.from_conf(p)
    assert o.use_energy is False and o.window_type == "hamming"
    with pytest.raises(ValueError, match="num_ceps"):
        mfcc.MfccOptions(num_ceps=24)
    with pytest.raises(ValueError, match="window_type"):
        mfcc.MfccOptions(window_type="blackman")
    with pytest.raises(ValueError, match="dither"):
        mfcc.MfccOptions(dither=1.0)


# ---- the wave reader ----------------------------------------------------------------------------------------------------

def _scp(tmp_path, files, name="wav.scp"):
    p = str(tmp_path / name)
    with open(p, "w") as fh:
        fh.write("".join(f"{k} {f}\n" for k, f in files))
    return p


def test_wave_reader(tmp_path):
    rng = np.random.default_rng(0)
    a = rng.integers(-32768, 32768, 1001).astype(np.int16)
    st = rng.integers(-32768, 32768, (700, 2)).astype(np.int16)
    files = {"plain": mfcc_ref.wav_bytes(a, 16000),
             "list": mfcc_ref.wav_bytes(a, 16000, extra=[(b"LIST", b"INFOISFT\x04\0\0\0abc\0")]),
             "odd": mfcc_ref.wav_bytes(a, 16000, extra=[(b"junk", b"12345")]),
             "ext": mfcc_ref.wav_bytes(a, 16000, extensible=True),
             "stereo": mfcc_ref.wav_bytes(st, 16000, channels=2),
             "open": mfcc_ref.wav_bytes(a, 16000, data_size=0xFFFFFFFF),
             "zero": mfcc_ref.wav_bytes(a, 16000, data_size=0),
             "empty": mfcc_ref.wav_bytes(a[:0], 16000)}
    for k, b in files.items():
        with open(tmp_path / f"{k}.wav", "wb") as fh:
            fh.write(b)
    for k in ("plain", "list", "odd", "ext", "open", "zero"):
        rate, x = kf.read_wav(str(tmp_path / f"{k}.wav"))
        assert rate == 16000 and x.dtype == np.int16 and np.array_equal(x, a), k
    assert np.array_equal(kf.read_wav(str(tmp_path / "stereo.wav"))[1], st[:, 0])
    assert np.array_equal(kf.read_wav(str(tmp_path / "stereo.wav"), channel=1)[1], st[:, 1])
    with pytest.raises(kf.KaldiFormatError, match="channel 2"):
        kf.read_wav(str(tmp_path / "stereo.wav"), channel=2)
    order = ["odd", "empty", "stereo", "ext", "plain"]
    scp = _scp(tmp_path, [(f"utt-{k}", str(tmp_path / f"{k}.wav")) for k in order])
    keys, offsets, samples = kf.load_wav_scp(scp, sample_frequency=16000, channel=0)
    assert keys == [f"utt-{k}" for k in order] and offsets.dtype == np.int64 and samples.dtype == np.int16
    assert offsets.tolist() == [0, 1001, 1001, 1701, 2702, 3703] and samples.flags["C_CONTIGUOUS"]
    assert np.array_equal(samples, np.concatenate([a, st[:, 0], a, a]))
    k2, o2, s2 = kf.load_wav_scp(scp, entries=kf.read_scp(scp)[2:3], channel=1)
    assert k2 == ["utt-stereo"] and o2.tolist() == [0, 700] and np.array_equal(s2, st[:, 1])
    k0, o0, s0 = kf.load_wav_scp(_scp(tmp_path, [], "none.scp"))
    assert k0 == [] and o0.tolist() == [0] and s0.shape == (0,)


def test_wave_reader_errors(tmp_path):
    a = np.arange(100, dtype=np.int16)
    bad = {"eight": mfcc_ref.wav_bytes(bytes(100), 16000, bits=8),
           "float": mfcc_ref.wav_bytes(bytes(400), 16000, bits=32, tag=3),
           "extfloat": mfcc_ref.wav_bytes(a, 16000, extensible=True, sub_tag=3),
           "short": mfcc_ref.wav_bytes(a, 16000, data_size=400),
           "rate": mfcc_ref.wav_bytes(a, 8000),
           "noriff": b"RIFX" + mfcc_ref.wav_bytes(a, 16000)[4:],
           "nodata": mfcc_ref.wav_bytes(a, 16000)[:36]}
    for k, b in list(bad.items()) + [("good", mfcc_ref.wav_bytes(a, 16000))]:
        with open(tmp_path / f"{k}.wav", "wb") as fh:
            fh.write(b)
    for k, what in (("eight", "8 bits"), ("float", "format tag 3"), ("extfloat", "format tag 3"), ("short", "truncated"),
                    ("rate", "sample rate 8000"), ("noriff", "RIFF"), ("nodata", "no data chunk")):
        scp = _scp(tmp_path, [("good", str(tmp_path / "good.wav")), (f"key-{k}", str(tmp_path / f"{k}.wav"))], f"{k}.scp")
        with pytest.raises(kf.KaldiFormatError, match=f"key-{k}.*{what}"):
            kf.load_wav_scp(scp, sample_frequency=16000)
    for k, what in (("eight", "8 bits"), ("float", "format tag 3"), ("short", "truncated")):
        with pytest.raises(kf.KaldiFormatError, match=what):
            kf.read_wav(str(tmp_path / f"{k}.wav"))
    scp = _scp(tmp_path, [("piped-utt", "sph2pipe -f wav -p -c 1 /corpus/a.sph |")], "pipe.scp")
    with pytest.raises(kf.KaldiFormatError, match="piped-utt.*pipe"):
        kf.load_wav_scp(scp)
    scp = _scp(tmp_path, [("gone-utt", str(tmp_path / "missing.wav"))], "gone.scp")
    with pytest.raises(kf.KaldiFormatError, match="gone-utt"):
        kf.load_wav_scp(scp)


def test_feature_archive_writer(tmp_path):
    rng = np.random.default_rng(1)
    mats = [rng.standard_normal((T, 30)).astype(np.float32) for T in (5, 0, 17)]
    ark, scp = str(tmp_path / "m.ark"), str(tmp_path / "m.scp")
    kf.write_feature_ark(ark, ["a", "b", "c"], mats, scp)
    back = list(kf.read_feature_scp(scp))
    assert [k for k, _ in back] == ["a", "b", "c"]
    for (_, g), m in zip(back, mats):
        assert g.shape == m.shape and np.array_equal(g, m)
    feats = kf.load_feature_scp(scp, cols=30)
    assert feats.desc["rows"].tolist() == [5, 0, 17] and set(feats.desc["format"].tolist()) == {kf.FEAT_FORMATS["FM"]}


# ---- the C ABI and the kernel's resources -------------------------------------------------------------------------------

def test_entry_points_check_their_arguments(hip_lib):
    from neuralplda_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    assert "typedef struct nplda_mfcc_geometry" in hdr and ctypes.sizeof(mfcc._Geometry) == 36
    assert f"#define NPLDA_MFCC_TILE {mfcc.FRAME_TILE}" in hdr
    for name in ("nplda_mfcc_frames_f32", "nplda_mfcc_image_bytes"):
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None
    assert hip_lib.nplda_abi_version() == 4
    g16, g8 = mfcc.geometry_of(opts_16k()), mfcc.geometry_of(opts_8k())
    sz = lambda g, w: hip_lib.nplda_mfcc_image_bytes(ctypes.byref(g), w)  # noqa: E731
    assert [sz(g16, w) for w in range(4)] == [25 * 32 * 1024, 16 * 2 * 1024, 4 * 1024, 0]       # 800 KB of DFT table
    assert [sz(g8, w) for w in range(3)] == [13 * 16 * 1024, 8 * 2 * 1024, 4 * 1024]
    assert mfcc.dft_image(opts_16k()).nbytes == sz(g16, 0) and mfcc.dft_image(opts_8k()).nbytes == sz(g8, 0)
    call = lambda g, U, R: hip_lib.nplda_mfcc_frames_f32(None, None, None, U, R, ctypes.byref(g), None, None, None, None,  # noqa: E731
                                                          None, None)
    assert call(g16, 0, 0) == 0 and call(g16, 5, 0) == 0                      # nothing to do: a no-op
    assert call(g16, 3, 10) == -22                                            # NPLDA_EINVAL: null buffers
    assert hip_lib.nplda_mfcc_frames_f32(None, None, None, 0, 0, None, None, None, None, None, None, None) == -22
    for o in (mfcc.MfccOptions(sample_frequency=44100), mfcc.MfccOptions(sample_frequency=22050),      # N = 1102, 551
              mfcc.MfccOptions(frame_length=25.125), mfcc.MfccOptions(frame_length=5),                  # N = 402, P = 128
              mfcc.MfccOptions(num_mel_bins=65)):
        g = mfcc.geometry_of(o)
        assert call(g, 3, 10) == _lib.NPLDA_EUNSUPPORTED and sz(g, 0) == 0, o
    g = mfcc.geometry_of(opts_16k())
    g.C = 31
    assert call(g, 3, 10) == _lib.NPLDA_EUNSUPPORTED


def test_kernel_uses_no_scratch():
    from tests.test_kernel_resources_cpu import _resources
    res = _resources("nplda_mfcc.hip")
    assert len(res) == 4 and all("mfcc_kernel" in k for k in res), sorted(res)      # P in {256, 512} x B <= 32 or <= 64
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] + v["AGPRs"] <= 256 and v["Occupancy"] >= 2, (k, v)
