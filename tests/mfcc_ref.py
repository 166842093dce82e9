"""NumPy restatement of `compute-mfcc-feats --dither=0` (csrc/nplda_mfcc.hip, neuralplda_amd/mfcc.py), shared by the MFCC
tests and tools/bench_mfcc.py.  A plain helper, not a conftest.

There is no Kaldi next to this project, so the list in design/k14_mfcc.md is the specification and this file restates it
without using the product's tables: `mfcc64` in float64 with np.fft.rfft, `mfcc32` with every array and every intermediate
in float32 and the DFT as a float32 MATRIX PRODUCT (cos / sin table computed in float64 and rounded once) — the unit of
error of tests/fp32_units: a direct sum, not an fp32 FFT, whose shorter sums no direct product can reach — and `write_wav`,
a RIFF writer for test inputs.  Options are read by attribute (sample_frequency, frame_length, ...), so any object with
MfccOptions' fields will do."""
import functools
import struct

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def sizes(o):
    """(N, S, P): samples per frame, per shift, and the smallest power of two >= N."""
    N = int(o.sample_frequency * 0.001 * o.frame_length)
    S = int(o.sample_frequency * 0.001 * o.frame_shift)
    P = 1
    while P < N:
        P *= 2
    return N, S, P


def num_frames(n, o):
    N, S, _ = sizes(o)
    if o.snip_edges:
        return 0 if n < N else 1 + (n - N) // S
    return (n + S // 2) // S


def reflect(i, n):
    """Index i reflected until it lies in [0, n): i < 0 -> -i - 1, i >= n -> 2 n - 1 - i."""
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - 1 - i
    return i


def frame_indices(n, o):
    """(T, N) sample indices of every frame of an utterance of n samples."""
    N, S, _ = sizes(o)
    T = num_frames(n, o)
    idx = np.empty((T, N), dtype=np.int64)
    for f in range(T):
        start = f * S if o.snip_edges else f * S + S // 2 - N // 2
        if 0 <= start and start + N <= n:
            idx[f] = np.arange(start, start + N)
        else:
            idx[f] = [reflect(start + i, n) for i in range(N)]
    return idx


def window(o):
    N = sizes(o)[0]
    a = 2.0 * np.pi * np.arange(N, dtype=np.float64) / (N - 1)
    if o.window_type == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if o.window_type == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if o.window_type == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    assert o.window_type == "rectangular", o.window_type
    return np.ones(N)


def mel(f):
    return 1127.0 * np.log(1.0 + f / 700.0)


def banks(o):
    """(B, P / 2 + 1) weights; the column of the Nyquist bin is there and is zero."""
    return _banks(float(o.sample_frequency), sizes(o)[2], int(o.num_mel_bins), float(o.low_freq), float(o.high_freq))


@functools.lru_cache(maxsize=None)
def _banks(sample_frequency, P, B, low_freq, high_freq):
    high = high_freq if high_freq > 0 else 0.5 * sample_frequency + high_freq
    lo, hi = mel(low_freq), mel(high)
    d = (hi - lo) / (B + 1)
    w = np.zeros((B, P // 2 + 1))
    for b in range(B):
        left, centre, right = lo + b * d, lo + (b + 1) * d, lo + (b + 2) * d
        for k in range(P // 2):
            m = mel(k * sample_frequency / P)
            if left < m <= centre:
                w[b, k] = (m - left) / (centre - left)
            elif centre < m < right:
                w[b, k] = (right - m) / (right - centre)
    return w


def dct(B):
    """The full (B, B) orthonormal DCT-II."""
    D = np.empty((B, B))
    j = np.arange(B)
    D[0] = np.sqrt(1.0 / B)
    for c in range(1, B):
        D[c] = np.sqrt(2.0 / B) * np.cos(np.pi / B * (j + 0.5) * c)
    return D


def lifter(C, L):
    c = np.arange(C)
    return 1.0 + 0.5 * L * np.sin(np.pi * c / L) if L != 0 else np.ones(C)


def _mfcc(samples, o, dt, direct):
    samples = np.asarray(samples)
    assert samples.dtype == np.int16 and samples.ndim == 1
    N, _, P = sizes(o)
    B, C = o.num_mel_bins, o.num_ceps
    idx = frame_indices(samples.shape[0], o)
    T = idx.shape[0]
    if T == 0:
        return np.zeros((0, C), dt), np.zeros((0, B), dt)
    x = samples[idx].astype(dt)
    if o.remove_dc_offset:
        x = x - (x.sum(axis=1, dtype=dt) / dt(N))[:, None]
    E = (x * x).sum(axis=1, dtype=dt)
    c = dt(o.preemphasis_coefficient)
    y = np.empty_like(x)
    y[:, 1:] = x[:, 1:] - c * x[:, :-1]
    y[:, 0] = x[:, 0] - c * x[:, 0]
    y = y * window(o).astype(dt)[None, :]
    if not o.raw_energy:
        E = (y * y).sum(axis=1, dtype=dt)
    logE = np.log(np.maximum(E, dt(FLT_EPSILON)))
    if o.energy_floor > 0:
        logE = np.maximum(logE, np.log(dt(o.energy_floor)))
    if direct:
        ang = 2.0 * np.pi * ((np.arange(N)[:, None] * np.arange(P // 2)[None, :]) % P) / P
        re, im = y @ np.cos(ang).astype(dt), y @ np.sin(ang).astype(dt)
        pw = re * re + im * im
    else:
        sp = np.fft.rfft(y, n=P, axis=1)[:, :P // 2]
        pw = sp.real * sp.real + sp.imag * sp.imag
    assert pw.dtype == dt
    energies = pw @ banks(o)[:, :P // 2].T.astype(dt)
    me = np.log(np.maximum(energies, dt(FLT_EPSILON)))
    out = (me @ dct(B)[:C].T.astype(dt)) * lifter(C, o.cepstral_lifter).astype(dt)[None, :]
    if o.use_energy:
        out[:, 0] = logE
    assert out.dtype == dt and energies.dtype == dt
    return out, energies


def mfcc64(samples, o, with_energies=False):
    """int16 samples of ONE utterance -> (T, num_ceps) float64 [, the (T, B) mel energies before floor and log]."""
    out, en = _mfcc(samples, o, np.float64, False)
    return (out, en) if with_energies else out


def mfcc32(samples, o):
    """The same stages in float32, the DFT as a float32 matrix product: the unit of error."""
    return _mfcc(samples, o, np.float32, True)[0]


def batch(fn, samples, offsets, o):
    """fn (mfcc64 / mfcc32) over the utterances samples[offsets[u]:offsets[u + 1]], rows one after the other."""
    parts = [fn(samples[offsets[u]:offsets[u + 1]], o) for u in range(len(offsets) - 1)]
    return np.concatenate(parts) if parts else np.zeros((0, o.num_ceps))


def floor_output(o):
    """What digital silence (and, with remove_dc_offset, any constant) gives: c0 = log(FLT_EPSILON),
    c_k = lifter_k log(FLT_EPSILON) sum_j D[k][j]."""
    le = np.log(FLT_EPSILON)
    out = lifter(o.num_ceps, o.cepstral_lifter) * le * dct(o.num_mel_bins)[:o.num_ceps].sum(axis=1)
    if o.use_energy:
        out[0] = le
    return out


# ---- RIFF writer ---------------------------------------------------------------------------------------------------------

PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def wav_bytes(samples, rate, channels=1, bits=16, tag=1, extensible=False, extra=(), data_size=None, sub_tag=1):
    """A RIFF/WAVE file as bytes.  samples: int16 (frames,) or (frames, channels) — or, for bits != 16, the raw body bytes;
    extra: [(chunk id, body bytes)] placed between fmt and data (odd-sized bodies are padded); data_size: the size field of
    the data chunk if it is to differ from the body (0, 0xFFFFFFFF, or more than there is)."""
    body = samples if isinstance(samples, (bytes, bytearray)) else np.ascontiguousarray(samples, dtype="<i2").tobytes()
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", sub_tag) + PCM_GUID_TAIL
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, cb in extra:
        chunks += cid + struct.pack("<I", len(cb)) + cb + (b"\0" if len(cb) & 1 else b"")
    chunks += b"data" + struct.pack("<I", len(body) if data_size is None else data_size) + body
    return b"RIFF" + struct.pack("<I", (4 + len(chunks)) & 0xFFFFFFFF) + b"WAVE" + chunks


def write_wav(path, samples, rate, **kw):
    with open(path, "wb") as fh:
        fh.write(wav_bytes(samples, rate, **kw))
