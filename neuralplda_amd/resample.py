"""Resampling and speed perturbation of 16-bit audio on the HIP device (csrc/nplda_resample.hip): a rational-ratio polyphase
windowed-sinc filter over a ragged batch, the step in front of `augment` and `mfcc`.

    keys, offsets, samples, rates = kaldi_format.load_wav_scp("data/wav.scp", return_rates=True)
    samples, offsets, clipped = resample(samples, offsets, rates, 16000)              # int16 on the device
    slow, slow_off, _ = speed_perturb(samples, offsets, 0.9, 16000)                   # 1 / 0.9 as long, lower in pitch

The filter is that of Kaldi's LinearResample and torchaudio's sinc_interp_hann (design/k29_resample.md holds the
specification; bit-compatibility with either is not claimed): with g = gcd(rin, rout), iu = rin / g, ou = rout / g and
T = rin ou ticks per second,

    y[k] = gain * sum_i w(i ou - k iu) x[i]   over |i ou - k iu| / T < ww = width / (2 fc),   fc = rolloff min(rin, rout) / 2,
    w(q) = h(q / T) / rin,   h(t) = sin(2 pi fc t) / (pi t) * (1 + cos(2 pi fc t / width)) / 2,   m = ceil(n ou / iu) outputs.

The weights are built here in float64 from the integer q and rounded once; the kernel forms each output as one float32 chain
over the taps in increasing i.  Equal rates are a copy times the gain.  Nothing is read back, two calls give the same bits,
and an utterance's result does not depend on the batch.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

__all__ = ["filter_bank", "output_lengths", "speed_rates", "resample", "speed_perturb", "prepare", "CHUNK", "MAX_UNITS",
           "MAX_TAPS"]

CHUNK, MAX_UNITS, MAX_TAPS = 1024, 1024, 128  # include/nplda_hip.h NPLDA_RESAMPLE_*

UTT_DTYPE = np.dtype([("in_off", "<i8"), ("out_off", "<i8"), ("n", "<i4"), ("m", "<i4"), ("ratio", "<i4"), ("gain", "<f4")])
RATIO_DTYPE = np.dtype([("iu", "<i4"), ("ou", "<i4"), ("taps", "<i4"), ("reserved", "<i4"), ("first_off", "<i8"),
                        ("weight_off", "<i8")])
assert UTT_DTYPE.itemsize == 32 and RATIO_DTYPE.itemsize == 32


class _Call(ctypes.Structure):  # nplda_resample_call of include/nplda_hip.h
    _fields_ = [(k, ctypes.c_void_p) for k in ("samples", "utts", "ratios", "first", "weights", "chunks", "out", "clipped")] + \
               [(k, ctypes.c_int64) for k in ("n_utts", "n_ratios", "total_chunks")] + \
               [(k, ctypes.c_int32) for k in ("max_iu", "max_ou", "max_taps", "max_span", "out_i16", "reserved")]


def _rate(r, what="rate"):
    if isinstance(r, (float, np.floating)) and float(r) != int(r):
        raise ValueError(f"{what} {r}: expected a positive integer")
    v = int(r)
    if v <= 0:
        raise ValueError(f"{what} {r}: expected a positive integer")
    return v


def units(rate_in, rate_out):
    """(iu, ou) = (rate_in, rate_out) / gcd."""
    rin, rout = _rate(rate_in, "rate_in"), _rate(rate_out, "rate_out")
    g = math.gcd(rin, rout)
    return rin // g, rout // g


def filter_bank(rate_in, rate_out, width=6, rolloff=0.99):
    """(iu, ou, first (ou,) int64, weights (ou, taps) float64): output k = b ou + p reads the inputs b iu + first[p] + t,
    t < taps, with weights[p, t]; a phase with fewer than `taps` weights has zeros at its end."""
    iu, ou = units(rate_in, rate_out)
    rin, rout = int(rate_in), int(rate_out)
    if not (width > 0 and 0 < rolloff <= 1):
        raise ValueError(f"width {width}, rolloff {rolloff}: expected width > 0 and 0 < rolloff <= 1")
    T = rin * ou
    fc = rolloff * min(rin, rout) / 2.0
    ww = width / (2.0 * fc)
    half = int(math.floor(ww * T / ou)) + 2
    p = np.arange(ou, dtype=np.int64)[:, None]
    i = (p * iu) // ou + np.arange(-half, half + 1, dtype=np.int64)[None, :]
    inside = np.abs(i * ou - p * iu) / T < ww
    counts = inside.sum(axis=1)
    first = i[np.arange(ou), np.argmax(inside, axis=1)]
    taps = int(counts.max())
    idx = first[:, None] + np.arange(taps, dtype=np.int64)[None, :]
    q = idx * ou - p * iu
    valid = np.abs(q) / T < ww
    assert (valid.sum(axis=1) == counts).all(), "the support of a phase is one run of inputs"
    assert (np.diff(first) >= 0).all() and first[-1] <= first[0] + iu, "the first input does not decrease with the output"
    t = q / float(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(q == 0, 2.0 * fc, np.sin(2.0 * np.pi * fc * t) / (np.pi * t))
    h = s * 0.5 * (1.0 + np.cos(2.0 * np.pi * fc * t / width))
    return iu, ou, first, np.where(valid, h / rin, 0.0)


def _per_utt(v, U, dtype, what):
    a = np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v)
    if a.ndim > 1 or (a.ndim == 1 and U is not None and a.shape[0] != U):
        raise ValueError(f"{what}: expected a scalar or one value per utterance")
    return np.broadcast_to(a, (U,)).astype(dtype) if U is not None else a.astype(dtype)


def _rates(rate, U, what):
    a = _per_utt(rate, U, np.float64, what)
    for u, r in enumerate(a.reshape(-1)):
        if not (np.isfinite(r) and r > 0 and r == int(r)):
            raise ValueError(f"utterance {u}: {what} {r}, expected a positive integer")
    return a.astype(np.int64)


def output_lengths(lengths, rate_in, rate_out):
    """Samples out per utterance, ceil(n rate_out / rate_in): host arithmetic (rates: scalars or one per utterance)."""
    n = np.asarray(lengths, dtype=np.int64)
    rin, rout = _rates(rate_in, None, "rate_in"), _rates(rate_out, None, "rate_out")
    g = np.gcd(rin, rout)
    iu, ou = rin // g, rout // g
    return -(-(n * ou) // iu)


def speed_rates(factors, sample_frequency, U=None):
    """rate_in = round(f sample_frequency) per speed factor f (torchaudio's SpeedPerturbation): resampling from it to
    sample_frequency and playing the result at sample_frequency is the utterance f times as fast."""
    sr = _rate(sample_frequency, "sample_frequency")
    f = _per_utt(factors, U, np.float64, "factors")
    for u, v in enumerate(f.reshape(-1)):
        if not (np.isfinite(v) and v > 0 and round(v * sr) >= 1):
            raise ValueError(f"utterance {u}: speed factor {v}")
    return np.rint(f * sr).astype(np.int64)


# ---- the banks of a call on a device -----------------------------------------------------------------------------------------

_BANKS = {}    # (rin, rout, width, rolloff) -> (iu, ou, taps padded to a multiple of 4, first int32, weights float32
               #                                  [tap][phase] with zero rows at the end, taps)
_TABLES = {}   # (the keys of a call, device index) -> the device arrays


def _bank(key):
    got = _BANKS.get(key)
    if got is None:
        iu, ou, first, w = filter_bank(*key)
        taps = w.shape[1]
        wt = np.zeros((-(-taps // 4) * 4, ou), dtype=np.float32)
        wt[:taps] = w.T.astype(np.float32)
        got = _BANKS[key] = (iu, ou, wt.shape[0], first.astype(np.int32), wt, taps)
    return got


def _tables(keys, dev):
    got = _TABLES.get((keys, dev.index))
    if got is None:
        lib = _lib.load()
        banks = [_bank(k) for k in keys]
        ratios = np.zeros(len(keys), dtype=RATIO_DTYPE)
        fo = wo = 0
        for r, (iu, ou, taps, first, w, _) in enumerate(banks):
            ratios[r] = (iu, ou, taps, 0, fo, wo)
            fo, wo = fo + ou, wo + ou * taps
        spans = [int(lib.nplda_resample_span_floats(b[0], b[1], b[2])) for b in banks]
        host = dict(max_iu=max(b[0] for b in banks), max_ou=max(b[1] for b in banks), max_taps=max(b[2] for b in banks),
                    max_span=max(spans))
        with _lib.on_device(dev):
            d = [torch.from_numpy(a).to(dev) for a in (ratios.view(np.uint8), np.concatenate([b[3] for b in banks]),
                                                       np.concatenate([b[4].reshape(-1) for b in banks]))]
        if len(_TABLES) >= 64:
            _TABLES.clear()
        got = _TABLES[(keys, dev.index)] = (d, host)
    return got


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the resampler runs on a HIP device, not on {dev}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


class Prepared:
    """prepare()'s result: `samples`, `offsets`, `clipped` as resample returns them, filled by every `launch()`, which
    enqueues one nplda_resample_batch call on the current stream and touches nothing on the host: it can be captured in a
    graph and replayed."""

    def __init__(self, call, keep, samples, offsets, clipped, device):
        self.call, self.keep, self.samples, self.offsets, self.clipped, self.device = call, keep, samples, offsets, clipped, device
        self.lib = _lib.load()

    def launch(self):
        with _lib.on_device(self.device):
            _lib.check(self.lib.nplda_resample_batch(ctypes.addressof(self.call), _lib.current_stream(self.device)),
                       "nplda_resample_batch")
        return self.samples, self.offsets, self.clipped


def check_ratio(rin, rout, width=6, rolloff=0.99, who="ratio"):
    """ValueError for a pair of rates beyond the kernel's limits (host arithmetic; equal rates always pass)."""
    if rin == rout:
        return
    iu, ou = units(rin, rout)
    if iu > MAX_UNITS or ou > MAX_UNITS:
        raise ValueError(f"{who}: {rin} -> {rout} is {iu}:{ou} in lowest terms, at most {MAX_UNITS}:{MAX_UNITS} is supported")
    taps = _bank((int(rin), int(rout), width, rolloff))[5]
    if taps > MAX_TAPS:
        raise ValueError(f"{who}: {rin} -> {rout} takes {taps} taps, at most {MAX_TAPS} are supported")


def prepare(samples, offsets, rate_in, rate_out, gain=1.0, out_dtype=torch.int16, device=None, width=6, rolloff=0.99):
    """Everything of resample() that touches the host — checks, output lengths, filter banks (cached per (rate_in,
    rate_out, width, rolloff) and device), index arrays and the output allocation — done once; the result's launch() only
    enqueues (the same count for the same shapes)."""
    if out_dtype not in (torch.int16, torch.float32):
        raise ValueError("out_dtype: torch.int16 or torch.float32")
    if torch.is_tensor(offsets):
        offsets = offsets.cpu().numpy()
    offs = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
    if torch.is_tensor(samples):
        if samples.dtype != torch.int16 or samples.dim() != 1 or not samples.is_contiguous():
            raise ValueError("samples: expected a contiguous one-dimensional int16 tensor")
    else:
        samples = np.asarray(samples)
        if samples.dtype != np.int16 or samples.ndim != 1:
            raise ValueError("samples: expected a one-dimensional int16 array (the values as they are, not scaled)")
    U = offs.shape[0] - 1
    if U < 0 or offs[0] < 0 or offs[-1] > int(samples.shape[0]) or (np.diff(offs) < 0).any():
        raise ValueError("offsets: expected U + 1 non-decreasing sample offsets inside the samples")
    n = np.diff(offs)
    rin, rout = _rates(rate_in, U, "rate_in"), _rates(rate_out, U, "rate_out")
    gains = _per_utt(gain, U, np.float32, "gain")
    keys, ratio = [], np.full(U, -1, dtype=np.int64)
    for u in range(U):
        if not np.isfinite(gains[u]):
            raise ValueError(f"utterance {u}: gain {gains[u]}")
        if rin[u] == rout[u]:
            continue
        check_ratio(int(rin[u]), int(rout[u]), width, rolloff, f"utterance {u}")
        key = (int(rin[u]), int(rout[u]), width, rolloff)
        if key not in keys:
            keys.append(key)
        ratio[u] = keys.index(key)
    m = output_lengths(n, rin, rout) if U else np.zeros(0, np.int64)
    for u in range(U):
        if max(int(n[u]), int(m[u])) > np.iinfo(np.int32).max - CHUNK:
            raise ValueError(f"utterance {u}: {int(n[u])} samples in, {int(m[u])} out are beyond the int32 indexing")
    out_offs = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    lib = _lib.load()
    total_chunks = int(lib.nplda_resample_chunk_table(out_offs.ctypes.data, U, None, 0))
    if total_chunks < 0:
        _lib.check(total_chunks, "nplda_resample_chunk_table")
    chunks = np.zeros((max(total_chunks, 1), 2), dtype=np.int32)
    got = int(lib.nplda_resample_chunk_table(out_offs.ctypes.data, U, chunks.ctypes.data, total_chunks))
    assert got == total_chunks, (got, total_chunks)
    utts = np.zeros(U, dtype=UTT_DTYPE)
    utts["in_off"], utts["out_off"], utts["n"], utts["m"], utts["ratio"], utts["gain"] = offs[:-1], out_offs[:-1], n, m, ratio, gains

    dev = _device(samples.device if torch.is_tensor(samples) and samples.is_cuda and device is None else device)
    with _lib.on_device(dev):
        d_samples = samples.to(dev) if torch.is_tensor(samples) else torch.from_numpy(np.ascontiguousarray(samples)).to(dev)
        if d_samples.data_ptr() % 16:
            d_samples = d_samples.clone()
        out = torch.empty(int(out_offs[-1]), dtype=out_dtype, device=dev)
        clipped = torch.zeros(U, dtype=torch.int32, device=dev)
        d_utts = torch.from_numpy(utts.view(np.uint8)).to(dev)
        d_chunks = torch.from_numpy(chunks.reshape(-1)).to(dev)
    c = _Call()
    c.samples, c.utts, c.chunks, c.out, c.clipped = (t.data_ptr() for t in (d_samples, d_utts, d_chunks, out, clipped))
    keep = [d_samples, d_utts, d_chunks, out, clipped]
    if keys:
        d, host = _tables(tuple(keys), dev)
        c.ratios, c.first, c.weights = (t.data_ptr() for t in d)
        c.max_iu, c.max_ou, c.max_taps, c.max_span = host["max_iu"], host["max_ou"], host["max_taps"], host["max_span"]
        keep.append(d)
    c.n_utts, c.n_ratios, c.total_chunks, c.out_i16 = U, len(keys), total_chunks, int(out_dtype == torch.int16)
    return Prepared(c, keep, out, out_offs, clipped, dev)


def resample(samples, offsets, rate_in, rate_out, gain=1.0, out_dtype=torch.int16, device=None, width=6, rolloff=0.99):
    """samples: int16 tensor or array holding every utterance; offsets: U + 1 sample offsets on the HOST; rate_in, rate_out,
    gain: scalars or (U,) arrays -> (samples' on the device in out_dtype (torch.int16 or torch.float32), offsets' int64 on
    the host, clipped (U,) int32 on the device: the samples that saturated, zero for float output).  Utterances of different
    ratios, copies (equal rates) and empty ones go in one launch.  The output lengths are host arithmetic: nothing is read
    back.  Argument errors are ValueErrors naming the utterance."""
    return prepare(samples, offsets, rate_in, rate_out, gain, out_dtype, device, width, rolloff).launch()


def speed_perturb(samples, offsets, factors, sample_frequency, gain=1.0, out_dtype=torch.int16, device=None, width=6,
                  rolloff=0.99):
    """resample() from round(f sample_frequency) to sample_frequency per speed factor f (a scalar or one per utterance):
    played at sample_frequency the result is f times as fast, 1 / f as long and shifted in pitch, as sox's `speed` of
    utils/perturb_data_dir_speed.sh and torchaudio's SpeedPerturbation."""
    U = len(offsets) - 1
    return resample(samples, offsets, speed_rates(factors, sample_frequency, U), _rate(sample_frequency, "sample_frequency"),
                    gain, out_dtype, device, width, rolloff)
