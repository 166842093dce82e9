"""Kaldi-compatible MFCCs from 16-bit audio on the HIP device (csrc/nplda_mfcc.hip): `compute-mfcc-feats --dither=0`.

    keys, offsets, samples = kaldi_format.load_wav_scp("data/test/wav.scp", sample_frequency=16000)
    opts = MfccOptions.from_conf("conf/mfcc.conf")
    frames, lengths = compute_mfcc(samples, offsets, opts)          # (sum T_u, num_ceps) float32 on the device

The samples go to the device as int16 (2 bytes each) and one launch computes every utterance of the call: framing with
reflected edges, DC removal, energy, pre-emphasis and window on the VALU, then the real DFT, the mel banks and the DCT as
three chained fp32 matrix products.  `XVectorNet_ETDNN_12Layer.extract_from_wav_scp` chains this with the energy VAD, the
sliding mean normalisation and the extractor.  design/k14_mfcc.md holds the specification.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["MfccOptions", "MfccPlan", "compute_mfcc", "num_frames", "FRAME_TILE"]

FRAME_TILE = 32  # include/nplda_hip.h NPLDA_MFCC_TILE: output frames per block
_WINDOWS = ("povey", "hamming", "hanning", "rectangular")
_REMOVE_DC, _USE_ENERGY, _RAW_ENERGY = 1, 2, 4  # NPLDA_MFCC_* flags


def _bool(s):
    v = str(s).strip().lower()
    if v in ("true", "t", "1"):
        return True
    if v in ("false", "f", "0"):
        return False
    raise ValueError(f"not a boolean: {s!r}")


_FIELDS = ("sample_frequency frame_length frame_shift low_freq high_freq num_mel_bins num_ceps use_energy raw_energy "
           "cepstral_lifter preemphasis_coefficient remove_dc_offset window_type snip_edges energy_floor dither")


class MfccOptions(collections.namedtuple("MfccOptions", _FIELDS)):
    """compute-mfcc-feats' options, with Kaldi's defaults except one: `dither` is 0 here (Kaldi: 1.0) and any other value
    raises ValueError — a random dither cannot be made bit-compatible, and the FLT_EPSILON floors under both logarithms
    make digital silence safe without it.  frame_length / frame_shift are milliseconds; high_freq <= 0 means Nyquist +
    high_freq.  Options this front end does not implement (--htk-compat, --vtln-*, --round-to-power-of-two=false,
    --allow-downsample, --subtract-mean, ...) are an error in from_conf."""
    __slots__ = ()
    _FLAGS = {"sample-frequency": ("sample_frequency", float), "frame-length": ("frame_length", float),
              "frame-shift": ("frame_shift", float), "low-freq": ("low_freq", float), "high-freq": ("high_freq", float),
              "num-mel-bins": ("num_mel_bins", int), "num-ceps": ("num_ceps", int), "use-energy": ("use_energy", _bool),
              "raw-energy": ("raw_energy", _bool), "cepstral-lifter": ("cepstral_lifter", float),
              "preemphasis-coefficient": ("preemphasis_coefficient", float), "remove-dc-offset": ("remove_dc_offset", _bool),
              "window-type": ("window_type", str), "snip-edges": ("snip_edges", _bool), "energy-floor": ("energy_floor", float),
              "dither": ("dither", float)}

    def __new__(cls, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, low_freq=20.0, high_freq=0.0,
                num_mel_bins=23, num_ceps=13, use_energy=True, raw_energy=True, cepstral_lifter=22.0,
                preemphasis_coefficient=0.97, remove_dc_offset=True, window_type="povey", snip_edges=True, energy_floor=0.0,
                dither=0.0):
        if float(dither) != 0.0:
            raise ValueError("MfccOptions: dither must be 0 (a random dither cannot be reproduced bit for bit)")
        if window_type not in _WINDOWS:
            raise ValueError(f"MfccOptions: window_type {window_type!r}, expected one of {_WINDOWS}")
        o = super(MfccOptions, cls).__new__(
            cls, float(sample_frequency), float(frame_length), float(frame_shift), float(low_freq), float(high_freq),
            int(num_mel_bins), int(num_ceps), bool(use_energy), bool(raw_energy), float(cepstral_lifter),
            float(preemphasis_coefficient), bool(remove_dc_offset), str(window_type), bool(snip_edges), float(energy_floor), 0.0)
        if o.num_mel_bins < 1 or not 1 <= o.num_ceps <= o.num_mel_bins:
            raise ValueError("MfccOptions: 1 <= num_ceps <= num_mel_bins")
        if o.frame_size < 2 or o.shift < 1 or o.energy_floor < 0.0 or not 0.0 <= o.preemphasis_coefficient <= 1.0:
            raise ValueError("MfccOptions: frame of >= 2 samples, shift of >= 1, energy_floor >= 0, 0 <= preemphasis <= 1")
        nyquist = 0.5 * o.sample_frequency
        if not (0.0 <= o.low_freq < o.high < nyquist + 1e-9):
            raise ValueError(f"MfccOptions: 0 <= low_freq < high_freq <= Nyquist, got {o.low_freq} and {o.high}")
        return o

    @property
    def frame_size(self):
        """N: samples per frame."""
        return int(self.sample_frequency * 0.001 * self.frame_length)

    @property
    def shift(self):
        """S: samples per frame shift."""
        return int(self.sample_frequency * 0.001 * self.frame_shift)

    @property
    def padded_size(self):
        """P: the smallest power of two >= N."""
        p = 1
        while p < self.frame_size:
            p *= 2
        return p

    @property
    def high(self):
        return self.high_freq if self.high_freq > 0.0 else 0.5 * self.sample_frequency + self.high_freq

    @classmethod
    def from_conf(cls, path):
        """A Kaldi option file: one `--name=value` per line, `#` comments.  Any option not in the table is an error."""
        kw = {}
        with open(path, "r") as fh:
            for n, ln in enumerate(fh, 1):
                ln = ln.split("#", 1)[0].strip()
                if not ln:
                    continue
                name, sep, val = ln.partition("=")
                name = name.strip().lstrip("-")
                if not sep or name not in cls._FLAGS:
                    raise ValueError(f"{path}:{n}: not an MFCC option this front end implements: {ln!r}")
                field, conv = cls._FLAGS[name]
                kw[field] = conv(val.strip())
        return cls(**kw)


def num_frames(n, options):
    """Frames of an utterance of n samples (int or integer array)."""
    n = np.asarray(n, dtype=np.int64)
    N, S = options.frame_size, options.shift
    if options.snip_edges:
        return np.where(n < N, 0, 1 + (n - N) // S)
    return (n + S // 2) // S


# ---- the tables, float64 ------------------------------------------------------------------------------------------------

def window_table(options):
    N = options.frame_size
    a = 2.0 * np.pi * np.arange(N, dtype=np.float64) / (N - 1)
    if options.window_type == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if options.window_type == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if options.window_type == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    return np.ones(N, dtype=np.float64)


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def bank_table(options):
    """(B, P / 2) triangular weights on the mel scale; the Nyquist bin is not used."""
    B, P = options.num_mel_bins, options.padded_size
    lo, hi = float(_mel(options.low_freq)), float(_mel(options.high))
    delta = (hi - lo) / (B + 1)
    m = _mel(np.arange(P // 2, dtype=np.float64) * options.sample_frequency / P)[None, :]
    left = (lo + delta * np.arange(B, dtype=np.float64))[:, None]
    centre, right = left + delta, left + 2.0 * delta
    up, down = (m - left) / (centre - left), (right - m) / (right - centre)
    return np.where((m > left) & (m <= centre), up, np.where((m > centre) & (m < right), down, 0.0))


def dct_table(options):
    """(C, B): the first C rows of the orthonormal DCT-II, each multiplied by its lifter coefficient."""
    B, C, L = options.num_mel_bins, options.num_ceps, options.cepstral_lifter
    c = np.arange(C, dtype=np.float64)[:, None]
    jj = np.arange(B, dtype=np.float64)[None, :]
    D = np.sqrt(2.0 / B) * np.cos(np.pi / B * (jj + 0.5) * c)
    D[0, :] = np.sqrt(1.0 / B)
    lift = 1.0 + 0.5 * L * np.sin(np.pi * c / L) if L != 0.0 else np.ones_like(c)
    return lift * D


class _Geometry(ctypes.Structure):  # nplda_mfcc_geometry of include/nplda_hip.h
    _fields_ = [("N", ctypes.c_int32), ("P", ctypes.c_int32), ("S", ctypes.c_int32), ("snip_edges", ctypes.c_int32),
                ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("flags", ctypes.c_int32), ("preemph", ctypes.c_float),
                ("energy_floor", ctypes.c_float)]


def geometry_of(options):
    flags = (_REMOVE_DC if options.remove_dc_offset else 0) | (_USE_ENERGY if options.use_energy else 0) | \
        (_RAW_ENERGY if options.raw_energy else 0)
    return _Geometry(options.frame_size, options.padded_size, options.shift, int(options.snip_edges), options.num_mel_bins,
                     options.num_ceps, flags, options.preemphasis_coefficient, options.energy_floor)


def _frag(mat, KB, XB):
    """The library's fragment order: out[kb][xb][lane][i] = mat[16 xb + (lane & 15)][16 kb + 4 (lane >> 4) + i], 0 outside."""
    full = np.zeros((16 * XB, 16 * KB), dtype=np.float32)
    full[:mat.shape[0], :mat.shape[1]] = mat
    lane = np.arange(64)
    rows = 16 * np.arange(XB)[None, :, None, None] + (lane & 15)[None, None, :, None]
    cols = 16 * np.arange(KB)[:, None, None, None] + (4 * (lane >> 4))[None, None, :, None] + np.arange(4)[None, None, None, :]
    return np.ascontiguousarray(full[rows, cols])


def dft_image(options):
    """[kb][wave][u][lane][i]: wave w owns bins [w P / 8, (w + 1) P / 8), NBW = P / 128 blocks of cosines, then of sines.
    Angles from (n bin) mod P in integers, float64 trigonometry, rounded once."""
    N, P = options.frame_size, options.padded_size
    KB, NBW = (N + 15) // 16, P // 128
    n = np.arange(16 * KB, dtype=np.int64)[:, None]
    k = np.arange(P // 2, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % P).astype(np.float64) / P
    valid = (n < N)
    table = np.stack([np.where(valid, np.cos(ang), 0.0), np.where(valid, np.sin(ang), 0.0)]).astype(np.float32)
    lane = np.arange(64)
    kb = np.arange(KB)[:, None, None, None, None]
    w = np.arange(4)[None, :, None, None, None]
    u = np.arange(2 * NBW)[None, None, :, None, None]
    ln = lane[None, None, None, :, None]
    i = np.arange(4)[None, None, None, None, :]
    rows = 16 * kb + 4 * (ln >> 4) + i
    bins = 16 * (w * NBW + u % NBW) + (ln & 15)
    return np.ascontiguousarray(table[u // NBW, rows, bins])


class MfccPlan:
    """The window and the three fragment images of one option set on one device (built once, cached by `get`)."""
    _cache = {}

    def __init__(self, options, device):
        lib = _lib.load()
        self.options, self.device = options, device
        self.geometry = geometry_of(options)
        gp = ctypes.byref(self.geometry)
        sizes = [int(lib.nplda_mfcc_image_bytes(gp, w)) for w in range(3)]
        if 0 in sizes:
            raise ValueError(f"MFCC geometry not supported by the kernel: frame of {options.frame_size} samples (<= 512, a "
                             f"multiple of 4), padded to {options.padded_size} (256 or 512), {options.num_mel_bins} mel bins "
                             "(<= 64)")
        MB = 2 if options.num_mel_bins <= 32 else 4
        images = [dft_image(options), _frag(bank_table(options), options.padded_size // 32, MB),
                  _frag(dct_table(options), MB, MB)]
        for img, nb in zip(images, sizes):
            assert img.dtype == np.float32 and img.nbytes == nb, (img.shape, nb)
        self.window = torch.from_numpy(window_table(options).astype(np.float32)).to(device)
        self.dft, self.bank, self.dct = (torch.from_numpy(im.reshape(-1)).to(device) for im in images)

    @classmethod
    def get(cls, options, device):
        key = (options, device.index)
        plan = cls._cache.get(key)
        if plan is None:
            plan = cls._cache[key] = cls(options, device)
        return plan


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the MFCC front end runs on a HIP device, not on {dev}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def compute_mfcc(samples, offsets, options=MfccOptions(), device=None):
    """samples: int16 tensor or array holding every utterance (on the host it is copied as int16, 2 bytes per sample);
    offsets: U + 1 sample offsets on the HOST -> (frames (sum T_u, num_ceps) float32 on the device, [T_u]).  The frame
    counts come from the offsets on the host, so there is no device synchronisation; one launch computes every utterance,
    whatever their lengths.  No utterances, or none with a frame, is a no-op."""
    if torch.is_tensor(offsets):
        offsets = offsets.cpu().numpy()
    offs = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
    if torch.is_tensor(samples):
        if samples.dtype != torch.int16 or samples.dim() != 1 or not samples.is_contiguous():
            raise ValueError("samples: expected a contiguous one-dimensional int16 tensor")
        dev = _device(samples.device if samples.is_cuda and device is None else device)
    else:
        samples = np.asarray(samples)
        if samples.dtype != np.int16 or samples.ndim != 1:
            raise ValueError("samples: expected a one-dimensional int16 array (the values as they are, not scaled)")
        dev = _device(device)
    total = int(samples.shape[0])
    U = offs.shape[0] - 1
    if U < 0 or offs[0] < 0 or offs[-1] > total or (np.diff(offs) < 0).any():
        raise ValueError("offsets: expected U + 1 non-decreasing sample offsets inside the samples")
    lengths = [int(t) for t in num_frames(np.diff(offs), options)]
    R = sum(lengths)
    C = options.num_ceps
    frames = torch.empty((R, C), dtype=torch.float32, device=dev)
    if R == 0:
        return frames, lengths
    plan = MfccPlan.get(options, dev)
    starts = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)
    lib = _lib.load()
    with _lib.on_device(dev):
        if torch.is_tensor(samples):
            d_samples = samples.to(dev)
        else:
            d_samples = torch.from_numpy(np.ascontiguousarray(samples)).to(dev)
        d_soff = torch.from_numpy(offs).to(dev)
        d_foff = torch.from_numpy(starts).to(dev)
        _lib.check(lib.nplda_mfcc_frames_f32(d_samples.data_ptr(), d_soff.data_ptr(), d_foff.data_ptr(), U, R,
                                             ctypes.addressof(plan.geometry), plan.window.data_ptr(), plan.dft.data_ptr(),
                                             plan.bank.data_ptr(), plan.dct.data_ptr(), frames.data_ptr(),
                                             _lib.current_stream(dev)), "nplda_mfcc_frames_f32")
    return frames, lengths
