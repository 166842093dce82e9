"""Augmentation of 16-bit audio on the HIP device (csrc/nplda_augment.hip): reverberation with room impulse responses and
additive noise, music and babble at drawn SNRs — the step of the Kaldi x-vector recipes (`wav-reverberate`) between the wave
files and the MFCCs.

    keys, offsets, samples = kaldi_format.load_wav_scp("data/train/wav.scp", sample_frequency=16000)
    rirs, noises = RirTable(rir_paths, 16000), NoiseTable(noise_paths, 16000, labels=noise_labels)
    aug = Augmenter(rirs, noises, seed=0)
    recipe = aug.draw(np.diff(offsets))
    samples2, offsets2, clipped = augment(samples, offsets, recipe, rirs, noises)     # int16 on the device
    frames, lengths = mfcc.compute_mfcc(samples2, offsets2, opts)

The convolution is uniformly partitioned overlap-save (block 256, transform 512), both transforms exact fp32 MFMA products
against constant tables; every scalar of an utterance comes from float64 sums in a fixed order, and the element-wise path is
plain float32 arithmetic in list order.  Nothing is read back, two calls give the same bits, and an utterance's result does
not depend on the batch.  design/k28_augment.md holds the specification.
"""
import ctypes

import numpy as np
import torch

from . import _lib, kaldi_format, resample as _resample

__all__ = ["RirTable", "NoiseTable", "Recipe", "Augmenter", "augment", "prepare", "output_lengths", "perturbed_lengths",
           "workspace_bytes", "BLOCK", "MAX_RIR"]

BLOCK, TILE, GROUP, CHUNK, MAX_RIR = 256, 32, 8, 2048, 32768  # include/nplda_hip.h NPLDA_AUGMENT_*
PSIZE = 2 * BLOCK

UTT_DTYPE = np.dtype([("in_off", "<i8"), ("out_off", "<i8"), ("y_off", "<i8"), ("n", "<i4"), ("n_out", "<i4"), ("shift", "<i4"),
                      ("rir", "<i4"), ("ent_begin", "<i4"), ("ent_count", "<i4"), ("n_early", "<i4"), ("normalize", "<i4"),
                      ("volume", "<f4"), ("reserved", "<i4")])
ENTRY_DTYPE = np.dtype([("noise_off", "<i8"), ("len", "<i4"), ("start", "<i4"), ("item", "<i4"), ("repeat", "<i4"),
                        ("ratio", "<f8")])
assert UTT_DTYPE.itemsize == 64 and ENTRY_DTYPE.itemsize == 32


class _Call(ctypes.Structure):  # nplda_augment_call of include/nplda_hip.h
    _fields_ = [(k, ctypes.c_void_p) for k in
                ("samples", "utts", "entries", "in_off", "in_len", "in_chunk_off", "out_chunk_off", "blk_off", "grp_off", "rir_of",
                 "early_len", "rir_spectra", "rir_parts", "noise", "noise_sums", "forward_table", "inverse_table", "out",
                 "clipped")] + \
               [(k, ctypes.c_int64) for k in ("n_utts", "n_entries", "total_blocks", "total_groups", "total_in_chunks",
                                              "total_out_chunks", "max_conv_len")] + \
               [("max_rir_len", ctypes.c_int32), ("out_i16", ctypes.c_int32)]


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the augmentation runs on a HIP device, not on {dev}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _cum(counts, dtype=np.int64):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(dtype)


def _ceil_div(a, b):
    return -(-np.asarray(a, dtype=np.int64) // b)


# ---- the two tables, float64 ---------------------------------------------------------------------------------------------

def forward_table():
    """(512, 512) float64: row o of the real DFT in the spectrum's layout ([0, 256) real parts, [256] Nyquist, [256 + k]
    imaginary part of bin k); angles from (o n) mod 512 in integers."""
    n = np.arange(PSIZE, dtype=np.int64)[None, :]
    k = (np.arange(PSIZE, dtype=np.int64) % BLOCK)[:, None]
    ang = 2.0 * np.pi * ((k * n) % PSIZE).astype(np.float64) / PSIZE
    F = np.where(np.arange(PSIZE)[:, None] < BLOCK, np.cos(ang), -np.sin(ang))
    F[BLOCK, :] = 1.0 - 2.0 * (np.arange(PSIZE) % 2)
    return F


def inverse_table():
    """(256, 512) float64: output sample 256 + t of the inverse transform, 1 / 512 and the factor 2 of the interior bins
    folded in."""
    t = (BLOCK + np.arange(BLOCK, dtype=np.int64))[:, None]
    k = (np.arange(PSIZE, dtype=np.int64) % BLOCK)[None, :]
    ang = 2.0 * np.pi * ((k * t) % PSIZE).astype(np.float64) / PSIZE
    G = np.where(np.arange(PSIZE)[None, :] < BLOCK, 2.0 * np.cos(ang), -2.0 * np.sin(ang)) / PSIZE
    G[:, 0] = 1.0 / PSIZE
    G[:, BLOCK] = (1.0 - 2.0 * (t[:, 0] % 2)) / PSIZE
    return G


def table_image(table):
    """[kb][wave][u][lane][i] = table[16 (NU wave + u) + (lane & 15)][16 kb + 4 (lane >> 4) + i], NU = rows / 64, float32."""
    rows, cols = table.shape
    NU, KB = rows // 64, cols // 16
    t32 = table.astype(np.float32)
    lane = np.arange(64)[None, None, None, :, None]
    r = 16 * (NU * np.arange(4)[None, :, None, None, None] + np.arange(NU)[None, None, :, None, None]) + (lane & 15)
    c = 16 * np.arange(KB)[:, None, None, None, None] + 4 * (lane >> 4) + np.arange(4)[None, None, None, None, :]
    return np.ascontiguousarray(t32[r, c])


class _Plan:
    """The two fragment images on one device (built once)."""
    _cache = {}

    def __init__(self, device):
        lib = _lib.load()
        images = [table_image(forward_table()), table_image(inverse_table())]
        for w, img in enumerate(images):
            assert img.nbytes == int(lib.nplda_augment_table_bytes(w)), (w, img.shape)
        self.forward, self.inverse = (torch.from_numpy(im.reshape(-1)).to(device) for im in images)

    @classmethod
    def get(cls, device):
        plan = cls._cache.get(device.index)
        if plan is None:
            plan = cls._cache[device.index] = cls(device)
        return plan


# ---- ragged tables -------------------------------------------------------------------------------------------------------

def _load_items(items, sample_frequency, what, resample=False, keep_dc=False):
    """The items as arrays.  resample: wave files at another rate are brought to sample_frequency on the device, all in one
    call: int16 again, or (keep_dc) float32 times rate / sample_frequency, so that the sum of the taps stays what it was."""
    out, other = [], []
    for i, it in enumerate(items):
        if isinstance(it, (str, bytes)) or hasattr(it, "__fspath__"):
            rate, x = kaldi_format.read_wav(it)
            if rate != int(sample_frequency):
                if not resample:
                    raise ValueError(f"{what} {i} ({it}): sample rate {rate}, expected {int(sample_frequency)}")
                _resample.check_ratio(rate, int(sample_frequency), who=f"{what} {i} ({it})")
                other.append((i, rate))
            out.append(x)
        else:
            a = np.asarray(it)
            if a.ndim != 1:
                raise ValueError(f"{what} {i}: expected a one-dimensional array")
            out.append(a)
    if other:
        rates = np.array([r for _, r in other], dtype=np.int64)
        y, yo, _ = _resample.resample(np.concatenate([out[i] for i, _ in other]), _cum([len(out[i]) for i, _ in other]), rates,
                                      int(sample_frequency), gain=rates / float(int(sample_frequency)) if keep_dc else 1.0,
                                      out_dtype=torch.float32 if keep_dc else torch.int16)
        y = y.cpu().numpy()
        for k, (i, _) in enumerate(other):
            out[i] = y[yo[k]:yo[k + 1]]
    return out


def early_window(h, sample_frequency):
    """(peak, a, b): the first index of the largest value of h, and the window [a, b) of its early reverberation."""
    peak = int(np.argmax(h))
    sr = int(sample_frequency)
    return peak, max(0, peak - sr // 1000), min(len(h), peak + sr // 20)


class RirTable:
    """Room impulse responses: float32, ragged, each of 1 .. 32 768 taps; from arrays or 16-bit wave files (the counts as
    float32, unscaled).  The spectra of every response and of its early window are computed once per device.  resample: a
    wave file at another rate is resampled once, here, on the current device (neuralplda_amd.resample); the result stays
    float32 (it is not rounded back to 16 bits) and is scaled by rate / sample_frequency, so that the response keeps its DC
    gain — the sum of its taps — at the new rate.  Without it such a file is a ValueError."""

    def __init__(self, arrays_or_wav_paths, sample_frequency, resample=False):
        self.sample_frequency = float(sample_frequency)
        hs = [np.ascontiguousarray(a, dtype=np.float32)
              for a in _load_items(arrays_or_wav_paths, sample_frequency, "RIR", resample, keep_dc=True)]
        for r, h in enumerate(hs):
            if len(h) < 1:
                raise ValueError(f"RIR {r}: empty")
            if len(h) > MAX_RIR:
                raise ValueError(f"RIR {r}: {len(h)} taps, at most {MAX_RIR} are supported")
            if not np.isfinite(h).all():
                raise ValueError(f"RIR {r}: not finite")
        self.lengths = np.array([len(h) for h in hs], dtype=np.int64)
        self.offsets = _cum(self.lengths)
        self.taps = np.concatenate(hs) if hs else np.zeros(0, np.float32)
        win = [early_window(h, sample_frequency) for h in hs]
        self.peaks = np.array([w[0] for w in win], dtype=np.int64)
        self.early_begin = np.array([w[1] for w in win], dtype=np.int64)
        self.early_lengths = np.array([w[2] - w[1] for w in win], dtype=np.int64)
        R = len(hs)
        # the filters of the device table: every response, then every early window
        self._src_off = np.concatenate([self.offsets[:-1], self.offsets[:-1] + self.early_begin]).astype(np.int64)
        self._src_len = np.concatenate([self.lengths, self.early_lengths]).astype(np.int32)
        self._blk_off = _cum(_ceil_div(self._src_len, BLOCK), np.int32)
        nparts = np.diff(self._blk_off)
        self.parts = np.stack([self._blk_off[:R], nparts[:R], self._blk_off[R:2 * R], nparts[R:]], axis=1).astype(np.int32) \
            if R else np.zeros((0, 4), np.int32)
        self._dev = {}

    def __len__(self):
        return len(self.lengths)

    def spectra_bytes(self):
        return int(self._blk_off[-1]) * PSIZE * 4

    def on(self, device):
        """(spectra, parts) on `device`."""
        got = self._dev.get(device.index)
        if got is None:
            lib = _lib.load()
            plan = _Plan.get(device)
            with _lib.on_device(device):
                spectra = torch.empty(int(self._blk_off[-1]) * PSIZE, dtype=torch.float32, device=device)
                if len(self):
                    taps = torch.from_numpy(self.taps).to(device)
                    d = [torch.from_numpy(a).to(device) for a in (self._src_off, self._src_len, self._blk_off)]
                    _lib.check(lib.nplda_augment_spectra_f32(taps.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                             2 * len(self), int(self._blk_off[-1]), int(self._src_len.min()),
                                                             int(self._src_len.max()), plan.forward.data_ptr(),
                                                             spectra.data_ptr(), _lib.current_stream(device)),
                               "nplda_augment_spectra_f32")
                    torch.cuda.current_stream(device).synchronize()  # taps and index arrays may go now
                got = self._dev[device.index] = (spectra, torch.from_numpy(self.parts.reshape(-1)).to(device))
        return got


class NoiseTable:
    """Noise items: int16, ragged; from arrays or 16-bit wave files.  `labels`: one of "noise", "music", "babble" per item
    (what an Augmenter may use it for); None: every item serves every kind.  The items' exact sums of squares are computed
    once per device.  resample: a wave file at another rate is resampled once, here, on the current device
    (neuralplda_amd.resample) and rounded back to int16; without it such a file is a ValueError."""

    def __init__(self, arrays_or_wav_paths, sample_frequency, labels=None, resample=False):
        self.sample_frequency = float(sample_frequency)
        xs = _load_items(arrays_or_wav_paths, sample_frequency, "noise item", resample)
        for i, x in enumerate(xs):
            if x.dtype != np.int16:
                raise ValueError(f"noise item {i}: expected int16 samples (the values as they are, not scaled)")
        self.lengths = np.array([len(x) for x in xs], dtype=np.int64)
        if (self.lengths > np.iinfo(np.int32).max).any():
            raise ValueError("noise item: more than 2^31 - 1 samples")
        self.offsets = _cum(self.lengths)
        self.samples = np.concatenate(xs).astype(np.int16) if xs else np.zeros(0, np.int16)
        if labels is not None:
            labels = [str(s) for s in labels]
            if len(labels) != len(xs) or any(s not in ("noise", "music", "babble") for s in labels):
                raise ValueError('labels: one of "noise", "music", "babble" per noise item')
        self.labels = labels
        self._dev = {}

    def __len__(self):
        return len(self.lengths)

    def items_of(self, kind):
        if self.labels is None:
            return np.arange(len(self), dtype=np.int64)
        return np.array([i for i, s in enumerate(self.labels) if s == kind], dtype=np.int64)

    def on(self, device):
        """(samples, sums of squares int64) on `device`."""
        got = self._dev.get(device.index)
        if got is None:
            lib = _lib.load()
            with _lib.on_device(device):
                samples = torch.from_numpy(self.samples).to(device)
                sums = torch.zeros(max(len(self), 1), dtype=torch.int64, device=device)
                if len(self):
                    coff = _cum(_ceil_div(self.lengths, CHUNK), np.int32)
                    d_off, d_coff = torch.from_numpy(self.offsets).to(device), torch.from_numpy(coff).to(device)
                    _lib.check(lib.nplda_augment_power_i64(samples.data_ptr(), d_off.data_ptr(), d_coff.data_ptr(), len(self),
                                                           int(coff[-1]), sums.data_ptr(), _lib.current_stream(device)),
                               "nplda_augment_power_i64")
                    torch.cuda.current_stream(device).synchronize()
                got = self._dev[device.index] = (samples, sums)
        return got


# ---- recipes -------------------------------------------------------------------------------------------------------------

class Recipe:
    """What to do with each of U utterances, as plain arrays: rir (U,) int, -1 for none; additive: U lists of (noise item,
    start sample in the output, snr_db, repeat); shift_output, normalize_output (U,) bool, default true; volume (U,) float,
    default 0 (a positive value is the gain and switches normalisation off); speed (U,) float, default 1: the utterance is
    first made `speed` times as fast (resample.speed_perturb: 1 / speed as long, shifted in pitch), and everything else —
    the additive entries' start samples too — refers to the perturbed utterance."""

    def __init__(self, rir, additive=None, shift_output=True, normalize_output=True, volume=0.0, speed=1.0):
        self.rir = np.array(rir, dtype=np.int64).reshape(-1)
        U = len(self.rir)
        self.additive = [[] for _ in range(U)] if additive is None else [[tuple(e) for e in ent] for ent in additive]
        self.shift_output = np.broadcast_to(np.asarray(shift_output, dtype=bool), (U,)).copy()
        self.normalize_output = np.broadcast_to(np.asarray(normalize_output, dtype=bool), (U,)).copy()
        self.volume = np.broadcast_to(np.asarray(volume, dtype=np.float32), (U,)).copy()
        self.speed = np.broadcast_to(np.asarray(speed, dtype=np.float64), (U,)).copy()
        if len(self.additive) != U:
            raise ValueError(f"Recipe: {len(self.additive)} additive lists for {U} utterances")

    def __len__(self):
        return len(self.rir)

    @classmethod
    def clean(cls, U):
        """The recipe that changes nothing (no RIR, no noise, unit gain)."""
        return cls(np.full(int(U), -1), normalize_output=False)

    def select(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return Recipe(self.rir[idx], [self.additive[i] for i in idx], self.shift_output[idx], self.normalize_output[idx],
                      self.volume[idx], self.speed[idx])

    def at_unit_speed(self):
        """The same recipe for utterances that are already perturbed."""
        return Recipe(self.rir, self.additive, self.shift_output, self.normalize_output, self.volume)

    def validate(self, lengths, rirs, noises):
        """ValueError naming the utterance for an index outside its table or a malformed entry."""
        if len(lengths) != len(self):
            raise ValueError(f"recipe of {len(self)} utterances for {len(lengths)}")
        R, M = (0 if rirs is None else len(rirs)), (0 if noises is None else len(noises))
        for u in range(len(self)):
            r = int(self.rir[u])
            if r < -1 or r >= R:
                raise ValueError(f"utterance {u}: RIR {r} outside the table of {R}")
            if not np.isfinite(self.volume[u]):
                raise ValueError(f"utterance {u}: volume {self.volume[u]}")
            if not (np.isfinite(self.speed[u]) and self.speed[u] > 0):
                raise ValueError(f"utterance {u}: speed {self.speed[u]}")
            for e in self.additive[u]:
                if len(e) != 4:
                    raise ValueError(f"utterance {u}: an additive entry is (noise item, start, snr_db, repeat), got {e!r}")
                item, start, snr = int(e[0]), int(e[1]), float(e[2])
                if not 0 <= item < M:
                    raise ValueError(f"utterance {u}: noise item {item} outside the table of {M}")
                if start < 0 or start > np.iinfo(np.int32).max:
                    raise ValueError(f"utterance {u}: additive entry starting at sample {start}")
                if not np.isfinite(snr):
                    raise ValueError(f"utterance {u}: snr_db {snr}")


def _sample_frequency(sample_frequency, rirs, noises=None):
    for sr in (sample_frequency, getattr(rirs, "sample_frequency", None), getattr(noises, "sample_frequency", None)):
        if sr is not None:
            return int(sr)
    raise ValueError("a recipe with a speed other than 1 needs sample_frequency (or a table that carries it)")


def perturbed_lengths(lengths, recipe, sample_frequency):
    """Samples per utterance after the recipe's speed perturbation, ceil(n sr / round(speed sr)): host arithmetic."""
    n = np.asarray(lengths, dtype=np.int64)
    if (recipe.speed == 1.0).all():
        return n
    sr = int(sample_frequency)
    return _resample.output_lengths(n, _resample.speed_rates(recipe.speed, sr, len(recipe)), sr)


def _perturbed(lengths, recipe, rirs, sample_frequency):
    if (recipe.speed == 1.0).all():
        return np.asarray(lengths, dtype=np.int64), recipe
    return perturbed_lengths(lengths, recipe, _sample_frequency(sample_frequency, rirs)), recipe.at_unit_speed()


def output_lengths(lengths, recipe, rirs, sample_frequency=None):
    """Samples out per utterance: with n the length after the recipe's speed perturbation, n with shift_output or without
    a RIR, else n + L - 1 (host arithmetic)."""
    n, recipe = _perturbed(lengths, recipe, rirs, sample_frequency)
    has = (recipe.rir >= 0) & (n > 0)   # the convolution of no samples is no samples
    L = np.where(has, rirs.lengths[np.where(has, recipe.rir, 0)], 1) if has.any() else np.ones_like(n)
    return np.where(has & ~recipe.shift_output, n + L - 1, n)


def _layout(lengths, recipe, rirs, sample_frequency=None):
    """The host arithmetic of a call: counts of blocks, groups and chunks per utterance (of the perturbed lengths)."""
    n, recipe = _perturbed(lengths, recipe, rirs, sample_frequency)
    has = (recipe.rir >= 0) & (n > 0)
    ridx = np.where(has, recipe.rir, 0)
    L = np.where(has, rirs.lengths[ridx], 0) if has.any() else np.zeros_like(n)
    conv = np.where(has, n + L - 1, 0)
    blocks = _ceil_div(conv, BLOCK)
    return dict(n=n, has=has, ridx=ridx, L=L, conv=conv, blocks=blocks, groups=_ceil_div(blocks, GROUP),
                n_out=output_lengths(n, recipe, rirs) if has.any() else n.copy())


def workspace_bytes(lengths, recipe, rirs=None, sample_frequency=None):
    """Bytes of workspace of one call on these utterances (host arithmetic, nplda_augment_workspace_bytes; the speed
    perturbation in front of it takes none)."""
    lay = _layout(lengths, recipe, rirs, sample_frequency)
    E = sum(len(e) for e in recipe.additive)
    return int(_lib.load().nplda_augment_workspace_bytes(len(recipe), E, int(lay["blocks"].sum()),
                                                         int(_ceil_div(lay["n_out"], CHUNK).sum())))


def _pieces(lengths, recipe, rirs, limit):
    """Whole utterances in order, as many per piece as fit under `limit` bytes of workspace (at least one)."""
    U = len(recipe)
    if U == 0 or workspace_bytes(lengths, recipe, rirs) <= limit:
        return [(0, U)]
    lib = _lib.load()
    lay = _layout(lengths, recipe, rirs)
    cols = np.stack([np.ones(U, np.int64), np.array([len(e) for e in recipe.additive], dtype=np.int64), lay["blocks"],
                     _ceil_div(lay["n_out"], CHUNK)], axis=1)
    out, lo, acc = [], 0, np.zeros(4, np.int64)
    for u in range(U):
        if u > lo and int(lib.nplda_augment_workspace_bytes(*[int(v) for v in acc + cols[u]])) > limit:
            out.append((lo, u))
            lo, acc = u, np.zeros(4, np.int64)
        acc = acc + cols[u]
    out.append((lo, U))
    return out


class PreparedCall:
    """One nplda_augment_batch call with its index arrays and output on the device: `launch()` enqueues it on the current
    stream and touches nothing on the host, so it can be captured in a graph and replayed.  The workspace (`ws`, at least
    `ws_bytes`) is given by the owner before the first launch: the calls of one batch run in order on one stream and share
    one."""

    def __init__(self, d_samples, offs, recipe, rirs, noises, out, out_offs, clipped, dev):
        lib = _lib.load()
        U = len(recipe)
        lay = _layout(np.diff(offs), recipe, rirs)
        n, has, ridx = lay["n"], lay["has"], lay["ridx"]
        blk_off = _cum(lay["blocks"], np.int32)
        utts = np.zeros(U, dtype=UTT_DTYPE)
        utts["in_off"], utts["out_off"], utts["y_off"] = offs[:-1], out_offs[:-1], BLOCK * blk_off[:-1].astype(np.int64)
        utts["n"], utts["n_out"], utts["rir"] = n, lay["n_out"], np.where(has, recipe.rir, -1)
        if has.any():
            utts["shift"] = np.where(has & recipe.shift_output, rirs.peaks[ridx], 0)
            utts["n_early"] = np.where(has, n + rirs.early_lengths[ridx] - 1, 0)
        counts = np.array([len(e) for e in recipe.additive], dtype=np.int64)
        ent_off = _cum(counts)
        utts["ent_begin"], utts["ent_count"] = ent_off[:-1], counts
        utts["normalize"], utts["volume"] = recipe.normalize_output, recipe.volume
        E = int(ent_off[-1])
        entries = np.zeros(E, dtype=ENTRY_DTYPE)
        k = 0
        for ent in recipe.additive:
            for item, start, snr, repeat in ent:
                entries[k] = (noises.offsets[int(item)], noises.lengths[int(item)], int(start), int(item), int(bool(repeat)),
                              10.0 ** (-float(snr) / 10.0))
                k += 1
        in_chunk = _cum(_ceil_div(n, CHUNK), np.int32)
        out_chunk = _cum(_ceil_div(lay["n_out"], CHUNK), np.int32)
        grp_off = _cum(lay["groups"], np.int32)
        total_blocks = int(blk_off[-1])

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        d_utts = up(utts.view(np.uint8))
        d_entries = up(entries.view(np.uint8)) if E else None
        d_in_off, d_in_len = up(offs.astype(np.int64)), up(n.astype(np.int32))
        d_in_chunk, d_out_chunk, d_blk, d_grp = up(in_chunk), up(out_chunk), up(blk_off), up(grp_off)
        d_rir_of, d_early = up(utts["rir"].astype(np.int32)), up(utts["n_early"].astype(np.int32))
        c = _Call()
        c.samples, c.utts, c.entries = d_samples.data_ptr(), d_utts.data_ptr(), _lib.ptr(d_entries)
        c.in_off, c.in_len, c.in_chunk_off, c.out_chunk_off = (t.data_ptr() for t in (d_in_off, d_in_len, d_in_chunk,
                                                                                      d_out_chunk))
        c.blk_off, c.grp_off, c.rir_of, c.early_len = (t.data_ptr() for t in (d_blk, d_grp, d_rir_of, d_early))
        self.keep = [d_samples, d_utts, d_entries, d_in_off, d_in_len, d_in_chunk, d_out_chunk, d_blk, d_grp, d_rir_of, d_early,
                     out, clipped]
        if total_blocks:
            plan = _Plan.get(dev)
            spectra, parts = rirs.on(dev)
            c.rir_spectra, c.rir_parts = spectra.data_ptr(), parts.data_ptr()
            c.forward_table, c.inverse_table = plan.forward.data_ptr(), plan.inverse.data_ptr()
            self.keep += [spectra, parts, plan]
        if E:
            d_noise, d_sums = noises.on(dev)
            c.noise, c.noise_sums = d_noise.data_ptr(), d_sums.data_ptr()
            self.keep += [d_noise, d_sums]
        c.out, c.clipped = out.data_ptr(), clipped.data_ptr()
        c.n_utts, c.n_entries, c.total_blocks, c.total_groups = U, E, total_blocks, int(grp_off[-1])
        c.total_in_chunks, c.total_out_chunks = int(in_chunk[-1]), int(out_chunk[-1])
        c.max_conv_len = int(lay["conv"].max()) if U else 0
        c.max_rir_len = int(lay["L"].max()) if U else 0
        c.out_i16 = int(out.dtype == torch.int16)
        self.ws_bytes = int(lib.nplda_augment_workspace_bytes(U, E, total_blocks, c.total_out_chunks))
        self.ws = None
        self.call, self.device, self.lib = c, dev, lib

    def launch(self):
        _lib.check(self.lib.nplda_augment_batch(ctypes.addressof(self.call), self.ws.data_ptr(), self.ws_bytes,
                                                _lib.current_stream(self.device)), "nplda_augment_batch")


class Prepared:
    """prepare()'s result: `samples`, `offsets`, `clipped` as augment returns them, filled by every `launch()`.  The calls
    (one per piece of the batch) run one after the other on the current stream and share ONE workspace of the largest
    piece's size, `workspace_bytes`: that, not the sum over the pieces, is what the batch holds on the device."""

    def __init__(self, calls, samples, offsets, clipped, device, speed=None):
        self.calls, self.samples, self.offsets, self.clipped, self.device = calls, samples, offsets, clipped, device
        self.speed = speed   # the resample.Prepared of the speed perturbation in front of the calls, or None
        self.workspace_bytes = max([c.ws_bytes for c in calls], default=0)
        self.workspace = torch.empty(max(self.workspace_bytes, 256), dtype=torch.uint8, device=device)
        for c in calls:
            c.ws = self.workspace

    def launch(self):
        with _lib.on_device(self.device):
            if self.speed is not None:
                self.speed.launch()
            for c in self.calls:
                c.launch()
        return self.samples, self.offsets, self.clipped


def prepare(samples, offsets, recipe, rirs=None, noises=None, out_dtype=torch.int16, device=None, workspace_limit=None,
            sample_frequency=None):
    """Everything of augment() that touches the host — checks, output lengths, index arrays, workspace and output
    allocation, the tables' device copies — done once; the result's launch() only enqueues kernels (the same count for the
    same shapes), so it can be captured in a graph.  With a speed other than 1 in the recipe, one resample launch (16-bit,
    unit gain) goes in front of the pieces, which then work on the perturbed utterances."""
    if out_dtype not in (torch.int16, torch.float32):
        raise ValueError("out_dtype: torch.int16 or torch.float32")
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
    U = offs.shape[0] - 1
    if U < 0 or offs[0] < 0 or offs[-1] > int(samples.shape[0]) or (np.diff(offs) < 0).any():
        raise ValueError("offsets: expected U + 1 non-decreasing sample offsets inside the samples")
    lengths = np.diff(offs)
    recipe.validate(lengths, rirs, noises)
    speed = None
    if (recipe.speed != 1.0).any():
        sr = _sample_frequency(sample_frequency, rirs, noises)
        speed = _resample.prepare(samples, offs, _resample.speed_rates(recipe.speed, sr, U), sr, device=dev)
        samples, offs, recipe = speed.samples, speed.offsets, recipe.at_unit_speed()
        lengths = np.diff(offs)
    lay = _layout(lengths, recipe, rirs)
    for u in range(U):
        if max(int(lay["conv"][u]), int(lengths[u])) > np.iinfo(np.int32).max - PSIZE:
            raise ValueError(f"utterance {u}: {int(lengths[u])} samples are beyond the int32 block indexing")
    out_offs = _cum(lay["n_out"])
    if workspace_limit is None:
        from . import xvector
        workspace_limit = xvector.MAX_WORKSPACE_BYTES
    with _lib.on_device(dev):
        d_samples = samples.to(dev) if torch.is_tensor(samples) else torch.from_numpy(np.ascontiguousarray(samples)).to(dev)
        out = torch.empty(int(out_offs[-1]), dtype=out_dtype, device=dev)
        clipped = torch.zeros(U, dtype=torch.int32, device=dev)
        calls = [PreparedCall(d_samples, offs[lo:hi + 1], recipe.select(np.arange(lo, hi)), rirs, noises, out,
                              out_offs[lo:hi + 1], clipped[lo:hi], dev)
                 for lo, hi in _pieces(lengths, recipe, rirs, int(workspace_limit)) if hi > lo]
        return Prepared(calls, out, out_offs, clipped, dev, speed)


def augment(samples, offsets, recipe, rirs=None, noises=None, out_dtype=torch.int16, device=None, workspace_limit=None,
            sample_frequency=None):
    """samples: int16 tensor or array holding every utterance; offsets: U + 1 sample offsets on the HOST; recipe: a Recipe of U
    utterances -> (samples' on the device in out_dtype (torch.int16 or torch.float32), offsets' int64 on the host, clipped
    (U,) int32 on the device: the samples that saturated, zero for float output).  The output lengths are host arithmetic:
    nothing is read back.  A batch whose workspace would exceed workspace_limit (default xvector.MAX_WORKSPACE_BYTES) is split
    by whole utterances; the split does not change a bit.  Argument errors are ValueErrors naming the utterance.  A recipe
    with speeds other than 1 resamples those utterances first (sample_frequency: that of the audio; default: the tables')."""
    return prepare(samples, offsets, recipe, rirs, noises, out_dtype, device, workspace_limit, sample_frequency).launch()


# ---- drawing recipes -----------------------------------------------------------------------------------------------------

KINDS = ("clean", "reverb", "noise", "music", "babble")
SNRS = {"noise": (15.0, 10.0, 5.0, 0.0), "music": (15.0, 10.0, 8.0, 5.0), "babble": (20.0, 17.0, 15.0, 13.0)}
BABBLE_SPEAKERS = (3, 7)   # inclusive
NOISE_GAP_SECONDS = 1.0


class Augmenter:
    """Draws recipes on the host from numpy.random.Generator(PCG64(seed)), with the kinds of the Kaldi voxceleb recipe; a
    seed repeats a run.  design/k28_augment.md states the draw step by step.  Per utterance, in order:
      with speeds (a tuple such as (0.9, 1.0, 1.1)): speed = speeds[integers(len(speeds))], and n becomes the perturbed
              length ceil(n sr / round(speed sr)); with speeds=None nothing is drawn here and the recipes are those of an
              Augmenter without the argument
      kind = kinds[integers(len(kinds))]
      clean:  nothing
      reverb: rir = integers(number of RIRs)
      noise:  t = 0; while t < n: item = noise items[integers(count)], snr = (15, 10, 5, 0)[integers(4)], entry
              (item, t, snr, no repeat), t += the item's length + one second
      music:  item = music items[integers(count)], snr = (15, 10, 8, 5)[integers(4)], entry (item, 0, snr, repeat)
      babble: k = integers(3, 8); k times: item = babble items[integers(count)], snr = (20, 17, 15, 13)[integers(4)],
              entry (item, 0, snr, repeat)
    Every recipe has shift_output and normalize_output on and volume 0.  All draws of an utterance follow one another, so
    the recipes do not depend on how the utterances are cut into calls of draw()."""

    def __init__(self, rirs, noises, kinds=KINDS, seed=0, speeds=None, sample_frequency=None):
        kinds = tuple(kinds)
        if not kinds or any(k not in KINDS for k in kinds):
            raise ValueError(f"kinds: a non-empty choice of {KINDS}")
        if "reverb" in kinds and (rirs is None or len(rirs) == 0):
            raise ValueError("kind 'reverb' needs a RirTable")
        self.items = {}
        for k in ("noise", "music", "babble"):
            if k in kinds:
                self.items[k] = noises.items_of(k) if noises is not None else np.zeros(0, np.int64)
                if len(self.items[k]) == 0:
                    raise ValueError(f"kind {k!r} needs noise items labelled {k!r}")
                if k == "noise" and (noises.lengths[self.items[k]] == 0).any():
                    raise ValueError("kind 'noise': an empty foreground item")
        self.rirs, self.noises, self.kinds = rirs, noises, kinds
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.gap = int(NOISE_GAP_SECONDS * (noises.sample_frequency if noises is not None else 0))
        self.speeds = None if speeds is None else tuple(float(f) for f in speeds)
        self.sample_frequency = sample_frequency
        if self.speeds is not None:
            if not self.speeds:
                raise ValueError("speeds: a non-empty tuple of speed factors, or None")
            self.sample_frequency = sr = _sample_frequency(sample_frequency, rirs, noises)
            for f, rate in zip(self.speeds, _resample.speed_rates(self.speeds, sr)):
                _resample.check_ratio(int(rate), sr, who=f"speed {f}")

    def draw(self, lengths):
        """A Recipe for utterances of these lengths (the generator moves on: the next call draws the next recipes)."""
        rng = self.rng
        rir, additive, speed = [], [], []
        for n in np.asarray(lengths, dtype=np.int64).reshape(-1):
            if self.speeds is not None:
                speed.append(self.speeds[int(rng.integers(len(self.speeds)))])
                sr = self.sample_frequency
                n = int(_resample.output_lengths(n, _resample.speed_rates(speed[-1], sr), sr))
            kind = self.kinds[int(rng.integers(len(self.kinds)))]
            r, ent = -1, []
            if kind == "reverb":
                r = int(rng.integers(len(self.rirs)))
            elif kind == "noise":
                t = 0
                while t < n:
                    item = int(self.items[kind][int(rng.integers(len(self.items[kind])))])
                    snr = SNRS[kind][int(rng.integers(4))]
                    ent.append((item, t, snr, False))
                    t += int(self.noises.lengths[item]) + self.gap
            elif kind == "music":
                item = int(self.items[kind][int(rng.integers(len(self.items[kind])))])
                ent.append((item, 0, SNRS[kind][int(rng.integers(4))], True))
            elif kind == "babble":
                for _ in range(int(rng.integers(BABBLE_SPEAKERS[0], BABBLE_SPEAKERS[1] + 1))):
                    item = int(self.items[kind][int(rng.integers(len(self.items[kind])))])
                    ent.append((item, 0, SNRS[kind][int(rng.integers(4))], True))
            rir.append(r)
            additive.append(ent)
        return Recipe(rir, additive, speed=speed if self.speeds is not None else 1.0)

    def __call__(self, samples, offsets, out_dtype=torch.int16, device=None):
        """Draw a recipe for these utterances and apply it: augment(...)'s three results."""
        offs = np.asarray(offsets.cpu().numpy() if torch.is_tensor(offsets) else offsets, dtype=np.int64).ravel()
        return augment(samples, offs, self.draw(np.diff(offs)), self.rirs, self.noises, out_dtype, device,
                       sample_frequency=self.sample_frequency)
