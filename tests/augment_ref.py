"""The twin of the augmentation (design/k28_augment.md, csrc/nplda_augment.hip) in numpy — a plain helper of the tests.

    augment64   items 1 - 6 of the specification in float64 with np.convolve
    augment32   the same with the uniformly partitioned block convolution restated in float32 (block 256, transform 512,
                partitions summed in ascending order, the two tables rounded from float64 once) and the scalars and the
                element-wise path as the kernel computes them: the UNIT of the accuracy tests, and on the path without a RIR
                the kernel's result bit for bit
    draw        the Augmenter's draws, restated
"""
import numpy as np

B, P = 256, 512


def early_window(h, sr):
    """(peak, a, b): the first index of the largest VALUE of h (not of |h|), a = max(0, peak - floor(0.001 sr)),
    b = min(L, peak + floor(0.05 sr))."""
    h = np.asarray(h)
    peak = 0
    for i in range(1, len(h)):
        if h[i] > h[peak]:
            peak = i
    sr = int(sr)
    return peak, max(0, peak - sr // 1000), min(len(h), peak + sr // 20)


def output_length(n, L, shift_output):
    return n if (L is None or shift_output) else n + L - 1


# ---- the block convolution -------------------------------------------------------------------------------------------------

def tables(dtype):
    """(F (512, 512), G (256, 512)) in float64, rounded once to dtype.  A spectrum is 512 numbers: [0, 256) the real parts of
    bins 0 .. 255, [256] the Nyquist bin, [256 + k] the imaginary part of bin k = 1 .. 255."""
    F = np.zeros((P, P))
    G = np.zeros((B, P))
    n = np.arange(P)
    t = B + np.arange(B)
    for k in range(B):
        F[k] = np.cos(2 * np.pi * ((k * n) % P) / P)
        if k:
            F[B + k] = -np.sin(2 * np.pi * ((k * n) % P) / P)
            G[:, k] = 2 * np.cos(2 * np.pi * ((k * t) % P) / P) / P
            G[:, B + k] = -2 * np.sin(2 * np.pi * ((k * t) % P) / P) / P
    F[B] = np.where(n % 2 == 0, 1.0, -1.0)
    G[:, 0] = 1.0 / P
    G[:, B] = np.where(t % 2 == 0, 1.0, -1.0) / P
    return F.astype(dtype), G.astype(dtype)


_TABLES = {}


def _tables(dtype):
    key = np.dtype(dtype).name
    if key not in _TABLES:
        _TABLES[key] = tables(dtype)
    return _TABLES[key]


MIN_ROWS = 8


def _transform(rows, table):
    """rows @ table.T with the arithmetic of a matrix product whatever the number of rows: numpy hands a product of one or two
    rows to a BLAS dot-product routine whose float32 error is 2.7 times smaller (1.0e-7 against 2.8e-7 of the rms on 512-term
    sums) than that of the blocked product every larger case gets — the unit would then depend on how many blocks an
    utterance has, which the kernel's arithmetic does not.  Fewer than MIN_ROWS rows are padded with rows of zeros."""
    if rows.shape[0] >= MIN_ROWS:
        return rows @ table.T
    padded = np.zeros((MIN_ROWS, rows.shape[1]), rows.dtype)
    padded[:rows.shape[0]] = rows
    return (padded @ table.T)[:rows.shape[0]]


def block_convolve(x, h, dtype=np.float32):
    """x * h (n + L - 1 samples) by overlap-save in `dtype`: X_b the transform of samples [(b - 1) B, (b + 1) B), H_p of taps
    [p B, (p + 1) B) padded with B zeros, Y_b = sum_p X_{b-p} H_p in ascending p (separate multiplies and adds), block b of
    the result the last B samples of the inverse transform of Y_b."""
    x, h = np.asarray(x, dtype=dtype), np.asarray(h, dtype=dtype)
    n, L = len(x), len(h)
    if n == 0:
        return np.zeros(0, dtype)
    m = n + L - 1
    nb, npart = -(-m // B), -(-L // B)
    F, G = _tables(dtype)
    xp = np.zeros((nb + 1) * B, dtype)
    xp[B:B + n] = x
    frames = np.stack([xp[b * B:b * B + P] for b in range(nb)])
    X = _transform(frames, F)
    taps = np.zeros(npart * B, dtype)
    taps[:L] = h
    hp = np.zeros((npart, P), dtype)
    hp[:, :B] = taps.reshape(npart, B)
    H = _transform(hp, F)
    Y = np.zeros((nb, P), dtype)
    Yr, Yi = Y[:, :B], Y[:, B:]
    for p in range(min(npart, nb)):
        Xr, Xi = X[:nb - p, :B], X[:nb - p, B:]
        Hr, Hi = H[p, :B], H[p, B:]
        re = Xr * Hr - Xi * Hi
        im = Xr * Hi + Xi * Hr
        re[:, 0] = Xr[:, 0] * Hr[0]          # bin 0 and the Nyquist bin are real
        im[:, 0] = Xi[:, 0] * Hi[0]
        Yr[p:] += re
        Yi[p:] += im
    return _transform(Y, G).reshape(-1)[:m].astype(dtype)


# ---- items 1 - 6 -------------------------------------------------------------------------------------------------------------

def _isum(x):
    return int((np.asarray(x, dtype=np.int64) ** 2).sum())


def round_int16(v):
    """(int16 by round-half-to-even with saturation, the number of saturated samples)."""
    r = np.rint(v)
    clipped = int(((r > 32767) | (r < -32768)).sum())
    return np.clip(r, -32768, 32767).astype(np.int16), clipped


def augment64(x, h=None, additive=(), noises=(), shift_output=True, normalize_output=True, volume=0.0, sr=16000):
    """One utterance in float64 -> g * out (float64)."""
    x64 = np.asarray(x, dtype=np.float64)
    n = len(x64)
    p_in = _isum(x) / n if n else 0.0
    if h is not None:
        h64 = np.asarray(h, dtype=np.float64)
        peak, a, b = early_window(h64, sr)
        e = np.convolve(x64, h64[a:b]) if n else np.zeros(0)
        p_sig = float((e * e).mean()) if len(e) else 0.0
        y = np.convolve(x64, h64) if n else np.zeros(0)
        out = y[peak:peak + n].copy() if shift_output else y.copy()
    else:
        p_sig, out = p_in, x64.copy()
    for item, start, snr, repeat in additive:
        z = np.asarray(noises[item], dtype=np.float64)
        p_noise = _isum(noises[item]) / len(z) if len(z) else 0.0
        if p_noise == 0.0 or start >= len(out):
            continue
        s = np.sqrt(10.0 ** (-snr / 10.0) * p_sig / p_noise)
        t = np.arange(start, len(out) if repeat else min(len(out), start + len(z)))
        out[t] += s * z[(t - start) % len(z)]
    if volume > 0:
        g = float(volume)
    elif normalize_output:
        p_mix = float((out * out).mean()) if len(out) else 0.0
        g = np.sqrt(p_in / p_mix) if p_mix > 0 else 1.0
    else:
        g = 1.0
    return g * out


def augment32(x, h=None, additive=(), noises=(), shift_output=True, normalize_output=True, volume=0.0, sr=16000):
    """One utterance as the kernel computes it -> float32(g * out).  Every scalar is a float64 expression of float32-rounded
    powers, rounded once; the element-wise path is separate float32 multiplies and adds in list order."""
    f32, f64 = np.float32, np.float64
    x32 = np.asarray(x).astype(f32)
    n = len(x32)
    p_in = f32(f64(_isum(x)) / f64(n)) if n else f32(0)
    if h is not None:
        h32 = np.asarray(h, dtype=f32)
        peak, a, b = early_window(h32, sr)
        e = block_convolve(x32, h32[a:b], f32).astype(f64)
        p_sig = f32((e * e).sum() / f64(len(e))) if len(e) else f32(0)
        y = block_convolve(x32, h32, f32)
        out = y[peak:peak + n].copy() if shift_output else y.copy()
    else:
        p_sig, out = p_in, x32.copy()
    for item, start, snr, repeat in additive:
        z = np.asarray(noises[item])
        p_noise = f32(f64(_isum(z)) / f64(len(z))) if len(z) else f32(0)
        if not p_noise > 0:
            continue
        s = f32(np.sqrt(f64(10.0 ** (-float(snr) / 10.0)) * f64(p_sig) / f64(p_noise)))
        if s == 0 or start >= len(out):
            continue
        t = np.arange(start, len(out) if repeat else min(len(out), start + len(z)))
        out[t] = out[t] + s * z[(t - start) % len(z)].astype(f32)
    assert out.dtype == f32
    if volume > 0:
        g = f32(volume)
    elif normalize_output:
        m = out.astype(f64)
        p_mix = f32((m * m).sum() / f64(len(m))) if len(m) else f32(0)
        g = f32(np.sqrt(f64(p_in) / f64(p_mix))) if p_mix > 0 else f32(1)
    else:
        g = f32(1)
    return g * out


# ---- the Augmenter's draws -----------------------------------------------------------------------------------------------------

SNRS = {"noise": (15.0, 10.0, 5.0, 0.0), "music": (15.0, 10.0, 8.0, 5.0), "babble": (20.0, 17.0, 15.0, 13.0)}


def draw(seed, lengths, kinds, n_rirs, items, noise_lengths, sr):
    """[(rir, [(item, start, snr_db, repeat), ...])] per utterance; items: {kind: the noise items it may use}."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for n in lengths:
        kind = kinds[int(rng.integers(len(kinds)))]
        rir, ent = -1, []
        if kind == "reverb":
            rir = int(rng.integers(n_rirs))
        elif kind == "noise":
            t = 0
            while t < n:
                item = int(items[kind][int(rng.integers(len(items[kind])))])
                ent.append((item, t, SNRS[kind][int(rng.integers(4))], False))
                t += int(noise_lengths[item]) + int(sr)
        elif kind == "music":
            item = int(items[kind][int(rng.integers(len(items[kind])))])
            ent.append((item, 0, SNRS[kind][int(rng.integers(4))], True))
        elif kind == "babble":
            k = int(rng.integers(3, 8))
            for _ in range(k):
                item = int(items[kind][int(rng.integers(len(items[kind])))])
                ent.append((item, 0, SNRS[kind][int(rng.integers(4))], True))
        out.append((rir, ent))
    return out


# ---- test inputs ---------------------------------------------------------------------------------------------------------------

def make_rir(rng, L, peak, decay=0.004):
    """A unit peak at index `peak`, exponentially decaying Gaussian noise after it and a faint lead-in before it; every other
    tap stays below 0.9 so that the peak is the largest value."""
    t = np.arange(L, dtype=np.float64)
    h = 0.3 * rng.standard_normal(L) * np.exp(-decay * np.maximum(t - peak, 0.0))
    h[:peak] *= 0.1
    h = np.clip(h, -0.9, 0.9)
    h[peak] = 1.0
    return h.astype(np.float32)
