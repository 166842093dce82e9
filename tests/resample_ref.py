"""The twin of the resampler (design/k29_resample.md, csrc/nplda_resample.hip) in numpy — a plain helper of the tests,
written from the specification:

    g = gcd(rin, rout), iu = rin / g, ou = rout / g, T = rin ou, fc = rolloff min(rin, rout) / 2, ww = width / (2 fc)
    m = ceil(n ou / iu);  y[k] = gain sum_i w(i ou - k iu) x[i] over |i ou - k iu| / T < ww,  x = 0 outside [0, n)
    w(q) = h(q / T) / rin,  h(t) = s(t) (1 + cos(2 pi fc t / width)) / 2,  s(t) = sin(2 pi fc t) / (pi t),  s(0) = 2 fc

    filter_bank     the ou phases: first input offset and weights per phase, float64
    output_length   m
    resample64      float64 sums on the float32-rounded table
    resample32      the same operations in numpy float32 (separate multiplies and adds, taps in increasing i): the UNIT of
                    the accuracy tests
    brute           the continuous formula per output sample in long double, no phase table
"""
import math

import numpy as np

CHUNK = 1024   # outputs per thread block of the kernel: the tile of the tests' regions

# (rate_in, rate_out): 9:10, 11:10, 2:1, 1:2, 441:160, 441:80 and, for the CPU tests, 3:1
RATES = ((14400, 16000), (17600, 16000), (16000, 8000), (8000, 16000), (44100, 16000), (44100, 8000))
ALL_RATES = RATES[:5] + ((48000, 16000),) + RATES[5:]
TAPS = {(14400, 16000): 13, (17600, 16000): 14, (16000, 8000): 25, (8000, 16000): 13, (44100, 16000): 34, (48000, 16000): 37,
        (44100, 8000): 67}


def units(rin, rout):
    g = math.gcd(int(rin), int(rout))
    return int(rin) // g, int(rout) // g


def output_length(n, rin, rout):
    iu, ou = units(rin, rout)
    return -(-(int(n) * ou) // iu)


def _h(q, rin, rout, T, width, rolloff):
    """w(q) for an array of tick distances, in q's floating type (float64 or long double)."""
    f = q.dtype.type
    fc = f(rolloff) * min(rin, rout) / 2
    pi = 4 * np.arctan(f(1))
    t = q / f(T)
    safe = np.where(t == 0, f(1), t)
    s = np.where(t == 0, 2 * fc, np.sin(2 * pi * fc * safe) / (pi * safe))
    return s * (1 + np.cos(2 * pi * fc * t / f(width))) / 2 / f(rin)


def filter_bank(rin, rout, width=6, rolloff=0.99):
    """(iu, ou, first (ou,), weights (ou, taps) float64, counts (ou,)): phase p = k mod ou of output k = b ou + p reads the
    inputs b iu + first[p] + t, t < counts[p]; weights beyond counts[p] are zero."""
    iu, ou = units(rin, rout)
    T = rin * ou
    ww = width / (2.0 * (rolloff * min(rin, rout) / 2.0))
    rows = []
    for p in range(ou):
        c = (p * iu) // ou
        r = int(ww * T / ou) + 3
        i = np.arange(c - r, c + r + 1, dtype=np.int64)
        q = i * ou - p * iu
        keep = np.abs(q) / T < ww
        assert keep.any() and not keep[0] and not keep[-1]
        rows.append((int(i[keep][0]), _h(q[keep].astype(np.float64), rin, rout, T, width, rolloff)))
    taps = max(len(w) for _, w in rows)
    weights = np.zeros((ou, taps))
    for p, (_, w) in enumerate(rows):
        weights[p, :len(w)] = w
    return iu, ou, np.array([f for f, _ in rows], dtype=np.int64), weights, np.array([len(w) for _, w in rows])


def _resample(x, rin, rout, gain, dtype, table32, width, rolloff):
    x = np.asarray(x)
    n = len(x)
    if n == 0:
        return np.zeros(0, dtype)
    if rin == rout:
        return (dtype(gain) * x.astype(dtype)).astype(dtype)
    iu, ou, first, w, _ = filter_bank(rin, rout, width, rolloff)
    if table32:
        w = w.astype(np.float32)
    w = w.astype(dtype)
    m = output_length(n, rin, rout)
    k = np.arange(m, dtype=np.int64)
    base = (k // ou) * iu + first[k % ou]
    xp = x.astype(dtype)
    acc = np.zeros(m, dtype)
    for t in range(w.shape[1]):
        i = base + t
        ok = (i >= 0) & (i < n)
        xi = np.where(ok, xp[np.clip(i, 0, n - 1)], dtype(0))
        prod = w[k % ou, t] * xi
        acc = acc + prod
        assert acc.dtype == dtype
    return (dtype(gain) * acc).astype(dtype)


def resample64(x, rin, rout, gain=1.0, width=6, rolloff=0.99, table32=True):
    """One utterance in float64 on the float32-rounded table (table32=False: on the float64 table)."""
    return _resample(x, rin, rout, gain, np.float64, table32, width, rolloff)


def resample32(x, rin, rout, gain=1.0, width=6, rolloff=0.99):
    """One utterance in float32: the float32 table, one chain of multiplies and adds per output, times float32(gain)."""
    return _resample(x, rin, rout, np.float32(gain), np.float32, True, width, rolloff)


def brute(x, rin, rout, width=6, rolloff=0.99):
    """y[k] from the continuous formula in long double, every input sample tried for every output: no phases, no table."""
    ld = np.longdouble
    x = np.asarray(x).astype(ld)
    n = len(x)
    iu, ou = units(rin, rout)
    T = rin * ou
    ww = ld(width) / (2 * (ld(rolloff) * min(rin, rout) / 2))
    m = output_length(n, rin, rout)
    y = np.zeros(m, ld)
    i = np.arange(n, dtype=np.int64)
    for k in range(m):
        q = i * ou - k * iu
        keep = np.abs(q).astype(ld) / T < ww
        y[k] = (_h(q[keep].astype(ld), rin, rout, T, width, ld(rolloff)) * x[keep]).sum()
    return y


def round_int16(v):
    """(int16 by round-half-to-even with saturation, the number of saturated samples)."""
    r = np.rint(v)
    clipped = int(((r > 32767) | (r < -32768)).sum())
    return np.clip(r, -32768, 32767).astype(np.int16), clipped


# ---- test inputs ---------------------------------------------------------------------------------------------------------------

def make_audio(rng, n, rate=16000.0, dc=2000.0, sigma=3000.0):
    """Gaussian noise of standard deviation 3000, two sinusoids and an offset of 2000, clipped to int16."""
    t = np.arange(n) / float(rate)
    x = rng.standard_normal(n) * sigma + dc
    for f, a in ((220.0, 4000.0), (1330.0, 2500.0)):
        x += a * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def grid_lengths(rin, rout):
    """1, 2, taps - 1, taps, one input sample less and one more than a chunk of outputs takes, 5000."""
    iu, ou = units(rin, rout)
    taps, c = TAPS[(rin, rout)], CHUNK * iu // ou
    return (1, 2, taps - 1, taps, c - 1, c + 1, 5000)


def grid_case():
    """[(x, rin, rout)]: every ratio of RATES with every length of grid_lengths, in one call."""
    rng = np.random.default_rng(29)
    return [(make_audio(rng, n, rin), rin, rout) for rin, rout in RATES for n in grid_lengths(rin, rout)]


def mixed_case():
    """[(x, rin, rout)]: each utterance another ratio, copies and empty utterances in between."""
    rng = np.random.default_rng(31)
    plan = [(3000, 14400, 16000), (0, 16000, 8000), (2500, 16000, 16000), (4100, 16000, 8000), (1, 8000, 8000),
            (1700, 8000, 16000), (0, 16000, 16000), (6000, 44100, 16000), (2047, 17600, 16000), (9000, 44100, 8000),
            (0, 44100, 16000), (2048, 48000, 16000), (1500, 15200, 16000), (1500, 16800, 16000)]
    return [(make_audio(rng, n, rin), rin, rout) for n, rin, rout in plan]


def big_cases():
    """[(x, rin, rout)]: 20 000 samples per ratio of RATES (the 16-bit test)."""
    rng = np.random.default_rng(37)
    return [(make_audio(rng, 20000, rin), rin, rout) for rin, rout in RATES]
