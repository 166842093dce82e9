"""Accuracy in units of an fp32 computation (a plain helper of the GPU accuracy tests, not a conftest).

The oracle gates of the older tests (|ds| <= 2e-5 + 1e-5 |s|, gradients 1e-4 of max-abs) sit ~100x above what the kernels
deliver, so they cannot tell a correct split-bf16 product from one that dropped a piece.  Here a kernel's error against the
fp64 oracle is measured in units of the error the SAME oracle makes when it runs in float32:

    rms_ratio = rms(got - ref64) / max(rms(ref32 - ref64), 2^-24 rms(ref64))
    max_ratio = max|got - ref64| / max(max|ref32 - ref64|, 2^-24 max|ref64|)

A kernel that computes every sum in fp32 (in whatever order) lands near 1; one whose products lose bits, or whose sums are
longer / narrower than the oracle's, lands well above.  Both ratios are taken over the whole output and separately over named
index regions (first tile, last full tile, ragged last tile, the remainder a FWD_SPLIT batch hands to its second kernel, a
random sample of the rest) so that one bad tile cannot hide in an average.
"""
import numpy as np

TINY = 2.0 ** -24
RMS_MAX, MAX_MAX = 3.0, 5.0  # default thresholds (tests state the ratio measured on hardware next to each use)
REGION_ROWS = 256  # rows per edge region: a ratio over a handful of values is a draw, not a statistic


def _f64(a):
    return np.asarray(a, dtype=np.float64).ravel()


def _ratio(num, den):
    if num == 0.0:
        return 0.0
    return num / den if den > 0.0 else float("inf")


def ratios(got, ref64, ref32):
    """(rms_ratio, max_ratio) of `got` against the fp64 oracle in units of the fp32 oracle's error (inf if got is not finite)."""
    got, ref64, ref32 = _f64(got), _f64(ref64), _f64(ref32)
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    if got.size == 0:
        return 0.0, 0.0
    if not np.all(np.isfinite(got)):
        return float("inf"), float("inf")
    e, e32 = got - ref64, ref32 - ref64
    rms = lambda a: float(np.sqrt(np.mean(a * a)))  # noqa: E731
    rms_r = _ratio(rms(e), max(rms(e32), TINY * rms(ref64)))
    max_r = _ratio(float(np.abs(e).max()), max(float(np.abs(e32).max()), TINY * float(np.abs(ref64).max())))
    return rms_r, max_r


class Regions:
    """Named row sets of a batch of n rows.  `idx` is the sorted union (the rows the oracle is run on), `pos[name]` the
    positions of a region's rows inside `idx`."""

    def __init__(self, n, tile, split=None, sample=2048, seed=0, full=False):
        rng = np.random.default_rng(seed)
        w = max(tile, REGION_ROWS)
        named = {"first tile": np.arange(0, min(n, w))}
        nfull = n // tile * tile
        if nfull > 0:
            named["last full tile"] = np.arange(max(0, nfull - w), nfull)
        if n % tile:
            named["ragged last tile"] = np.arange(max(0, n - w), n)
        if split is not None and 0 < split < n:
            rem = np.arange(split, n)
            if rem.size > 8192:
                rem = np.unique(np.concatenate([rem[:w], rem[-w:], rng.choice(rem, 4096, replace=False)]))
            named["split remainder"] = rem
        if full or n <= sample + 2 * w:
            named["rest"] = np.arange(n)
        else:
            named["sample"] = np.sort(rng.choice(n, sample, replace=False))
        self.idx = np.unique(np.concatenate(list(named.values())))
        self.pos = {k: np.searchsorted(self.idx, v) for k, v in named.items()}
        self.n = n


def measure(got, ref64, ref32, regions=None):
    """{region: (rms_ratio, max_ratio)} over the whole output ('all') and each region (rows = first axis)."""
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    out = {"all": ratios(got, ref64, ref32)}
    if regions is not None:
        for name, p in regions.pos.items():
            out[name] = ratios(got[p], ref64[p], ref32[p])
    return out


def assert_fp32_level(got, ref64, ref32, what, regions=None, rms_max=RMS_MAX, max_max=MAX_MAX):
    """Assert rms_ratio <= rms_max and max_ratio <= max_max over the whole output and every region; returns the ratios."""
    r = measure(got, ref64, ref32, regions)
    bad = {k: v for k, v in r.items() if not (v[0] <= rms_max and v[1] <= max_max)}
    assert not bad, f"{what}: error above {rms_max} (rms) / {max_max} (max) fp32 units: {bad} (all regions: {r})"
    return r
