"""fp64 NumPy restatement of the feature front end (csrc/nplda_feat.hip, neuralplda_amd/features.py), shared by the feature
tests and tools/bench_features.py.  A plain helper, not a conftest.

There is no Kaldi next to this project, so the compressed-matrix layout is written down here from Kaldi's
compressed-matrix.h as the issue that introduced the front end states it, and this file and the hand-written byte strings of
tests/test_features_cpu.py are the specification the product code is held to:

    after the token: float32 min_value, float32 range, int32 num_rows, int32 num_cols (16 bytes, no size markers)
    CM   num_cols x (uint16 p0, p25, p75, p100), then num_rows * num_cols bytes COLUMN-major
    CM2  num_rows * num_cols uint16, row-major           CM3  num_rows * num_cols uint8, row-major
    uint16 v -> min_value + range * (1 / 65535) * v      CM3 byte b -> min_value + range * b / 255
    CM byte b, with the column's decoded percentiles:  b <= 64: p0 + (p25 - p0) b / 64;  b <= 192: p25 + (p75 - p25)
    (b - 64) / 128;  else p75 + (p100 - p75) (b - 192) / 63

An encoder AND a decoder for the three forms, the archive / scp writers, the energy-VAD rule (compute-vad-energy), the
sliding-window rule (apply-cmvn-sliding --center=true --norm-vars=false) and their composition."""
import struct

import numpy as np

FORMATS = ("FM", "DM", "CM", "CM2", "CM3")


# ---- compressed matrices ---------------------------------------------------------------------------------------------

def _global_header(mat):
    """float32 (min_value, range) that cover the matrix: min_value <= every value <= min_value + range."""
    lo, hi = (float(mat.min()), float(mat.max())) if mat.size else (0.0, 0.0)
    mn = np.float32(lo)
    if float(mn) > lo:
        mn = np.nextafter(mn, np.float32(-np.inf))
    rg = np.float32(hi - float(mn))
    if rg <= 0:
        rg = np.float32(1.0)
    while float(mn) + float(rg) < hi:
        rg = np.nextafter(rg, np.float32(np.inf))
    return float(mn), float(rg)


def _to_u16(x, mn, rg):
    return np.clip(np.rint((np.asarray(x, np.float64) - mn) / rg * 65535.0), 0, 65535).astype(np.int64)


def _from_u16(v, mn, rg):
    return mn + rg * (1.0 / 65535.0) * np.asarray(v, np.float64)


def encode(mat, fmt):
    """The object bytes after the binary marker (token included) of `mat` (T, D) in format `fmt`."""
    mat = np.asarray(mat, np.float64)
    T, D = mat.shape
    if fmt == "FM" or fmt == "DM":
        return fmt.encode() + b" \x04" + struct.pack("<i", T) + b"\x04" + struct.pack("<i", D) + \
            mat.astype("<f4" if fmt == "FM" else "<f8").tobytes()
    mn, rg = _global_header(mat)
    head = fmt.encode() + b" " + struct.pack("<ffii", mn, rg, T, D)
    if fmt == "CM2":
        return head + _to_u16(mat, mn, rg).astype("<u2").tobytes()
    if fmt == "CM3":
        return head + np.clip(np.rint((mat - mn) / rg * 255.0), 0, 255).astype(np.uint8).tobytes()
    assert fmt == "CM", fmt
    hdr = np.zeros((D, 4), dtype=np.int64)
    body = np.zeros((D, T), dtype=np.uint8)
    for c in range(D):
        col = np.sort(mat[:, c]) if T else np.zeros(1)
        q = [col[0], col[len(col) // 4], col[(3 * len(col)) // 4], col[-1]]
        p0 = min(int(_to_u16(q[0], mn, rg)), 65532)
        p25 = min(max(int(_to_u16(q[1], mn, rg)), p0 + 1), 65533)
        p75 = min(max(int(_to_u16(q[2], mn, rg)), p25 + 1), 65534)
        p100 = max(int(_to_u16(q[3], mn, rg)), p75 + 1)
        hdr[c] = (p0, p25, p75, p100)
        f0, f25, f75, f100 = (_from_u16(v, mn, rg) for v in hdr[c])
        x = mat[:, c]
        b = np.where(x < f25, np.clip(np.rint((x - f0) / (f25 - f0) * 64.0), 0, 64),
                     np.where(x < f75, 64 + np.clip(np.rint((x - f25) / (f75 - f25) * 128.0), 0, 128),
                              192 + np.clip(np.rint((x - f75) / (f100 - f75) * 63.0), 0, 63)))
        body[c] = b.astype(np.uint8)
    return head + hdr.astype("<u2").tobytes() + body.tobytes()


def decode(obj):
    """encode()'s bytes -> (float64 (T, D) matrix, bound): every value a correct decoder returns in float32 lies within
    `bound` = 4 ulp (fp32) of the largest magnitude the header admits (max |min_value|, |min_value + range|; for FM / DM
    the largest |value|) of this fp64 result."""
    tok, _, rest = obj.partition(b" ")
    fmt = tok.decode()
    if fmt in ("FM", "DM"):
        T, D = struct.unpack("<i", rest[1:5])[0], struct.unpack("<i", rest[6:10])[0]
        m = np.frombuffer(rest[10:], dtype="<f4" if fmt == "FM" else "<f8").astype(np.float64).reshape(T, D)
        return m, ulp_bound(float(np.abs(m).max()) if m.size else 0.0, 0.0)
    mn, rg, T, D = struct.unpack("<ffii", rest[:16])
    mn, rg = float(mn), float(rg)
    rest = rest[16:]
    if fmt == "CM2":
        m = _from_u16(np.frombuffer(rest, dtype="<u2"), mn, rg).reshape(T, D)
    elif fmt == "CM3":
        m = (mn + rg * (np.frombuffer(rest, dtype=np.uint8).astype(np.float64) / 255.0)).reshape(T, D)
    else:
        p = _from_u16(np.frombuffer(rest[:8 * D], dtype="<u2"), mn, rg).reshape(D, 4)
        b = np.frombuffer(rest[8 * D:], dtype=np.uint8).astype(np.float64).reshape(D, T)
        m = np.empty((T, D))
        for c in range(D):
            p0, p25, p75, p100 = p[c]
            bc = b[c]
            m[:, c] = np.where(bc <= 64, p0 + (p25 - p0) * bc / 64.0,
                               np.where(bc <= 192, p25 + (p75 - p25) * (bc - 64.0) / 128.0,
                                        p75 + (p100 - p75) * (bc - 192.0) / 63.0))
    return m, ulp_bound(mn, rg)


def ulp_bound(min_value, rng):
    """4 ulp (fp32) of max(|min_value|, |min_value + range|)."""
    big = np.float32(max(abs(min_value), abs(min_value + rng)))
    return 4.0 * float(np.spacing(big))


def write_ark(path, items):
    """items: [(key, matrix, format)] -> binary archive at `path`; returns {key: offset of the \\0B marker}."""
    offs, chunks, pos = {}, [], 0
    for key, mat, fmt in items:
        kb = key.encode("ascii") + b" "
        offs[key] = pos + len(kb)
        obj = kb + b"\0B" + encode(mat, fmt)
        chunks.append(obj)
        pos += len(obj)
    with open(path, "wb") as fh:
        fh.write(b"".join(chunks))
    return offs


def write_scp(path, ark_path, offs, order):
    with open(path, "w") as fh:
        fh.write("".join(f"{k} {ark_path}:{offs[k]}\n" for k in order))


# ---- energy VAD (compute-vad-energy) -----------------------------------------------------------------------------------

def vad_threshold(c0, energy_threshold=5.5, energy_mean_scale=0.5):
    c0 = np.asarray(c0, np.float64)
    return energy_threshold + energy_mean_scale * float(c0.mean()) if c0.size else energy_threshold


def vad_energy(c0, energy_threshold=5.5, energy_mean_scale=0.5, proportion_threshold=0.12, frames_context=2):
    """c0 (T,) -> bool (T,): frame t is voiced iff, over t2 in [t - ctx, t + ctx] clipped to [0, T), the number of frames
    with c0[t2] > thr is >= (number of t2) * proportion_threshold."""
    c0 = np.asarray(c0, np.float64)
    T = c0.shape[0]
    thr = vad_threshold(c0, energy_threshold, energy_mean_scale)
    above = np.concatenate([[0], np.cumsum(c0 > thr)])
    t = np.arange(T)
    lo, hi = np.maximum(t - frames_context, 0), np.minimum(t + frames_context, T - 1)
    return (above[hi + 1] - above[lo]) >= (hi - lo + 1) * proportion_threshold


# ---- sliding CMN (apply-cmvn-sliding --center=true --norm-vars=false) ----------------------------------------------

def window(t, T, W):
    s = t - W // 2
    e = s + W
    if s < 0:
        e -= s
        s = 0
    if e > T:
        s -= e - T
        e = T
    return max(s, 0), e


def sliding_mean(x, W):
    """x (T, D) -> fp64 (T, D): the mean of x[s:e] for every frame's window."""
    x = np.asarray(x, np.float64)
    T = x.shape[0]
    P = np.concatenate([np.zeros((1, x.shape[1])), np.cumsum(x, axis=0)])
    se = np.array([window(t, T, W) for t in range(T)], dtype=np.int64).reshape(T, 2)
    return (P[se[:, 1]] - P[se[:, 0]]) / (se[:, 1] - se[:, 0])[:, None]


def cmn(x, W):
    """-> (ref64, ref32): x - mean in fp64, and float32(x) - float32(mean) subtracted in float32."""
    x = np.asarray(x, np.float64)
    if W == 0:
        return x.copy(), x.astype(np.float32)
    m = sliding_mean(x, W)
    return x - m, x.astype(np.float32) - m.astype(np.float32)


def prepare(mats, masks=None, W=300, min_frames=25):
    """mats: [(T_u, D) decoded matrices], masks: [bool (T_u,)] or None -> (rows64, rows32, lengths, counts): the normalised
    voiced rows of the utterances that keep at least min_frames, one after the other; counts covers every utterance."""
    r64, r32, lengths, counts = [], [], [], []
    for i, x in enumerate(mats):
        keep = np.ones(x.shape[0], bool) if masks is None else np.asarray(masks[i], bool)
        n = int(keep.sum())
        counts.append(n)
        if n < min_frames or n == 0:
            continue
        a, b = cmn(x, W)
        r64.append(a[keep])
        r32.append(b[keep])
        lengths.append(n)
    D = mats[0].shape[1] if mats else 30
    cat = lambda L, dt: np.concatenate(L) if L else np.zeros((0, D), dt)  # noqa: E731
    return cat(r64, np.float64), cat(r32, np.float32), lengths, counts
