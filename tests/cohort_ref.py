"""Inputs, references and the split-product model of the AS-norm cohort score GEMMs (csrc/nplda_cohort.hip,
csrc/nplda_cohort_fused.hip; a plain helper of tests/test_cohort_ref_cpu.py and tests/test_cohort_fp32_units_gpu.py, not a
conftest).

The score is s_rm = q_r + q_m + 2 sum_d P_d z_rd z_md with P = fp32(P_sqrt^2).  The embedding tables z (rows, ldz; columns
>= D2 zero) and the self terms q are made HERE, on the CPU, so the kernels' inputs are known bit for bit and the fp32
embedding error (1.2e-7, larger than what a lost low-order pass costs) is not part of any comparison.  ref64 is the score in
float64 from those float32 inputs, ref32 the same in float32 by plain left-to-right sums (tests/topk_ref.scores: the unit of
tests/fp32_units.py).

Input families.  `normal`: z ~ N(0, 1).  `stress`: every operand the split kernel cuts into bf16 pieces — z_m on the cohort
side, fp32(2 P z_r) on the row side — is h + m + l with h a bf16 value and m, l at 0.40 .. 0.49 of the ulp of the piece
above, random signs: the low-order passes (mm, hl, lh) carry as much of a product as they can.  Self terms: "zero" (q = 0:
the GEMM alone) or "real" (q = sum_d Q_d z_d^2 rounded to fp32: the epilogue's centring q_m + (q_r - c_r) in play).  The
cohort rows of the first and of the last 64-column tile are 1.5 x as large as the others, so that those columns are
over-represented among a row's extreme scores (what the order-statistic probe sees).

The order-statistic probe.  With top-N = n the third statistic of a row is the fp64 mean of its n extreme scores, so
n mean_n - (n - 1) mean_(n-1) is the row's n-th smallest (select "lowest") or n-th largest ("highest") score: 2 x 16 single
scores per row out of the fused path, which never writes its score matrix.  Order statistics are 1-Lipschitz in the max norm,
so they are compared with the same order statistics of ref64 / ref32 and no column matching is needed.

The model.  split_model() is the six-pass product in numpy: three bf16 pieces (round to nearest even; the residuals are exact
in fp32) of fp32(2 P z_r) and of z_m, the piece products of every 32-column block summed in fp32 in the kernel's order
mm, hl, lh, hm, mh, hh, then q added — and the six forms that drop one pass.  A case's gate is the geometric mean of the
six-pass form's rms ratio (r_ok) and the smallest rms ratio of a dropped-pass form (r_mut): g = sqrt(r_ok r_mut), with
r_ok <= g / 1.5 and r_mut >= 1.5 g asserted by tests/test_cohort_ref_cpu.py.  It comes from this file alone, never from a
kernel run."""
import functools

import numpy as np

from tests import fp32_units as fu
from tests import topk_ref as tr

NPROBE = 16          # order statistics probed per row and selection
R_FUSED = 300        # rows of a fused case: two full 128-row tiles and a ragged one
PASSES = ("mm", "hl", "lh", "hm", "mh", "hh")                              # the kernel's order inside a 32-column block
_PIECES = {"mm": (1, 1), "hl": (0, 2), "lh": (2, 0), "hm": (0, 1), "mh": (1, 0), "hh": (0, 0)}  # (cohort piece, row piece)


# ---- bf16 pieces ------------------------------------------------------------------------------------------------------------

def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split3(v):
    """(h, m, l) float32 arrays: h = bf16(v), m = bf16(v - h), l = bf16(v - h - m); both residuals are exact in float32."""
    v = np.asarray(v, dtype=np.float32)
    h = bf16_round(v)
    r1 = v - h
    m = bf16_round(r1)
    return h, m, bf16_round(r1 - m)


def _bf16_ulp(x):
    """The spacing of bf16 values at |x| (float64; x != 0)."""
    return np.exp2(np.floor(np.log2(np.abs(x))) - 7.0)


def stress_values(base, rng):
    """float32 values h + m + l: h = bf16(base), m and l at 0.40 .. 0.49 of the bf16 ulp of the piece above, random signs."""
    h = bf16_round(np.where(base == 0, 1.0, base).astype(np.float32)).astype(np.float64)
    sgn = lambda: rng.choice([-1.0, 1.0], h.shape)  # noqa: E731
    m = sgn() * rng.uniform(0.40, 0.49, h.shape) * _bf16_ulp(h)
    l = sgn() * rng.uniform(0.40, 0.49, h.shape) * _bf16_ulp(m)
    return (h + m + l).astype(np.float32)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def edge_columns(M):
    """Cohort rows of the first 64-column tile and of the last one (ragged unless 64 divides M)."""
    return np.arange(min(64, M)), np.arange((M - 1) // 64 * 64, M)


@functools.lru_cache(maxsize=None)
def inputs(family, qkind, D, R, M, seed=0):
    """dict(P_sqrt, Q, zr (R, ldz), qr (R,), zc (M, ldz), qc (M,)), all float32."""
    fam, qk = ("normal", "stress").index(family), ("zero", "real").index(qkind)
    rng = np.random.default_rng([seed, fam, qk, D, R, M])
    P_sqrt, Q = rng.uniform(0.2, 1.5, D).astype(np.float32), (-rng.uniform(0.0, 1.0, D)).astype(np.float32)
    ld = tr.padded_dim(D)
    br, bc = rng.standard_normal((R, D)), rng.standard_normal((M, D))
    first, last = edge_columns(M)
    bc[first] *= 1.5
    bc[last[last >= 64]] *= 1.5
    zr, zc = np.zeros((R, ld), np.float32), np.zeros((M, ld), np.float32)
    if family == "normal":
        zr[:, :D], zc[:, :D] = br, bc
    else:
        P2 = np.float32(2) * (P_sqrt * P_sqrt)
        zr[:, :D] = stress_values(br * P2.astype(np.float64), rng) / P2   # fp32(2 P z_r) is (to its last bit) a stress value
        zc[:, :D] = stress_values(bc, rng)
    if qkind == "real":
        qr, qc = tr.qvec(zr, Q, np.float32), tr.qvec(zc, Q, np.float32)
    else:
        qr, qc = np.zeros(R, np.float32), np.zeros(M, np.float32)
    return dict(D=D, R=R, M=M, P_sqrt=P_sqrt, Q=Q, zr=zr, qr=qr, zc=zc, qc=qc)


def refs(c):
    """(ref64, ref32): the (R, M) score matrix in float64 and in float32, from the float32 inputs."""
    a = (c["zr"], c["qr"], c["zc"], c["qc"], c["P_sqrt"])
    return tr.scores(*a, np.float64), tr.scores(*a, np.float32)


# ---- the probe --------------------------------------------------------------------------------------------------------------

def order_stats(S):
    """(R, 2 NPROBE) float64: the NPROBE smallest scores of every row ascending, then the NPROBE largest descending."""
    s = np.sort(np.asarray(S, dtype=np.float64), axis=1)
    return np.concatenate([s[:, :NPROBE], s[:, ::-1][:, :NPROBE]], axis=1)


def probe(mean_top):
    """Order statistics from top-N means: mean_top(n, select) -> (R,) float64 mean of the n extreme scores of every row, for
    n = 1 .. NPROBE and both selections.  Returns (R, 2 NPROBE) laid out as order_stats()."""
    cols = []
    for select in ("lowest", "highest"):
        prev = None
        for n in range(1, NPROBE + 1):
            cur = np.asarray(mean_top(n, select), dtype=np.float64)
            cols.append(cur.copy() if n == 1 else n * cur - (n - 1) * prev)
            prev = cur
    return np.stack(cols, axis=1)


def probed_columns(ref64):
    """(R, 2 NPROBE) column numbers the probe's order statistics come from."""
    o = np.argsort(ref64, axis=1, kind="stable")
    return np.concatenate([o[:, :NPROBE], o[:, ::-1][:, :NPROBE]], axis=1)


# ---- the six-pass product -------------------------------------------------------------------------------------------------------

def split_model(c):
    """{None: S, "mm": S without the mm pass, ...}: (R, M) float32 score matrices of the six-pass split product and of its
    six single-pass-dropped forms."""
    D = c["D"]
    P2 = np.float32(2) * (c["P_sqrt"] * c["P_sqrt"])
    a = np.zeros_like(c["zr"])
    a[:, :D] = c["zr"][:, :D] * P2                       # fp32(2 P z_r): what the kernel cuts into pieces on the row side
    rp, cp = split3(a), split3(c["zc"])
    forms = (None,) + PASSES
    acc = {f: np.zeros((c["R"], c["M"]), np.float32) for f in forms}
    for k0 in range(0, a.shape[1], 32):
        prod = {p: cp[_PIECES[p][0]][:, k0:k0 + 32] @ rp[_PIECES[p][1]][:, k0:k0 + 32].T for p in PASSES}
        for f in forms:
            for p in PASSES:
                if p != f:
                    acc[f] += prod[p].T
    q = c["qr"][:, None] + c["qc"][None, :]
    return {f: acc[f] + q for f in forms}


def gate_of(r_ok, r_mut):
    return float(np.sqrt(r_ok * r_mut))


@functools.lru_cache(maxsize=None)
def summary(family, qkind, D, R, M):
    """What the tests need of a case, without its matrices: the references' order statistics and row moments, the probed
    columns' coverage counts, and r_ok / r_mut / g of the model over the whole matrix ("all") and over the probe ("probe")."""
    c = inputs(family, qkind, D, R, M)
    ref64, ref32 = refs(c)
    os64, os32 = order_stats(ref64), order_stats(ref32)
    out = dict(os64=os64, os32=os32,
               mean64=ref64.mean(axis=1), std64=ref64.std(axis=1),
               mean32=ref32.astype(np.float64).mean(axis=1), std32=ref32.astype(np.float64).std(axis=1))
    cols = probed_columns(ref64)
    first, last = edge_columns(M)
    out["lane_hits"] = np.bincount((cols % 64).ravel(), minlength=64)
    out["first_tile_hits"] = int((cols < 64).sum())
    out["last_tile_hits"] = int((cols >= last[0]).sum())
    r = {"all": {}, "probe": {}}
    for f, S in split_model(c).items():
        r["all"][f] = fu.ratios(S, ref64, ref32)[0]
        r["probe"][f] = fu.ratios(order_stats(S), os64, os32)[0]
    for k in ("all", "probe"):
        r_ok, r_mut = r[k][None], min(r[k][p] for p in PASSES)
        out[k] = dict(r_ok=r_ok, r_mut=r_mut, g=gate_of(r_ok, r_mut), dropped={p: r[k][p] for p in PASSES})
    return out


# ---- case tables --------------------------------------------------------------------------------------------------------------

COHORT_SIZES = (4096, 4099, 5000)   # the smallest cohort the fused path takes, a ragged 64-column tile of 3, one of 8
SPLIT_DIMS = (150, 160, 170, 176)   # NB = 10 / 11: the split form is the default, the fp32-input form stays selectable
FP32_DIMS = (24, 64, 192)           # the fp32-input form only

# (family, qkind, D, M, half): `half` is the value of NPLDA_COHORT_HALF ("0": 256-row tiles, "1": 128-row tiles; None: the
# dispatch's own choice — 128-row tiles at 300 rows).  D = 176 in 256-row tiles is the unbatched row-load branch.
FUSED_CASES = (
    [("stress", "zero", D, M, h) for D in (150, 176) for M in COHORT_SIZES for h in ("0", "1")]
    + [("stress", "zero", D, M, None) for D in (160, 170) + FP32_DIMS for M in COHORT_SIZES]
    + [("normal", "real", D, M, None) for D in (150, 170) for M in COHORT_SIZES])
FUSED_INPUTS = sorted({c[:4] for c in FUSED_CASES})

# (D, R, M) of the spilling GEMM (128 x 128 tiles): ragged in both directions, the narrowest and the widest model, and at
# M = 24 700 two super-bands of column tiles
SPILL_CASES = [(150, 130, 257), (170, 200, 1000), (16, 129, 1025), (24, 140, 24700), (192, 129, 513)]
