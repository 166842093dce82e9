"""Chain-order reference of the fused forward — test infrastructure, plain numpy, no GPU.

A float32 restatement of the two layers of NeuralPlda.forward that accumulates in the order the HIP kernels do
(csrc/nplda_fwd_small.h, nplda_fwd_v2.h, nplda_l1_ksplit.h), written from those sources.  It is NOT the code under test and no
test compares a kernel with it.  It exists to say how many units of the float32 oracle's error (tests/fp32_units.py) a
CORRECT kernel with this summation order is entitled to: the oracle sums through BLAS blocks, the kernels through one long
sequential chain per accumulator, and the two differ by more than rounding noise once the chain is 100 steps long.

What is modelled, per output element (feature f of row j):

 * layer 1, generic: the accumulator starts from the bias b1[f]; k16-steps ks = 0 .. KS1 - 1 in order; inside a step four
   MFMAs r = 0 .. 3, MFMA (ks, r) adding the four products of columns k = 16 ks + 4 g + r, g = 0 .. 3 (the packed image's
   k-permutation, csrc/nplda_common.h).  Columns >= D0 of a ragged last step meet zero weights and add exactly 0.
 * layer 1, K-split (D0 = 512, NB = 10 / 11, pair and training modes of the small-batch kernel): wave w runs the eight
   k16-steps 8 m + 2 w, 8 m + 2 w + 1 (m = 0 .. 3) from a ZERO accumulator; the owner v of a unit then forms
   ((p_v + p_(v+1)) + p_(v+2)) + p_(v+3) (wave indices mod 4) and adds the bias last.  Owner: block b < 8 -> wave b & 3;
   NB = 10: block 8 + i of side s -> wave 2 i + s; NB = 11: block 8 + i -> wave i.
 * row norm: sum of squares as an fmaf chain per lane over the lane's features in the kernel's order (small-batch kernel:
   wave w holds blocks w, w + 4, .. and, at NB = 10 in the pair modes, the half slot 8 + w / 2 of side w & 1; v2: one wave
   holds every block), the two lane butterflies (s0 + s1) + (s2 + s3), the small-batch kernel's ((w0 + w1) + w2) + w3 over
   its waves, then rn = 1 / max(sqrtf(ss), 1e-12) and y = u * rn — a reciprocal and a product, not a division.
 * layer 2: accumulator from b2, feature blocks kb = 0 .. NB - 1 of y in order, four MFMAs each, same k-permutation.
 * score: per lane fmaf(Q, fmaf(z1, z1, z2 * z2), .) then fmaf(2 P, z1 * z2, .) over the lane's features, P = P_sqrt^2
   rounded to float32, then the same butterflies and cross-wave sum as the norm.

The order of the four products INSIDE one MFMA is not documented.  It is treated as exact here (mfma = EXACT, the default):
the four products and the incoming accumulator are summed without intermediate rounding (in float64, where each product of
two float32 values is exact) and rounded to float32 once per MFMA step.  mfma = FMAF is the other end of what the hardware
may do, the model the header of csrc/nplda_fwd_kernel.h states ("a k-ordered fmaf chain"): one rounding per product, the four
k of an MFMA in ascending order — four times as many roundings per chain.  (Both go through float64 and round a second time
to float32; a double rounding changes one result in ~2^29.)  tests/test_fwd_chain_ref_cpu.py records both.

Entry points shadow oracle/nplda_oracle.py: extract_plda_embeddings (with intermediates) and forward.  The pieces (layer1,
layer1_partials / combine_partials, row_norm, layer2, score) are public so that tests can build numpy mutants from them.
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS_NORMALIZE = F32(1e-12)
NB_SIZES = (2, 4, 8, 10, 11, 12)  # csrc/nplda_common.h: nplda_kernel_nb
SMALL, V2 = "small", "v2"
PAIR, TRAIN, EMBED = "pair", "train", "embed"
EXACT, FMAF = "exact", "fmaf"  # the two models of one MFMA (module docstring)


def kernel_nb(D1, D2):
    nb = (max(D1, D2) + 15) // 16
    for s in NB_SIZES:
        if nb <= s:
            return s
    raise ValueError((D1, D2))


def is_ksplit(D0, NB, kernel, mode):
    """nplda_fwd_small.h: KSPLIT = KS1C == 32 && (NB == 10 || NB == 11) && (MODE_PAIR || MODE_TRAIN)."""
    return kernel == SMALL and mode in (PAIR, TRAIN) and D0 == 512 and NB in (10, 11)


def is_half(NB, kernel, mode):
    """nplda_fwd_small.h: HALF = NB == 10 && (MODE_PAIR || MODE_TRAIN)."""
    return kernel == SMALL and mode in (PAIR, TRAIN) and NB == 10


def _pad(a, shape):
    out = np.zeros(shape, F64)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def _mfma_chain(acc, X, W, steps, mfma=EXACT):
    """acc (n, F) float32 += X (n, K) W (F, K)^T over the k16-steps `steps`, one float32 rounding per MFMA (X, W in float64
    holding float32 values: their products are exact, so the float64 sum of four of them and acc stands in for the exact
    one); mfma = FMAF: one rounding per product, k = g ascending inside the MFMA."""
    g4 = 4 * np.arange(4)
    for ks in steps:
        for r in range(4):
            cols = 16 * ks + g4 + r
            if mfma == EXACT:
                acc = (acc.astype(F64) + X[:, cols] @ W[:, cols].T).astype(F32)
            else:
                for c in cols:
                    acc = (acc.astype(F64) + X[:, c:c + 1] * W[:, c]).astype(F32)
    return acc


def ksplit_steps(w):
    return [8 * m + 2 * w + h for m in range(4) for h in range(2)]


def ksplit_owner(NB, b, side):
    if b < 8:
        return b & 3
    return 2 * (b - 8) + side if NB == 10 else b - 8


def layer1_partials(x, p, NB, mfma=EXACT):
    """The four per-wave partial sums (4, n, 16 NB) of the K-split layer 1 (no bias)."""
    x = np.asarray(x, F32)
    X, W = x.astype(F64), _pad(np.asarray(p.W1, F32), (16 * NB, 512))
    assert x.shape[1] == 512
    return np.stack([_mfma_chain(np.zeros((x.shape[0], 16 * NB), F32), X, W, ksplit_steps(w), mfma) for w in range(4)])


def combine_partials(parts, p, NB, side):
    """own + next wave + ... in the owner's fixed order, the bias last (nplda_l1_ksplit.h: own_sum)."""
    b1 = _pad(np.asarray(p.b1, F32), (16 * NB,)).astype(F32)
    u = np.empty(parts.shape[1:], F32)
    for b in range(NB):
        v = ksplit_owner(NB, b, side)
        f = slice(16 * b, 16 * b + 16)
        acc = parts[v][:, f] + parts[(v + 1) & 3][:, f]
        acc = acc + parts[(v + 2) & 3][:, f]
        acc = acc + parts[(v + 3) & 3][:, f]
        u[:, f] = acc + b1[f]
    return u


def layer1(x, p, kernel=SMALL, mode=TRAIN, side=0, mfma=EXACT):
    """u = W1 x + b1, (n, 16 NB) float32 with exact zeros in the pad columns."""
    x = np.asarray(x, F32)
    D1, D0 = np.asarray(p.W1).shape
    NB = kernel_nb(D1, np.asarray(p.W2).shape[0])
    assert x.shape[1] == D0 and D0 % 4 == 0
    if is_ksplit(D0, NB, kernel, mode):
        return combine_partials(layer1_partials(x, p, NB, mfma), p, NB, side)
    KS1 = (D0 + 15) // 16
    X, W = _pad(x, (x.shape[0], 16 * KS1)), _pad(np.asarray(p.W1, F32), (16 * NB, 16 * KS1))
    acc = np.broadcast_to(_pad(np.asarray(p.b1, F32), (16 * NB,)).astype(F32), (x.shape[0], 16 * NB))
    return _mfma_chain(acc, X, W, range(KS1), mfma)


def lane_orders(NB, kernel=SMALL, mode=TRAIN, side=0):
    """(waves, 4, T) feature indices: the order in which lane group g of wave w visits its features in the norm and score
    reductions (-1: no feature).  v2 has one wave per tile."""
    if kernel == V2:
        blocks = [list(range(NB))]
    else:
        half = is_half(NB, kernel, mode)
        nbf = NB // 4 if half else (NB + 3) // 4
        blocks = [[w + 4 * i for i in range(nbf) if w + 4 * i < NB] for w in range(4)]
        if half:  # wave w: block 8 + w / 2 of side w & 1, after its whole blocks
            for w in range(4):
                if (w & 1) == side:
                    blocks[w].append(8 + (w >> 1))
    T = 4 * max(len(b) for b in blocks)
    out = -np.ones((len(blocks), 4, T), np.int64)
    for w, bl in enumerate(blocks):
        for g in range(4):
            feats = [16 * nb + 4 * g + r for nb in bl for r in range(4)]
            out[w, g, :len(feats)] = feats
    return out


def _lane_reduce(terms, order, fma_with=None):
    """Reduce `terms` (n, F) float64-held float32 values per the kernel: a chain per lane (acc = round(term + acc)), the two
    butterflies, then the waves left to right.  fma_with: a second (n, F) term chained after the first of each feature."""
    n = terms.shape[0]
    z = np.zeros((n, 1), F64)
    t1 = np.concatenate([terms, z], axis=1)  # index -1 -> 0
    t2 = None if fma_with is None else np.concatenate([fma_with, z], axis=1)
    acc = np.zeros((n,) + order.shape[:2], F32)
    for t in range(order.shape[2]):
        acc = (acc.astype(F64) + t1[:, order[:, :, t]]).astype(F32)
        if t2 is not None:
            acc = (acc.astype(F64) + t2[:, order[:, :, t]]).astype(F32)
    lanes = (acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3])  # (n, waves) float32
    out = lanes[:, 0]
    for w in range(1, lanes.shape[1]):
        out = out + lanes[:, w]
    return out


def row_norm(u, NB, kernel=SMALL, mode=TRAIN, side=0):
    """(y, rn): rn = 1 / max(sqrtf(sum of squares), 1e-12), y = u * rn."""
    u = np.asarray(u, F32)
    u64 = u.astype(F64)
    ss = _lane_reduce(u64 * u64, lane_orders(NB, kernel, mode, side))
    rn = F32(1.0) / np.maximum(np.sqrt(ss), EPS_NORMALIZE)
    return u * rn[:, None], rn


def layer2(y, p, NB, mfma=EXACT):
    """z = W2 y + b2 over the NB feature blocks of y in order, (n, 16 NB) float32 with exact zeros in the pad columns."""
    y = np.asarray(y, F32)
    W = _pad(np.asarray(p.W2, F32), (16 * NB, 16 * NB))
    acc = np.broadcast_to(_pad(np.asarray(p.b2, F32), (16 * NB,)).astype(F32), y.shape)
    return _mfma_chain(acc, y.astype(F64), W, range(NB), mfma)


def score(z1, z2, p, NB, kernel=SMALL, mode=TRAIN):
    z1, z2 = np.asarray(z1, F32), np.asarray(z2, F32)
    Q = _pad(np.asarray(p.Q, F32), (16 * NB,))
    ps = np.asarray(p.P_sqrt, F32)
    P2 = 2.0 * _pad(ps * ps, (16 * NB,))  # P rounded to float32 when the image is packed; 2 P is exact
    a, b = z1.astype(F64), z2.astype(F64)
    inner = (a * a + (z2 * z2).astype(F64)).astype(F32).astype(F64)  # fmaf(z1, z1, z2 * z2)
    return _lane_reduce(Q * inner, lane_orders(NB, kernel, mode, 0), fma_with=P2 * (z1 * z2).astype(F64))


def extract_plda_embeddings(x, p, dtype=np.float32, with_intermediates=False, kernel=SMALL, mode=TRAIN, side=0, mfma=EXACT):
    """orc.extract_plda_embeddings in the kernels' order.  z (n, D2); intermediates (u, y, rn) trimmed to D1 like the
    oracle's (u, y, nrm) — except that the third is the RECIPROCAL norm the kernels save.  side: 0 = the x1 rows, 1 = the x2
    rows of a pair tile (the K-split and the half slot of NB = 10 assign the two sides to different waves)."""
    assert np.dtype(dtype) == np.float32, "the chain reference is float32 only"
    D1, D2 = np.asarray(p.W1).shape[0], np.asarray(p.W2).shape[0]
    NB = kernel_nb(D1, D2)
    u = layer1(x, p, kernel, mode, side, mfma)
    y, rn = row_norm(u, NB, kernel, mode, side)
    z = layer2(y, p, NB, mfma)
    assert not u[:, D1:].any() and not y[:, D1:].any() and not z[:, D2:].any()
    if with_intermediates:
        return z[:, :D2], (u[:, :D1], y[:, :D1], rn)
    return z[:, :D2]


def forward(x1, x2, p, dtype=np.float32, kernel=SMALL, mode=TRAIN, with_intermediates=False, mfma=EXACT):
    """orc.forward in the kernels' order; with_intermediates also ((z1, u1, y1, rn1), (z2, u2, y2, rn2))."""
    assert np.dtype(dtype) == np.float32, "the chain reference is float32 only"
    D1, D2 = np.asarray(p.W1).shape[0], np.asarray(p.W2).shape[0]
    NB = kernel_nb(D1, D2)
    z1, i1 = extract_plda_embeddings(x1, p, dtype, True, kernel, mode, 0, mfma)
    z2, i2 = extract_plda_embeddings(x2, p, dtype, True, kernel, mode, 1, mfma)
    s = score(_pad(z1, (z1.shape[0], 16 * NB)).astype(F32), _pad(z2, (z2.shape[0], 16 * NB)).astype(F32), p, NB, kernel, mode)
    if with_intermediates:
        return s, ((z1,) + i1, (z2,) + i2)
    return s


# ---- the shape table of tests/test_fwd_chain_ref_cpu.py and tests/test_fp32_units_fwd_train_gpu.py --------------------------
# (D0, D1, D2): the smallest shapes that reach each template instance and edge of the generic forward kernels
SHAPES = [
    (4, 16, 16), (20, 24, 20),  # NB = 2, KS1 = 1 / 2: K shorter than the prefetch ring; D1 != D2
    (64, 40, 24),               # NB = 4, D1 != D2
    (128, 100, 40),             # NB = 8, part-filled 7th block
    (72, 150, 150),             # NB = 10, ragged K (8 of 16)
    (500, 150, 160),            # NB = 10, ragged K (4 of 16), D1 != D2
    (512, 150, 150), (512, 170, 170),  # the K-split instances (NB = 10 / 11)
    (512, 170, 150),            # NB = 11, D1 != D2
    (400, 180, 192), (512, 192, 192),  # NB = 12
]
OUTPUTS = ("s", "y", "z", "rn")


def oracle_outputs(x1, x2, p, dtype):
    """{s (n), y (2n, D1), z (2n, D2), rn (2n)} of oracle/nplda_oracle.py in `dtype`, x1 rows then x2 rows as forward_train
    saves them; rn = 1 / max(||u||, eps)."""
    from oracle import nplda_oracle as orc
    z, (_, y, nrm) = orc.extract_plda_embeddings(np.concatenate([x1, x2]), p, dtype, with_intermediates=True)
    out = dict(y=y, z=z, rn=dtype(1) / np.maximum(nrm, dtype(orc.EPS_NORMALIZE)))
    if len(x1) == len(x2):
        out["s"] = orc.forward(x1, x2, p, dtype)
    return out


def chain_outputs(x1, x2, p, kernel=SMALL, mode=TRAIN, mfma=EXACT):
    """The same dictionary from the chain reference."""
    s, (a, b) = forward(x1, x2, p, np.float32, kernel, mode, True, mfma)
    return dict(s=s, z=np.concatenate([a[0], b[0]]), y=np.concatenate([a[2], b[2]]), rn=np.concatenate([a[3], b[3]]))
