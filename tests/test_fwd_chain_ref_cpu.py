"""The chain-order reference (tests/fwd_chain_ref.py) on the CPU: what a correct forward kernel with the kernels' summation
order is entitled to in units of the float32 oracle's error (tests/fp32_units.py), and that numpy mutants of it — the slips
the generic forward instances could make — land far above the bounds tests/test_fp32_units_fwd_train_gpu.py uses.

The ratios measured here are the only source of a bound above fp32_units.RMS_MAX / MAX_MAX = 3 / 5 in that file: a case may
take more only where the reference's own ratio exceeds 2 (rms) or 3.3 (max), and then 1.5 x that ratio (fwd_bound below).
Measured (256 rows per side, every shape of fcr.SHAPES, the small-batch kernel's training and embedding schedules and v2's;
worst over shapes and schedules; run with -s to see each figure):

    one rounding per MFMA (EXACT):    s 1.50 / 1.65   y 1.02 / 1.09   z 0.88 / 1.10   rn 0.92 / 1.38
    one rounding per product (FMAF):  s 1.82 / 2.52   y 1.41 / 1.89   z 1.55 / 1.85   rn 1.14 / 1.43

Nothing exceeds 2 / 3.3, so every case of the GPU file keeps 3 / 5 and CHAIN_BOUNDS is empty.  A 100 - 128-step chain is NOT
worth 3 units: it is worth 0.5 - 0.7 with one rounding per MFMA and 1.0 - 1.4 with one per product (the float32 oracle's BLAS
is itself a sequential fmaf chain over K per output element), and the K-split instances about half of that (y 0.43 / 0.73
against 0.71 / 1.39 at (512, 150, 150)).  The MI355X lands on the FMAF figures to two digits (y 0.74 and 1.40, z 1.18 and 1.51
at those two; tests/test_fp32_units_fwd_train_gpu.py).

What IS worth 3 units is the unit: it depends on the BATCH the oracle is run on.  numpy's float32 matmul takes another BLAS
path for a handful of rows (here: up to 6 rows at (400, 180, 192), up to 8 at (500, 150, 160) and (512, 150, 150)), where the
oracle's own rms error is 2.3 - 3.1 x smaller (test_unit_shrinks_for_tiny_oracle_batches prints it), while the chain reference
is the same row by row whatever the batch.  Against a 6-row oracle the FMAF reference measures 3.1 - 3.2 (y) and 3.6 - 3.7 (z)
units at D0 = 400 / 500 — the "3.0 / 3.8" that tests/test_fp32_units_grad_gpu.py reported for the kernel at B = 3.  The GPU
tests of this pull request therefore pool the rows of many tiny launches and run the oracle once on the pooled rows.
"""
import numpy as np
import pytest

from tests import fp32_units as fu
from tests import fwd_chain_ref as fcr
from tests.test_forward_gpu import rand_params

N = 256  # rows per side
# (v2 treats a row the same in its training and embedding modes; the small-batch kernel's embedding mode has neither the
# K-split nor the half slot of NB = 10)
SCHEDULES = [(fcr.SMALL, fcr.TRAIN), (fcr.V2, fcr.TRAIN), (fcr.SMALL, fcr.EMBED)]
# (shape, kernel, output) -> (rms, max) ratio of the chain reference where it exceeds 2 / 3.3: none does
CHAIN_BOUNDS = {}


def fwd_bound(shape, kernel, output):
    """(rms_max, max_max) of one output of one case of tests/test_fp32_units_fwd_train_gpu.py."""
    if (shape, kernel, output) in CHAIN_BOUNDS:
        r, m = CHAIN_BOUNDS[(shape, kernel, output)]
        return max(fu.RMS_MAX, 1.5 * r), max(fu.MAX_MAX, 1.5 * m)
    return fu.RMS_MAX, fu.MAX_MAX


def make_inputs(shape, n=N, seed=0):
    D0, D1, D2 = shape
    rng = np.random.default_rng(sum(shape) + seed)
    p = rand_params(rng, D0, D1, D2)
    x1 = rng.standard_normal((n, D0)).astype(np.float32)
    x2 = rng.standard_normal((n, D0)).astype(np.float32)
    return p, x1, x2


_CACHE = {}


def refs(shape):
    """(p, x1, x2, fp64 outputs, fp32 outputs) of a shape, computed once and left unchanged."""
    if shape not in _CACHE:
        p, x1, x2 = make_inputs(shape)
        r64, r32 = fcr.oracle_outputs(x1, x2, p, np.float64), fcr.oracle_outputs(x1, x2, p, np.float32)
        for d in (r64, r32):
            for a in d.values():
                a.setflags(write=False)
        _CACHE[shape] = (p, x1, x2, r64, r32)
    return _CACHE[shape]


def all_ratios(got, r64, r32):
    return {k: fu.ratios(got[k], r64[k], r32[k]) for k in fcr.OUTPUTS if k in got}


def fmt(r):
    return "  ".join(f"{k} {v[0]:.2f} / {v[1]:.2f}" for k, v in r.items())


@pytest.mark.parametrize("shape", fcr.SHAPES)
def test_chain_reference_against_fp64(shape):
    """The reference's own ratios for s, y, z, rn: every schedule, both MFMA models.  A ratio of the reference (EXACT) above
    2 / 3.3 must be in CHAIN_BOUNDS (within 10 %: the bound of its case is traceable to this printout); every other one keeps
    3 / 5.  The per-product model (FMAF) is printed beside it and must itself meet the bound its case uses on the GPU."""
    p, x1, x2, r64, r32 = refs(shape)
    for kernel, mode in SCHEDULES:
        for mfma in (fcr.EXACT, fcr.FMAF):
            r = all_ratios(fcr.chain_outputs(x1, x2, p, kernel, mode, mfma), r64, r32)
            print(f"chain reference {shape} {kernel:5s} {mode:5s} {mfma:5s}: {fmt(r)}")
            for k, (rms, mx) in r.items():
                if mfma == fcr.FMAF:
                    bound = fwd_bound(shape, kernel, k)
                    assert rms <= bound[0] and mx <= bound[1], (shape, kernel, mode, k, rms, mx)
                elif (shape, kernel, k) in CHAIN_BOUNDS:
                    tr, tm = CHAIN_BOUNDS[(shape, kernel, k)]
                    assert rms >= tr / 1.1 and mx >= tm / 1.1, (shape, kernel, mode, k, rms, mx)
                else:
                    assert rms <= 2.0 and mx <= 3.3, (shape, kernel, mode, k, rms, mx)


def test_chain_reference_rows_do_not_depend_on_the_batch():
    p, x1, x2, _, _ = refs((500, 150, 160))
    whole = fcr.chain_outputs(x1[:40], x2[:40], p)
    for lo, hi in ((0, 1), (1, 4), (4, 21)):
        part = fcr.chain_outputs(x1[lo:hi], x2[lo:hi], p)
        n = hi - lo
        assert np.array_equal(part["s"], whole["s"][lo:hi])
        for k in ("y", "z", "rn"):
            assert np.array_equal(part[k][:n], whole[k][lo:hi]) and np.array_equal(part[k][n:], whole[k][40 + lo:40 + hi])


@pytest.mark.parametrize("shape", [(500, 150, 160), (400, 180, 192), (512, 150, 150)])
def test_unit_shrinks_for_tiny_oracle_batches(shape):
    """Prints the float32 oracle's own rms error of y against the rows handed to it per call, and the FMAF reference's y / z
    ratios with the oracle run on 3 pairs at a time (the unit of a B = 3 test) and on all rows at once.  Nothing about the
    BLAS library is asserted beyond what holds on any: run on all rows at once, the reference stays below 3 / 5."""
    from oracle import nplda_oracle as orc
    p, x1, x2, r64, r32 = refs(shape)
    for m in (3, 6, 8, 16, 240):
        y32 = np.concatenate([orc.extract_plda_embeddings(x1[i:i + m], p, np.float32, True)[1][1] for i in range(0, 240, m)])
        print(f"{shape} float32 oracle, {m} rows per call: rms error of y {np.sqrt(np.mean((y32 - r64['y'][:240]) ** 2)):.2e}")
    n = 240
    got = fcr.chain_outputs(x1[:n], x2[:n], p, fcr.V2, fcr.TRAIN, fcr.FMAF)
    tiny = [fcr.oracle_outputs(x1[i:i + 3], x2[i:i + 3], p, np.float32) for i in range(0, n, 3)]
    for k in ("y", "z"):
        sel = np.r_[0:n, N:N + n]
        t32 = np.concatenate([t[k][:3] for t in tiny] + [t[k][3:] for t in tiny])
        big, small = fu.ratios(got[k], r64[k][sel], r32[k][sel]), fu.ratios(got[k], r64[k][sel], t32)
        print(f"{shape} {k}: oracle on all rows {big[0]:.2f} / {big[1]:.2f}, on 6 rows at a time {small[0]:.2f} / {small[1]:.2f}")
        assert big[0] <= fu.RMS_MAX and big[1] <= fu.MAX_MAX


# ---- mutants: each is the reference with one slip a generic instance could make --------------------------------------------

def _params(p, **kw):
    from oracle import nplda_oracle as orc
    d = dict(W1=p.W1, b1=p.b1, W2=p.W2, b2=p.b2, P_sqrt=p.P_sqrt, Q=p.Q)
    d.update(kw)
    return orc.Params(*(np.array(d[k], np.float32) for k in ("W1", "b1", "W2", "b2", "P_sqrt", "Q")))


def _from_u(u1, u2, p, NB, D1, D2, rn_swap=False, bf16_y=False):
    """The rest of the small-batch training forward from the layer-1 outputs, with the two slips behind layer 1."""
    (y1, rn1), (y2, rn2) = fcr.row_norm(u1, NB, side=0), fcr.row_norm(u2, NB, side=1)
    if rn_swap:  # the norm of the pair's other row
        y1, y2, rn1, rn2 = u1 * rn2[:, None], u2 * rn1[:, None], rn2, rn1
    l1, l2 = y1, y2
    if bf16_y:  # y rounded to bfloat16 (round to nearest even) on its way to layer 2; the saved y stays float32
        def bf16(a):
            b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
            return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
        l1, l2 = bf16(y1), bf16(y2)
    z1, z2 = fcr.layer2(l1, p, NB), fcr.layer2(l2, p, NB)
    return dict(s=fcr.score(z1, z2, p, NB), y=np.concatenate([y1, y2])[:, :D1], z=np.concatenate([z1, z2])[:, :D2],
                rn=np.concatenate([rn1, rn2]))


def mutants(shape, p, x1, x2):
    """{name: outputs} of every mutant that exists at this shape (small-batch kernel, training mode)."""
    D0, D1, D2 = shape
    NB, KS1 = fcr.kernel_nb(D1, D2), (D0 + 15) // 16
    out = {}
    run = lambda q: fcr.chain_outputs(x1, x2, q)  # noqa: E731
    if D0 % 16:  # the ragged K tail dropped (the last 4 columns at D0 = 500, the last 8 at 72)
        W1 = p.W1.copy()
        W1[:, 16 * (KS1 - 1):] = 0
        out["ragged K tail dropped"] = run(_params(p, W1=W1))
    if KS1 >= 2:  # the last k16-step's weight fragment clamped to the previous step's
        W1 = p.W1.copy()
        w = D0 - 16 * (KS1 - 1)
        W1[:, 16 * (KS1 - 1):] = p.W1[:, 16 * (KS1 - 2):16 * (KS1 - 2) + w]
        out["last k16-step clamped to the previous"] = run(_params(p, W1=W1))
    if D1 % 16:  # the features of the last part-filled 16-block of layer 1 zeroed (150 .. 159 at NB = 10)
        W1, b1 = p.W1.copy(), p.b1.copy()
        W1[D1 // 16 * 16:], b1[D1 // 16 * 16:] = 0, 0
        out["part-filled feature block zeroed"] = run(_params(p, W1=W1, b1=b1))
    if D1 != D2:  # D1 and D2 swapped where the image is padded: W1 / b1 rows < D2, W2 rows < D1 and columns < D2, b2 < D1
        W1, b1, W2, b2 = p.W1.copy(), p.b1.copy(), p.W2.copy(), p.b2.copy()
        W1[D2:], b1[D2:], W2[D1:], b2[D1:] = 0, 0, 0, 0
        W2[:, D2:] = 0
        out["D1 and D2 swapped in the padding"] = run(_params(p, W1=W1, b1=b1, W2=W2, b2=b2))
    u1, u2 = fcr.layer1(x1, p, side=0), fcr.layer1(x2, p, side=1)
    out["rn of the partner row"] = _from_u(u1, u2, p, NB, D1, D2, rn_swap=True)
    out["y in bf16 before layer 2"] = _from_u(u1, u2, p, NB, D1, D2, bf16_y=True)
    if fcr.is_ksplit(D0, NB, fcr.SMALL, fcr.TRAIN):
        parts = fcr.layer1_partials(np.concatenate([x1, x2]), p, NB)
        for skip in range(4):
            q = parts.copy()
            q[skip] = 0
            n = len(x1)
            out[f"K-split partial {skip} skipped"] = _from_u(fcr.combine_partials(q[:, :n], p, NB, 0),
                                                             fcr.combine_partials(q[:, n:], p, NB, 1), p, NB, D1, D2)
    return out


@pytest.mark.parametrize("shape", fcr.SHAPES)
def test_mutants_land_above_the_bounds(shape):
    """Every mutant must exceed the bound of at least one output that the GPU case asserts — by a wide margin (x 3), so
    that the verdict does not hang on a draw."""
    p, x1, x2, r64, r32 = refs(shape)
    base = all_ratios(fcr.chain_outputs(x1, x2, p), r64, r32)
    found = mutants(shape, p, x1, x2)
    D0, D1, D2 = shape
    want = {"rn of the partner row", "y in bf16 before layer 2"}
    want |= {"ragged K tail dropped"} if D0 % 16 else set()
    want |= {"last k16-step clamped to the previous"} if D0 > 16 else set()
    want |= {"part-filled feature block zeroed"} if D1 % 16 else set()
    want |= {"D1 and D2 swapped in the padding"} if D1 != D2 else set()
    want |= {f"K-split partial {i} skipped" for i in range(4)} if shape[0] == 512 and D1 in (150, 170) else set()
    assert set(found) == want
    for name, got in found.items():
        r = all_ratios(got, r64, r32)
        print(f"mutant {shape} {name}: {fmt(r)}   (reference: {fmt(base)})")
        over = [k for k, (rms, mx) in r.items()
                if rms > 3 * fwd_bound(shape, fcr.SMALL, k)[0] or mx > 3 * fwd_bound(shape, fcr.SMALL, k)[1]]
        assert over, (shape, name, r)
