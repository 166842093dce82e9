"""The AS-norm cohort score GEMMs held to fp32-level error PER SCORE (tests/fp32_units.py), on inputs made on the CPU
(tests/cohort_ref.py): the kernels read exactly the float32 tables the float64 / float32 references are computed from, so no
embedding error sits in the comparison and no average over a row's scores hides a lost low-order pass of the split product.

(a) The spilling GEMM (cohort_gemm_kernel), every score, through ops.cohort_scores.
(b) The fused GEMM (cohort_fused2_kernel: split form and fp32-input form, 128- and 256-row tiles), which never writes its
    matrix: 2 x 16 order statistics per row, recovered from the top-N means of n = 1 .. 16 (cohort_ref.probe).  The split
    form's gate is the case's g = sqrt(r_ok r_mut) of the numpy six-pass model — tests/test_cohort_ref_cpu.py shows that the
    six-pass product passes it by 1.5 x and each of the six dropped-pass forms misses it by 1.5 x."""
import numpy as np
import pytest
import torch

from tests import cohort_ref as cr
from tests import fp32_units as fu
from tests.test_topk_gpu import packed_for

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(c):
    packed = packed_for(c["P_sqrt"], c["Q"])
    assert packed.ldz == c["zr"].shape[1] == c["zc"].shape[1]
    return packed, _dev(c["zr"]), _dev(c["qr"]), _dev(c["zc"]), _dev(c["qc"])


def _fmt(r):
    return ", ".join(f"{k} {v[0]:.2f} / {v[1]:.2f}" for k, v in r.items())


# ---- (a) the spilling GEMM, every score ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,R,M", cr.SPILL_CASES)
def test_spilling_gemm_every_score(hip_lib, D, R, M):
    """ops.cohort_scores against ref64 in units of ref32's error: over all scores, over the row regions of the 128-row tiles
    and over the column regions of the 128-column tiles (first tile, last full tile, ragged last tile, a sample of the rest);
    default gates 3 / 5.  The matrix is bit-reproducible, and its row statistics are those of the spilling cohort_stats call.
    Measured on MI355X (rms / max ratio, worst over the row and column regions): D = 150 0.91 / 0.84, D = 170 0.99 / 1.38,
    D = 16 0.94 / 1.00, D = 24 0.92 / 1.11, D = 192 0.83 / 1.15."""
    from neuralplda_amd import ops
    c = cr.inputs("normal", "real", D, R, M)
    packed, zr, qr, zc, qc = _tables(c)
    S = ops.cohort_scores(zr, qr, zc, qc, packed)
    assert S.shape == (R, M) and S.dtype == torch.float32 and S.stride(1) == 1
    got = S.cpu().numpy()
    ref64, ref32 = cr.refs(c)
    rows, cols = fu.Regions(R, 128), fu.Regions(M, 128, seed=M)
    assert np.array_equal(rows.idx, np.arange(R))
    what = f"cohort_scores D={D} R={R} M={M}"
    print(what, "rows:", _fmt(fu.measure(got, ref64, ref32, rows)))
    print(what, "columns:", _fmt(fu.measure(got.T[cols.idx], ref64.T[cols.idx], ref32.T[cols.idx], cols)))
    fu.assert_fp32_level(got, ref64, ref32, what + " (row regions)", rows)
    fu.assert_fp32_level(got.T[cols.idx], ref64.T[cols.idx], ref32.T[cols.idx], what + " (column regions)", cols)
    assert torch.equal(S, ops.cohort_scores(zr, qr, zc, qc, packed))
    topn = min(100, M)
    fmin = hip_lib.nplda_cohort_fused_min_workspace_bytes(M, topn, D, D)
    if fmin == 0 or fmin - 256 >= 256 + (M + 3) // 4 * 4 * 4:   # (else no workspace size selects the spilling path)
        for select in ("lowest", "highest"):
            assert torch.equal(ops.row_stats(S, topn=topn, select=select),
                               ops.cohort_stats(zr, qr, zc, qc, packed, topn=topn, select=select, force_spill=True)), select


# ---- (b) the fused GEMM, probed scores ----------------------------------------------------------------------------------------

def _probe_form(ops, tabs, R, what):
    """The 2 x 16 order statistics of every row out of the fused path, the (R, 4) statistics of its n = 1 call, and the
    largest number of rows any of the 32 calls had on its fail list."""
    packed, zr, qr, zc, qc = tabs
    first, fails = {}, [0]

    def mean_top(n, select):
        st, nfb = ops.cohort_stats(zr, qr, zc, qc, packed, topn=n, select=select, return_fallback_rows=True)
        assert nfb is not None and nfb <= R // 20, (what, n, select, nfb)   # rows recomputed exactly: their share is capped
        fails[0] = max(fails[0], nfb)
        st = st.cpu().numpy()
        if n == 1:
            first[select] = st
        return st[:, 2]

    return cr.probe(mean_top), first["lowest"], fails[0]


@pytest.mark.parametrize("family,qkind,D,M,half", cr.FUSED_CASES)
def test_fused_gemm_probed_scores(hip_lib, monkeypatch, family, qkind, D, M, half):
    """Every probed score of the fused path against the same order statistic of ref64, in units of ref32's error over all rows
    and the regions of the 128-row tiles.  Split form: rms <= g of the case (1.59 .. 2.01 over the table), max <= 5; fp32-input
    form: rms <= min(g, 3), max <= 5.  Row mean and row std of the n = 1 call at the default gates 3 / 5, and the two forms
    against each other within the sum of their errors.
    Measured on MI355X, worst over the cohort sizes, tile heights and regions (rms / max ratio; design/k08_cohort_asnorm.md,
    "Accuracy per score", has the table).  Probe, split form: stress D = 150 0.82 / 0.87, 160 0.80 / 0.93, 170 0.84 / 0.85,
    176 0.80 / 0.92; normal with self terms D = 150 0.71 / 0.85, 170 0.73 / 0.86.  Probe, fp32-input form: stress D = 24
    1.03 / 1.20, 64 1.04 / 1.21, 150 1.02 / 1.02, 160 1.01 / 1.08, 170 1.01 / 0.99, 176 1.01 / 1.42, 192 1.01 / 1.19; normal
    with self terms D = 150 0.88 / 1.01, 170 0.89 / 1.14.  Row mean 0.00 / 0.00 everywhere (formed analytically in fp64), row
    std at most 0.22 / 0.48.  No call had a row on its fail list."""
    from neuralplda_amd import ops
    R = cr.R_FUSED
    assert hip_lib.nplda_cohort_fused_min_workspace_bytes(M, cr.NPROBE, D, D) > 0   # these shapes take the fused path
    s = cr.summary(family, qkind, D, R, M)
    g = s["probe"]["g"]
    tabs = _tables(cr.inputs(family, qkind, D, R, M))
    if half is not None:
        monkeypatch.setenv("NPLDA_COHORT_HALF", half)
    reg = fu.Regions(R, 128)
    assert np.array_equal(reg.idx, np.arange(R))
    forms = ("split", "fp32") if D in cr.SPLIT_DIMS else ("fp32",)
    got = {}
    for form in forms:
        if form == "fp32":
            monkeypatch.setenv("NPLDA_COHORT_SPLIT", "0")
        else:
            monkeypatch.delenv("NPLDA_COHORT_SPLIT", raising=False)
        what = f"fused {form} {family} q={qkind} D={D} M={M} half={half}"
        got[form], st, nfb = _probe_form(ops, tabs, R, what)
        print(f"{what} (g = {g:.3f}, at most {nfb} rows on a fail list) probe:", _fmt(fu.measure(got[form], s["os64"], s["os32"], reg)))
        print(f"{what} mean:", _fmt(fu.measure(st[:, 0], s["mean64"], s["mean32"], reg)),
              "| std:", _fmt(fu.measure(st[:, 1], s["std64"], s["std32"], reg)))
        fu.assert_fp32_level(got[form], s["os64"], s["os32"], what + " probe", reg,
                             rms_max=g if form == "split" else min(g, fu.RMS_MAX))
        fu.assert_fp32_level(st[:, 0], s["mean64"], s["mean32"], what + " row mean", reg)
        fu.assert_fp32_level(st[:, 1], s["std64"], s["std32"], what + " row std", reg)
    if len(forms) == 2:
        ea, eb = np.abs(got["split"] - s["os64"]), np.abs(got["fp32"] - s["os64"])
        assert np.all(np.abs(got["split"] - got["fp32"]) <= ea + eb + 1e-12 * np.abs(s["os64"])), what
