"""backend.fit_backend end to end on the GPU against the float64 oracle (tests/backend_ref.py), in units of the error of the
same oracle with float32 row statistics (tests/fp32_units.py, default thresholds).  Every check is invariant under sign flips
of the LDA / PLDA rows and under rotations inside near-degenerate eigenspaces: Gram matrices, eigenvalues and scores."""
import numpy as np
import pytest
import torch

from neuralplda_amd import backend, models
from neuralplda_amd.sv_trials_loaders import XvectorTable
from tests import backend_ref as ref
from tests import fp32_units as fu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LDA = 24
SEED = 3   # chosen on the CPU: the 24th / 25th LDA eigenvalues of the oracle are a factor > 10 apart (asserted below)


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, LDA, LDA
    beta, alpha, device, loss = [99.0], 15.0, DEV, "SoftCdet"


@pytest.fixture(scope="module")
def data():
    d = ref.synth(SEED)
    rng = np.random.default_rng(SEED + 1)
    x = d["table"]
    d["xt"] = XvectorTable.from_matrix(d["ids"], x)
    d["center"] = (x[rng.integers(0, len(x), 700)] + 0.3 * rng.standard_normal(512).astype(np.float32)).astype(np.float32)
    pivot = x.mean(0, dtype=np.float64).astype(np.float32)   # the float32 oracle takes its statistics about the mean, as the kernel does
    for name, kw in (("unit", {}), ("sqrt", {"length_norm": "sqrt_dim", "center": d["center"]})):
        d["o64" + name] = ref.fit_backend(x, d["offs"], LDA, rows=d["rows"], **kw)
        d["o32" + name] = ref.fit_backend(x, d["offs"], LDA, rows=d["rows"], dtype=np.float32, pivot=pivot, **kw)
    i = rng.integers(0, len(x), (2, 4096))
    d["pairs"] = (torch.from_numpy(x[i[0]]).to(DEV), torch.from_numpy(x[i[1]]).to(DEV))
    return d


def _model(be):
    torch.manual_seed(0)
    m = models.NeuralPlda(NC()).to(DEV)
    be.apply(m)
    return m.eval()


def _as_backend(o, length_norm="unit"):
    return backend.Backend(o["mean_vec"], o["transform_mat"], o["plda_mean"], o["plda_transform"], o["psi"], length_norm)


def _scores(m, pairs):
    with torch.no_grad():
        return m(*pairs).cpu().numpy()


def _check_all(be, d, tag, length_norm, got_scores):
    o64, o32 = d["o64" + tag], d["o32" + tag]
    assert o64["lda_eigs"][LDA - 1] >= 10.0 * o64["lda_eigs"][LDA], o64["lda_eigs"][LDA - 2:LDA + 2]
    A, A32 = be.transform_mat[:, :-1], o32["transform_mat"][:, :-1]
    W, B = o64["W"], o64["B"]
    out = {}
    out["A W A^T"] = fu.assert_fp32_level(A @ W @ A.T, np.eye(LDA), A32 @ W @ A32.T, f"{tag}: A W A^T")["all"]
    out["eigs"] = fu.assert_fp32_level(np.sort(np.diag(A @ B @ A.T))[::-1], o64["lda_eigs"][:LDA],
                                       np.sort(np.diag(A32 @ B @ A32.T))[::-1], f"{tag}: LDA eigenvalues")["all"]
    out["psi"] = fu.assert_fp32_level(be.psi, o64["psi"], o32["psi"], f"{tag}: psi")["all"]
    out["mean_vec"] = fu.assert_fp32_level(be.mean_vec, o64["mean_vec"], o32["mean_vec"], f"{tag}: mean.vec")["all"]
    s64 = _scores(_model(_as_backend(o64, length_norm)), d["pairs"])
    s32 = _scores(_model(_as_backend(o32, length_norm)), d["pairs"])
    out["scores"] = fu.assert_fp32_level(got_scores, s64, s32, f"{tag}: scores of 4096 pairs")["all"]
    # MI355X (rms / max), "unit": A W A^T 0.44 / 0.67, eigenvalues 0.47 / 0.54, psi 0.32 / 0.37, mean.vec 0.05 / 0.05,
    # scores 0.51 / 0.46; "sqrt": the same LDA figures, psi 0.32 / 0.37, mean.vec 0.09 / 0.15, scores 0.51 / 0.42
    print(f"{tag}: (rms, max) fp32 units {out}")
    assert np.abs(be.transform_mat[:, -1]).max() == 0.0   # the LDA is estimated on centred rows


def test_init_from_xvectors_against_the_oracle(data):
    torch.manual_seed(0)
    m = models.NeuralPlda(NC()).to(DEV)
    be = m.InitFromXvectors(data["xt"], data["spk2utt"])
    assert be.plda_transform.shape == (LDA, LDA) and be.transform_mat.shape == (LDA, 513) and be.length_norm == "unit"
    _check_all(be, data, "unit", "unit", _scores(m.eval(), data["pairs"]))


def test_sqrt_dim_and_in_domain_centre(data):
    center = torch.from_numpy(data["center"]).to(DEV)
    be = backend.fit_backend(data["xt"], data["spk2utt"], LDA, length_norm="sqrt_dim", center=center, device=DEV)
    _check_all(be, data, "sqrt", "sqrt_dim", _scores(_model(be), data["pairs"]))
    # the same estimate in the other geometry
    unit = backend.fit_backend(data["xt"], data["spk2utt"], LDA, device=DEV)
    c = np.sqrt(LDA)
    assert np.abs(be.psi - unit.psi).max() <= 1e-9 * unit.psi.max()
    assert np.abs(np.abs(be.plda_transform) * c - np.abs(unit.plda_transform)).max() <= 1e-9 * np.abs(unit.plda_transform).max()
    assert np.abs(be.mean_vec - unit.mean_vec).max() > 0.01   # the in-domain centre, not the training mean


def test_lda_only_models_and_truncation(data, capsys):
    spk2utt = list(data["spk2utt"])
    spk2utt[0] = (spk2utt[0][0], spk2utt[0][1] + ["not-in-the-table"])
    g = models.GaussianBackend(NC()).to(DEV)
    be = g.InitFromXvectors(data["xt"], spk2utt)
    assert "not-in-the-table" in capsys.readouterr().err
    assert be.plda_transform is None
    o64, o32 = data["o64unit"], data["o32unit"]
    A, A32 = be.transform_mat[:, :-1], o32["transform_mat"][:, :-1]
    fu.assert_fp32_level(A @ o64["W"] @ A.T, np.eye(LDA), A32 @ o64["W"] @ A32.T, "LDA only: A W A^T")
    assert np.array_equal(g.centering_and_LDA.weight.detach().cpu().numpy(), A.astype(np.float32))
    d = models.DPlda(NC()).to(DEV)
    d.InitFromXvectors(data["xt"], data["spk2utt"])
    assert torch.equal(d.centering_and_LDA.weight, g.centering_and_LDA.weight)
    cut = backend.fit_backend(data["xt"], data["spk2utt"], LDA, plda_dim=10, device=DEV)
    assert cut.plda_transform.shape == (10, LDA) and cut.psi.shape == (10,)
    fu.assert_fp32_level(cut.psi, o64["psi"][:10], o32["psi"][:10], "plda_dim = 10: psi")
    # fit_lda on raw rows: [A | -A mean]
    tm = backend.fit_lda(data["xt"].on(DEV), data["rows"], data["offs"], LDA)
    assert tm.shape == (LDA, 513)
    fu.assert_fp32_level(tm[:, -1], -(tm[:, :-1] @ o64["mean_vec"]), -(tm[:, :-1] @ o32["mean_vec"]), "fit_lda: offset column")
    fu.assert_fp32_level(tm[:, :-1] @ o64["W"] @ tm[:, :-1].T, np.eye(LDA), A32 @ o64["W"] @ A32.T, "fit_lda: A W A^T")


def test_lda_dim_that_is_no_multiple_of_four():
    """lda_dim = 22: the class scatter of y runs on 24 columns, two of them padding of the projection's output that the
    estimator slices away.  Data of between-class rank 22, so that the cut is at a gap."""
    L = 22
    d = ref.synth(SEED + 10, rank=L, S=64, max_utts=40)
    x = d["table"]
    pivot = x.mean(0, dtype=np.float64).astype(np.float32)
    o64 = ref.fit_backend(x, d["offs"], L, rows=d["rows"])
    o32 = ref.fit_backend(x, d["offs"], L, rows=d["rows"], dtype=np.float32, pivot=pivot)
    assert o64["lda_eigs"][L - 1] >= 10.0 * o64["lda_eigs"][L]
    be = backend.fit_backend(XvectorTable.from_matrix(d["ids"], x), d["spk2utt"], L, device=DEV)
    assert be.plda_transform.shape == (L, L) and np.isfinite(be.plda_transform).all() and np.isfinite(be.psi).all()
    A, A32 = be.transform_mat[:, :-1], o32["transform_mat"][:, :-1]
    r = {"A W A^T": fu.assert_fp32_level(A @ o64["W"] @ A.T, np.eye(L), A32 @ o64["W"] @ A32.T, "lda 22: A W A^T")["all"],
         "psi": fu.assert_fp32_level(be.psi, o64["psi"], o32["psi"], "lda 22: psi")["all"]}
    print(f"lda 22: (rms, max) fp32 units {r}")   # MI355X: A W A^T 0.66 / 0.60, psi 0.44 / 0.43
