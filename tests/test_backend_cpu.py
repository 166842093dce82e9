"""The back-end estimators without a GPU: properties of the float64 oracle (tests/backend_ref.py), the library's dense
algebra (neuralplda_amd/backend.py: torch float64 on the CPU here, numpy on the host) against it, the speaker-list helpers,
the file round trip and the host-side sizing of the scatter kernel's workspace."""
import os
import warnings

import numpy as np
import pytest
import torch

from neuralplda_amd import backend, kaldi_format
from neuralplda_amd.sv_trials_loaders import XvectorTable
from tests import backend_ref as ref


@pytest.fixture(scope="module")
def small():
    """400 speakers x 1 .. 12 utterances in 12 dimensions, full-rank between-class covariance."""
    d = ref.synth(7, D0=12, rank=12, S=400, max_utts=12, within_max=0.5, cond=20.0)
    x = d["table"].astype(np.float64)
    d["stats"] = ref.plda_stats(x, d["offs"], d["rows"])
    return d


def test_oracle_em_never_lowers_the_data_log_likelihood(small):
    means, counts, off = small["stats"]
    trace = []
    ref.plda_em(means, counts, off, 10, trace=trace)
    assert len(trace) == 11
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(trace, trace[1:])), trace
    assert trace[-1] > trace[0]


def test_oracle_lda_whitens_within_and_diagonalises_between(small):
    x = small["table"].astype(np.float64)
    mean, T, W = ref.lda_covariances(x, small["offs"], small["rows"])
    A, eigs = ref.lda_transform(T, W, 8)
    np.testing.assert_allclose(A @ W @ A.T, np.eye(8), atol=1e-9)
    G = A @ (T - W) @ A.T
    assert np.abs(G - np.diag(np.diag(G))).max() <= 1e-9
    assert np.all(np.diff(np.diag(G)) <= 1e-9)
    np.testing.assert_allclose(np.diag(G), eigs[:8], atol=1e-9)
    tm = ref.fit_lda(x, small["offs"], 8, small["rows"])
    np.testing.assert_allclose(tm[:, -1], -(A @ mean), atol=1e-12)


def test_oracle_sqrt_dim_is_the_unit_estimate_rescaled(small):
    x = small["table"].astype(np.float64)
    y = ref.normalise(x - x.mean(0))
    D = y.shape[1]
    mu, tr, psi = ref.fit_plda(y, small["offs"], 10, small["rows"])
    mu_s, tr_s, psi_s = ref.fit_plda(y, small["offs"], 10, small["rows"], length_scale=np.sqrt(D))
    np.testing.assert_allclose(tr_s, tr / np.sqrt(D), rtol=0, atol=1e-10 * np.abs(tr).max())
    np.testing.assert_allclose(mu_s, mu * np.sqrt(D), rtol=0, atol=1e-10 * np.abs(mu_s).max())
    np.testing.assert_allclose(psi_s, psi, rtol=0, atol=1e-10 * psi.max())


def test_grouped_em_equals_the_literal_loop(small):
    means, counts, off = small["stats"]
    Wr, Br, mur = ref.plda_em(means, counts, off, 10)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    W, B, mu = backend.plda_em(t(means), t(counts), t(off), 10)
    assert W.dtype == torch.float64 and W.device.type == "cpu"
    for got, want in ((W, Wr), (B, Br), (mu, mur)):
        assert np.abs(got.numpy() - want).max() <= 1e-10 * np.abs(want).max()
    out, outr = backend.plda_output(W, B, mu), ref.plda_output(Wr, Br, mur)
    assert np.abs(out[2] - outr[2]).max() <= 1e-9 * outr[2].max()
    # the statistics the library forms from the kernel's outputs (here: from the oracle's) are the oracle's too
    sm, sc, cs = ref.class_stats(small["table"].astype(np.float64), small["offs"], small["rows"])
    m2, n2, off2 = backend.plda_stats(t(sc), t(cs), t(np.diff(small["offs"]).astype(np.float64)))
    assert np.abs(m2.numpy() - means).max() <= 1e-12 and np.abs(off2.numpy() - off).max() <= 1e-10 * np.abs(off).max()
    assert np.array_equal(n2.numpy(), counts)


def test_library_lda_algebra_equals_the_oracle(small):
    x = small["table"].astype(np.float64)
    mean, T, W = ref.lda_covariances(x, small["offs"], small["rows"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tm, eigs, nfl = backend.lda_from_stats(T, W, mean, 8)
    assert nfl == 0 and tm.shape == (8, 13)
    np.testing.assert_allclose(tm, ref.fit_lda(x, small["offs"], 8, small["rows"]), atol=1e-9)
    assert np.all(tm[np.arange(8), np.abs(tm[:, :-1]).argmax(1)] > 0)   # the sign rule
    # a singular within-class covariance is floored, counted and reported
    Ws = W.copy()
    Ws[:, 0] = Ws[0, :] = 0.0
    with pytest.warns(UserWarning, match="floored 1 of 12"):
        assert backend.lda_from_stats(T, Ws, mean, 4)[2] == 1


def _table(d):
    return XvectorTable.from_matrix(d["ids"], d["table"])


def test_spk2utt_and_class_layout(tmp_path, small):
    table = _table(small)
    spk2utt = list(small["spk2utt"][:5])
    spk2utt[1] = (spk2utt[1][0], ["nobody-1"] + spk2utt[1][1] + ["nobody-2"])   # two unknown utterances
    spk2utt.insert(3, ("ghost", ["nobody-3", "nobody-4"]))                      # a speaker left with nothing
    path = tmp_path / "spk2utt"
    path.write_text("".join(f"{s} {' '.join(u)}\n" for s, u in spk2utt) + "\n")
    parsed = backend.read_spk2utt(str(path))
    assert parsed == spk2utt
    rows, offs, speakers, missing = backend.class_layout(table, str(path))
    assert missing == ["nobody-1", "nobody-2", "nobody-3", "nobody-4"]
    assert speakers == [s for s, _ in small["spk2utt"][:5]]
    assert rows.dtype == np.int64 and offs.dtype == np.int64
    assert np.array_equal(offs, small["offs"][:6]) and np.array_equal(rows, small["rows"][:offs[-1]])
    same = backend.class_layout(table, dict(spk2utt))
    assert np.array_equal(same[0], rows) and np.array_equal(same[1], offs)


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 12, 8, 8
    beta, alpha, device, loss = [99.0], 15.0, "cpu", "SoftCdet"


def _oracle_backend(small, length_norm="unit"):
    r = ref.fit_backend(small["table"], small["offs"], 8, rows=small["rows"], length_norm=length_norm)
    return backend.Backend(r["mean_vec"], r["transform_mat"], r["plda_mean"], r["plda_transform"], r["psi"], length_norm)


def test_saved_files_fold_like_the_arrays(tmp_path, small):
    from neuralplda_amd import models
    be = _oracle_backend(small)
    out = be.save(str(tmp_path / "init"))
    assert sorted(os.listdir(out)) == ["mean.vec", "plda", "transform.mat"]
    np.testing.assert_allclose(kaldi_format.read_vector(os.path.join(out, "mean.vec")), be.mean_vec, rtol=1e-6)
    plda = kaldi_format.read_plda(os.path.join(out, "plda"))
    assert np.array_equal(plda["Psi_across_covar_diag"], be.psi) and np.array_equal(plda["plda_mean"], be.plda_mean)
    torch.manual_seed(0)
    a, b = models.NeuralPlda(NC()), models.NeuralPlda(NC())
    be.apply(a)
    b.LoadPldaParamsFromKaldi(os.path.join(out, "mean.vec"), os.path.join(out, "transform.mat"), os.path.join(out, "plda"))
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    assert torch.isfinite(a.P_sqrt).all() and float(a.P_sqrt.detach().min()) > 0
    # the LDA-only models take the LDA of the same arrays
    g = models.GaussianBackend(NC())
    be.apply(g)
    assert torch.equal(g.centering_and_LDA.weight, a.centering_and_LDA.weight)
    assert torch.equal(g.centering_and_LDA.bias, a.centering_and_LDA.bias)
    # a "sqrt_dim" estimate folds to the same model: layer 2 sees unit-length rows
    c = models.NeuralPlda(NC())
    _oracle_backend(small, "sqrt_dim").apply(c)
    for k in ("centering_and_wccn_plda.weight", "centering_and_wccn_plda.bias", "P_sqrt", "Q"):
        np.testing.assert_allclose(c.state_dict()[k].numpy(), a.state_dict()[k].numpy(), rtol=1e-5, atol=1e-6)


def test_plda_dim_keeps_the_leading_rows(small):
    be = _oracle_backend(small)
    cut = be.with_plda_dim(5)
    assert cut.plda_transform.shape == (5, 8) and cut.psi.shape == (5,) and cut.plda_mean.shape == (8,)
    assert np.array_equal(cut.plda_transform, be.plda_transform[:5]) and np.array_equal(cut.psi, be.psi[:5])
    assert np.all(np.diff(be.psi) <= 0)   # ... which are the largest between-class variances
    assert np.array_equal(cut.transform_mat, be.transform_mat)
    with pytest.raises(ValueError):
        be.with_plda_dim(9)


def test_scatter_workspace_is_host_arithmetic(hip_lib):
    f = hip_lib.nplda_class_scatter_workspace_bytes
    for n in (4, 152, 512):
        sizes = [f(N, 7, n) for N in (0, 1, 1000, 1025, 4096, 100_000, 1_200_000)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (n, sizes)
        assert f(5000, 1, n) <= f(5000, 50, n) <= f(5000, 5000, n)
    for n in (0, -4, 6, 516, 1024):
        assert f(1000, 7, n) == 0
    assert f(-1, 7, 512) == 0 and f(10, -1, 512) == 0
    # bounded: the fp64 slabs are per chunk of row groups, not per row group
    assert f(1_200_000, 7323, 512) < 256 << 20
