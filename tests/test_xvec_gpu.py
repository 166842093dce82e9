"""The HIP E-TDNN x-vector extractor (csrc/nplda_xvec.hip) on the MI355X: accuracy in units of fp32 error against the fp64
restatement (tests/xvec_ref.py), the reference-generated fixture g13, bit-identity across batch composition, layout,
chunking and runs, the edge cases, and head training on top of a frozen extractor."""
import os

import numpy as np
import pytest
import torch

from tests import fp32_units, xvec_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = os.path.join(ROOT, "tests", "golden", "g13_etdnn.npz")
DEV = torch.device("cuda:0")


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


@pytest.fixture(scope="module")
def params():
    return xvec_ref.make_params()


def _extractor(params, pooling=torch.std):
    from neuralplda_amd import models
    m = models.XVectorNet_ETDNN_12Layer(pooling_function=pooling)
    xvec_ref.load_into(m, params)
    return m.to(DEV).eval().requires_grad_(False)


def _check_fp32(got, frames, lengths, params, pooling, what):
    ref64 = xvec_ref.extract_ragged(frames, lengths, params, pooling, np.float64)
    ref32 = xvec_ref.extract_ragged(frames.astype(np.float32), lengths, params, pooling, np.float32)
    return fp32_units.assert_fp32_level(got, ref64, ref32, what)


@pytest.mark.parametrize("B,T", [(1, 24), (3, 40), (17, 301)])
@pytest.mark.parametrize("pooling", ["std", "var"])
def test_extract_in_fp32_units(params, B, T, pooling):
    # gates 3 / 5 (rms / max); measured on MI355X: std 1.36 / 1.51 (1, 24), 1.62 / 1.57 (3, 40), 1.24 / 2.12 (17, 301);
    # var 1.14 / 1.25, 1.63 / 1.52, 1.03 / 1.38
    m = _extractor(params, torch.var if pooling == "var" else torch.std)
    x = np.random.default_rng(B * 1000 + T).standard_normal((B, 30, T)).astype(np.float32)
    got = m.extract(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.shape == (B, 512)
    frames = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, 30)
    _check_fp32(got, frames, [T] * B, params, pooling, f"extract B={B} T={T} {pooling}")


def test_ragged_batch_in_fp32_units(params):
    # 64 utterances of 24..400 frames (T = 23, one pooled frame, is NaN: test_edge_cases); gates 3 / 5, measured 1.42 / 1.69
    rng = np.random.default_rng(64)
    lengths = rng.integers(24, 401, 64)
    frames = rng.standard_normal((int(lengths.sum()), 30)).astype(np.float32)
    m = _extractor(params)
    got = m.extract_ragged(torch.from_numpy(frames).to(DEV), lengths).cpu().numpy()
    _check_fp32(got, frames, lengths, params, "std", "ragged 64")


def test_large_batch_in_fp32_units(params):
    """Above 200 k frames: ~1 650 row tiles per layer, twelve column slices at tdnn10.  The oracle runs on the first and
    last utterances and a sample between (an utterance's result does not depend on the rest of the batch)."""
    rng = np.random.default_rng(200)
    lengths = rng.integers(300, 361, 640)
    total = int(lengths.sum())
    assert total > 200_000
    frames = rng.standard_normal((total, 30)).astype(np.float32)
    m = _extractor(params)
    got = m.extract_ragged(torch.from_numpy(frames).to(DEV), lengths).cpu().numpy()
    assert np.isfinite(got).all()
    pick = np.unique(np.concatenate([[0, 1, 638, 639], rng.choice(640, 4, replace=False)]))
    off = np.concatenate([[0], np.cumsum(lengths)])
    sub = np.concatenate([frames[off[u]:off[u + 1]] for u in pick])
    # gates 3 / 5, measured 1.08 / 1.55
    _check_fp32(got[pick], sub, lengths[pick], params, "std", "large batch")


def test_reference_fixture(params):
    g = np.load(G13)
    head = xvec_ref.make_head()
    from neuralplda_amd import models
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    xvec_ref.load_into(e.xvector_extractor, params)
    xvec_ref.load_into(e, head)
    e = e.to(DEV).train1()
    e.xvector_extractor.requires_grad_(False)
    for n in range(3):
        x = torch.from_numpy(g[f"x{n}"]).to(DEV)
        for pool, fn in (("std", torch.std), ("var", torch.var)):
            got = _extractor(params, fn).extract(x).cpu().numpy()
            ref = g[f"{pool}{n}"]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (n, pool)
            if np.isfinite(ref).any():
                assert np.nanmax(np.abs(got - ref)) <= 1e-4 * np.nanmax(np.abs(ref)), (n, pool)
        with torch.no_grad():
            s = e(x, torch.flip(x, dims=[2])).cpu().numpy()
        ref = g[f"score{n}"]
        assert np.array_equal(np.isnan(s), np.isnan(ref)), n
        ok = np.isfinite(ref)
        assert np.all(np.abs(s[ok] - ref[ok]) <= 2e-5 + 1e-5 * np.abs(ref[ok])), (n, s, ref)


def test_bit_identity(params):
    m = _extractor(params)
    rng = np.random.default_rng(7)
    lengths = rng.integers(23, 260, 40)
    frames = torch.from_numpy(rng.standard_normal((int(lengths.sum()), 30)).astype(np.float32)).to(DEV)
    whole = m.extract_ragged(frames, lengths)
    assert torch.equal(torch.nan_to_num(whole, nan=7.0), torch.nan_to_num(m.extract_ragged(frames, lengths), nan=7.0))
    off = np.concatenate([[0], np.cumsum(lengths)])
    single = torch.cat([m.extract_ragged(frames[off[u]:off[u + 1]], lengths[u:u + 1]) for u in range(len(lengths))])
    assert torch.equal(torch.nan_to_num(whole, nan=7.0), torch.nan_to_num(single, nan=7.0))
    chunked = m.extract_ragged(frames, lengths, workspace_bytes=4 << 20)  # one to a few utterances per call
    assert torch.equal(torch.nan_to_num(whole, nan=7.0), torch.nan_to_num(chunked, nan=7.0))
    # the reference's (B, 30, T) layout against the same utterances as ragged rows
    x = torch.from_numpy(rng.standard_normal((9, 30, 77)).astype(np.float32)).to(DEV)
    a = m.extract(x)
    b = m.extract_ragged(x.transpose(1, 2).reshape(-1, 30), [77] * 9)
    assert torch.equal(a, b)
    assert torch.equal(a, m.extract(x, workspace_bytes=1))
    assert torch.equal(a, m.extract(x.cpu()).to(DEV))


def test_edge_cases(params):
    m = _extractor(params)
    x = torch.randn(2, 30, 23, device=DEV)
    out = m.extract(x)
    assert out.shape == (2, 512) and torch.isnan(out).all()  # one pooled frame: std NaN, as torch.std
    e = m.extract(torch.zeros(0, 30, 50, device=DEV))
    assert e.shape == (0, 512) and e.device == DEV
    assert m.extract_ragged(torch.zeros(0, 30, device=DEV), []).shape == (0, 512)
    with pytest.raises(ValueError):
        m.extract(torch.zeros(1, 30, 22, device=DEV))


def test_packed_cache_follows_parameters(params):
    m = _extractor(params)
    x = torch.randn(2, 30, 60, device=DEV)
    a = m.extract(x)
    with torch.no_grad():
        m.tdnn4.kernel.weight.mul_(0.5)  # in place: version bump
    b = m.extract(x)
    assert not torch.equal(a, b)
    m.tdnn4.kernel.weight = torch.nn.Parameter(m.tdnn4.kernel.weight.detach() * 2.0, requires_grad=False)  # replaced
    assert torch.equal(a, m.extract(x))


def test_head_training_on_frozen_extractor(params):
    from neuralplda_amd import models
    head = xvec_ref.make_head()
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    xvec_ref.load_into(e.xvector_extractor, params)
    xvec_ref.load_into(e, head)
    e = e.to(DEV).train1()
    rng = np.random.default_rng(5)
    x1 = torch.from_numpy(rng.standard_normal((24, 30, 60)).astype(np.float32)).to(DEV)
    x2 = torch.from_numpy(rng.standard_normal((24, 30, 60)).astype(np.float32)).to(DEV)
    t = torch.from_numpy((rng.random(24) < 0.3).astype(np.float32)).to(DEV)
    with pytest.raises(RuntimeError, match="backward"):
        e(x1, x2)  # a trainable extractor: no backward through it
    e.xvector_extractor.requires_grad_(False)
    loss = e.loss(e(x1, x2), t)
    loss.backward()
    # the same step on x-vectors computed separately, through a plain NeuralPlda head
    h = models.NeuralPlda(NC())
    xvec_ref.load_into(h, head)
    h = h.to(DEV).train()
    with torch.no_grad():
        v1, v2 = e.xvector_extractor.extract(x1), e.xvector_extractor.extract(x2)
    lh = h.loss(h(v1, v2), t)
    lh.backward()
    assert torch.equal(loss.detach(), lh.detach())
    for name in ("centering_and_LDA.weight", "centering_and_LDA.bias", "centering_and_wccn_plda.weight", "P_sqrt", "Q",
                 "Th99"):
        ge, gh = e.get_parameter(name).grad, h.get_parameter(name).grad
        assert ge is not None and torch.equal(ge, gh), name
    assert all(p.grad is None for p in e.xvector_extractor.parameters())
    e.train()  # batch-statistics batch norm in the tdnns
    with pytest.raises(RuntimeError, match="train1"):
        e(x1, x2)
