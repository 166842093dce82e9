"""Backward through the HIP E-TDNN extractor (csrc/nplda_xvec_bwd.hip) on the MI355X: the 22 gradients in units of fp32
error against the fp64 torch restatement (tests/xvec_grad_ref.py), the reference-generated fixture g14 (gradients and one
Adam step), the training forward's bit-identity with extract(), determinism, batch consistency and end-to-end training
of Etdnn_Xvec_NeuralPlda with torch's Adam and with the fused Adam.

Measured on one MI355X (fp32_units gates 3 rms / 5 max): worst rms ratio 2.27 (B = 1, T = 24, var), worst max ratio 4.24
up to 1000 frames; 11.0 at 17 x 301 frames with var pooling and 2.67 for the ragged 64-utterance batch, under MAX_KINK.
The five GPU test groups take about 10 s."""
import os

import numpy as np
import pytest
import torch

from tests import fp32_units, xvec_grad_ref as gref, xvec_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G14 = os.path.join(ROOT, "tests", "golden", "g14_etdnn_grads.npz")
DEV = torch.device("cuda:0")


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


@pytest.fixture(scope="module")
def params():
    return xvec_ref.make_params()


def _extractor(params, pooling="std"):
    from neuralplda_amd import models
    m = models.XVectorNet_ETDNN_12Layer(pooling_function=torch.var if pooling == "var" else torch.std)
    xvec_ref.load_into(m, params)
    return m.to(DEV).eval().enable_backward()


def _hip_grads(m, frames, lengths, G):
    m.zero_grad(set_to_none=True)
    xv = m.extract_ragged(torch.from_numpy(frames).to(DEV), lengths)
    (xv * torch.from_numpy(G).to(DEV)).sum().backward()
    sd = dict(m.named_parameters())
    return {k: sd[k].grad.detach().cpu().double().numpy() for k in gref.GRAD_KEYS}


def _case(seed, lengths):
    rng = np.random.default_rng(seed)
    frames = rng.standard_normal((int(sum(lengths)), 30)).astype(np.float32)
    G = rng.standard_normal((len(lengths), 512)).astype(np.float32)
    return frames, G


class _Rows:
    """fp32_units.Regions stand-in for a weight's first / last 16-row blocks and per-tap column blocks (biases are
    measured whole: 16 entries of a bias are too few for a ratio)."""

    def __init__(self, shape, tap_din=None, taps=1):
        n = shape[0]
        self.pos = {"first 16 rows": np.arange(min(16, n)), "last 16 rows": np.arange(max(0, n - 16), n)}
        self.cols = {}
        if taps > 1:
            for j in range(taps):
                self.cols[f"tap {j}"] = np.arange(j * tap_din, (j + 1) * tap_din)


# Above ~1000 frames some pre-activations lie within fp32 rounding of 0 and take the other ReLU branch in the fp64
# restatement than in any fp32 computation; each such kink moves a few gradient entries by a whole frame's contribution.
# The rms ratio is untouched by them; the max ratio of those cases gets a wider gate.
MAX_KINK = 16.0


def _check_all(got, ref64, ref32, what, max_max=fp32_units.MAX_MAX):
    worst = (0.0, 0.0)
    for i, k in enumerate(gref.GRAD_KEYS):
        g, r64, r32 = got[k], ref64[k], ref32[k]
        layer = i // 2
        c = xvec_ref.LAYERS[layer][2] if layer < 10 else 1
        reg = _Rows(g.shape, xvec_ref.LAYERS[layer][0] if layer < 10 else None, c if g.ndim == 2 else 1)
        r = fp32_units.assert_fp32_level(g, r64, r32, f"{what} {k}", reg if g.ndim == 2 else None, max_max=max_max)
        for name, cols in reg.cols.items():
            t = fp32_units.assert_fp32_level(g[:, cols], r64[:, cols], r32[:, cols], f"{what} {k} {name}",
                                             max_max=max_max)
            r.update({f"{name} {q}": v for q, v in t.items()})
        worst = (max(worst[0], max(v[0] for v in r.values())), max(worst[1], max(v[1] for v in r.values())))
    print(f"fp32 units {what}: worst rms {worst[0]:.2f} max {worst[1]:.2f}")
    return worst


@pytest.mark.parametrize("B,T", [(1, 24), (3, 40), (17, 301)])
@pytest.mark.parametrize("pooling", ["std", "var"])
def test_gradients_in_fp32_units(params, B, T, pooling):
    lengths = [T] * B
    frames, G = _case(100 + B + T, lengths)
    got = _hip_grads(_extractor(params, pooling), frames, lengths, G)
    ref64 = gref.extractor_grads(frames, lengths, params, G, pooling, torch.float64, DEV)
    ref32 = gref.extractor_grads(frames, lengths, params, G, pooling, torch.float32, DEV)
    _check_all(got, ref64, ref32, f"B={B} T={T} {pooling}", MAX_KINK if B * T > 1000 else fp32_units.MAX_MAX)


def test_ragged_batch_in_fp32_units_and_batch_consistency(params):
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(24, 401, 64)]
    assert sum(lengths) % 128 != 0
    frames, G = _case(8, lengths)
    m = _extractor(params)
    got = _hip_grads(m, frames, lengths, G)
    ref64 = gref.extractor_grads(frames, lengths, params, G, "std", torch.float64, DEV)
    ref32 = gref.extractor_grads(frames, lengths, params, G, "std", torch.float32, DEV)
    _check_all(got, ref64, ref32, "ragged 64", MAX_KINK)
    # the batch's gradient is the sum of its utterances' gradients (8 of them, to keep the test short)
    sub = lengths[:8]
    fsub, Gsub = frames[:sum(sub)], G[:8]
    whole = _hip_grads(m, fsub, sub, Gsub)
    off = np.concatenate([[0], np.cumsum(sub)])
    parts = [_hip_grads(m, fsub[off[u]:off[u + 1]], [sub[u]], Gsub[u:u + 1]) for u in range(8)]
    r64 = gref.extractor_grads(fsub, sub, params, Gsub, "std", torch.float64, DEV)
    r32 = gref.extractor_grads(fsub, sub, params, Gsub, "std", torch.float32, DEV)
    for k in gref.GRAD_KEYS:
        summed = np.sum([p[k] for p in parts], axis=0)
        # in fp32 units: the difference of two fp32 computations, each ~1 unit from the fp64 value
        rms_r, max_r = fp32_units.ratios(whole[k] - summed + r64[k], r64[k], r32[k])
        assert rms_r <= 2 * fp32_units.RMS_MAX and max_r <= MAX_KINK, (k, rms_r, max_r)


def test_training_forward_bits_and_determinism(params):
    lengths = [57, 130, 24, 301]
    frames, G = _case(9, lengths)
    m = _extractor(params)
    X = torch.from_numpy(frames).to(DEV)
    with torch.no_grad():
        plain = m.extract_ragged(X, lengths)
    xv = m.extract_ragged(X, lengths)
    assert xv.requires_grad and torch.equal(xv.detach(), plain)
    x3 = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 30, 50)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        p3 = m.extract(x3)
    assert torch.equal(m.extract(x3).detach(), p3)
    a = _hip_grads(m, frames, lengths, G)
    b = _hip_grads(m, frames, lengths, G)
    for k in gref.GRAD_KEYS:
        assert np.array_equal(a[k], b[k]), k
    # unused parameters keep grad None; switch off: the old error
    sd = dict(m.named_parameters())
    assert all(sd[k].grad is None for k in sd if k not in gref.GRAD_KEYS)
    m.enable_backward(False)
    with pytest.raises(RuntimeError, match="backward"):
        m.extract(x3)


def test_errors_with_the_switch_on(params):
    m = _extractor(params)
    x = torch.zeros(1, 30, 40, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="its input must not require grad"):
        m.extract(x)
    m.tdnn3.bn.train()
    with pytest.raises(RuntimeError, match="train1"):
        m.extract(x.detach())


def _load_model(params, head, pooling="std", alpha=15.0):
    from neuralplda_amd import models
    nc = NC()
    nc.pooling_function, nc.alpha = pooling, alpha
    e = models.Etdnn_Xvec_NeuralPlda(nc)
    xvec_ref.load_into(e.xvector_extractor, params)
    xvec_ref.load_into(e, head)
    return e.to(DEV).train1(finetune_extractor=True)


def test_reference_fixture(params):
    g = np.load(G14)
    head = xvec_ref.make_head()
    for n in range(int(g["ncases"])):
        pooling = str(g[f"pool{n}"])
        e = _load_model(params, head, pooling, float(g["alpha"]))
        with torch.no_grad():
            for b in e.beta:
                e.threshold[b].fill_(float(g[f"th{n}"]))
        x1, x2, t = (torch.from_numpy(g[f"{k}{n}"]).to(DEV) for k in ("xa", "xb", "t"))
        opt = torch.optim.Adam(e.parameters(), lr=float(g["lr"]))
        opt.zero_grad()
        loss = e.loss(e(x1, x2), t)
        loss.backward()
        assert abs(loss.item() - float(g[f"loss{n}"])) <= 1e-4 * abs(float(g[f"loss{n}"])), n
        sd = dict(e.named_parameters())
        for k in gref.HEAD_KEYS:
            ref = g[f"hgrad{n}/{k}"]
            got = sd[k].grad.cpu().numpy().ravel()[g[f"hidx{n}/{k}"]]
            assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (n, k)
        idx = {}
        for k in gref.GRAD_KEYS:
            name = "xvector_extractor." + k
            gg = sd[name].grad.detach().cpu().numpy().ravel()
            idx[k] = g[f"idx{n}/{k}"]
            ref = g[f"grad{n}/{k}"]
            assert abs(np.linalg.norm(gg) - float(g[f"norm{n}/{k}"])) <= 1e-4 * float(g[f"norm{n}/{k}"]), (n, k)
            assert np.abs(gg[idx[k]] - ref).max() <= 1e-4 * np.abs(ref).max(), (n, k)
        opt.step()
        for k in gref.GRAD_KEYS:
            p = sd["xvector_extractor." + k].detach().cpu().numpy().ravel()[idx[k]]
            ref = g[f"step{n}/{k}"]
            assert np.abs(p - ref).max() <= 1e-4 * np.abs(ref).max(), (n, k)


def _restated_steps(params, head, x1, x2, t, steps, lr, th0, alpha):
    """fp64 restatement of `steps` SoftCdet + Adam steps of the whole model; returns (losses, {key: param after the first
    step})."""
    P = gref.torch_params(params, torch.float64, DEV)
    H = {k: torch.tensor(head[k], dtype=torch.float64, device=DEV, requires_grad=True) for k in gref.HEAD_KEYS}
    th = [torch.full((1,), th0, dtype=torch.float64, device=DEV, requires_grad=True) for _ in range(2)]
    leaves = [P[k] for k in gref.GRAD_KEYS] + [H[k] for k in gref.HEAD_KEYS] + th
    opt = torch.optim.Adam(leaves, lr=lr)
    X1, X2, Tt = (torch.from_numpy(a).to(DEV, torch.float64) for a in (x1, x2, t))
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = gref.e2e_loss(X1, X2, Tt, P, H, th, alpha=alpha)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if len(losses) == 1:
            first = {k: P[k].detach().cpu().numpy() for k in gref.GRAD_KEYS}
    return losses, first


@pytest.mark.parametrize("fused", [False, True])
def test_end_to_end_training(params, fused):
    from neuralplda_amd import compat
    from neuralplda_amd.optim import FusedAdam
    head = xvec_ref.make_head()
    rng = np.random.default_rng(21)
    x1 = rng.standard_normal((6, 30, 40)).astype(np.float32)
    x2 = rng.standard_normal((6, 30, 52)).astype(np.float32)
    t = np.array([1, 0, 0, 1, 0, 0], np.float32)
    steps, lr, alpha = 3, 1e-3, 1.0  # thresholds at the median score, alpha 1: an unsaturated SoftCdet
    if fused:
        compat.install(fused_adam=True)
    try:
        e = _load_model(params, head, alpha=alpha)
        X1, X2, T = (torch.from_numpy(a).to(DEV) for a in (x1, x2, t))
        with torch.no_grad():
            th0 = float(e(X1, X2).median())
            for b in e.beta:
                e.threshold[b].fill_(th0)
        opt = torch.optim.Adam(e.parameters(), lr=lr)
        assert isinstance(opt, FusedAdam) == fused
        losses = []
        ext = e.xvector_extractor
        for _ in range(steps):
            opt.zero_grad()
            loss = e.loss(e(X1, X2), T)
            loss.backward()
            opt.step()
            losses.append(loss.item())
            if len(losses) == 1:
                sd = dict(e.named_parameters())
                first = {k: sd["xvector_extractor." + k].detach().cpu().numpy() for k in gref.GRAD_KEYS}
    finally:
        if fused:
            compat.uninstall()
    ref_losses, ref_p = _restated_steps(params, head, x1, x2, t, steps, lr, th0, alpha)
    assert np.allclose(losses, ref_losses, rtol=1e-4, atol=0), (losses, ref_losses)
    sd = dict(e.named_parameters())
    for k in gref.GRAD_KEYS:  # after the first step (later Adam steps amplify the few ill-conditioned entries)
        upd, ref_upd = first[k] - params[k], ref_p[k] - params[k]
        # Adam's first steps move a weight by about lr * sign(g): where |g| is within fp32 error of 0 the two runs may
        # step apart, elsewhere they agree.  A wrong gradient would move about half the entries the wrong way.
        off = np.abs(upd - ref_upd) > 0.1 * lr
        assert off.mean() <= 0.01, (k, off.mean())
    # an extract after the steps uses the new weights
    with torch.no_grad():
        now = ext.extract(X1)
        P = gref.torch_params({**params, **{k: sd["xvector_extractor." + k].detach().cpu().numpy() for k in gref.GRAD_KEYS}},
                              torch.float64, DEV)
        want = torch.stack([gref.extract_one(torch.from_numpy(x1[b].T.copy()).to(DEV, torch.float64), P) for b in range(6)])
    assert torch.allclose(now.double(), want, rtol=0, atol=1e-4 * want.abs().max().item())
