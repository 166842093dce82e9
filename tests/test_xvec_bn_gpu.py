"""The batch-statistics extractor (csrc/nplda_xvec_bn.hip, XVectorNet_ETDNN_12Layer.enable_batch_stats) on the MI355X
against its twin (tests/xvec_bn_ref.py): ReLU branches, accuracy in units of fp32 error with the device's branches forced
into the twin, the running-statistics update, bit-level determinism, the switch and its errors, and training
Etdnn_Xvec_NeuralPlda end to end under a plain .train().

Shapes: [40, 40, 40] (120 rows, less than one 128-row tile), [57, 130, 24, 301, 33] (545 rows: no tile multiple, several
statistics splits, a 24-frame utterance with 2 valid rows in tdnn7..tdnn10) and 17 x 301 = 5 117 rows (many splits; std
and var pooling).

Measured on one MI355X (fp32_units gates 3 rms / 5 max), worst over the four cases: x-vectors 1.65 rms / 2.20 max, the 22
gradients and their row / tap regions 1.59 / 2.14, batch means 1.45 / 1.97, unbiased variances 2.05 / 2.81 (both at
3 x 40); 0, 3 and 29 branches differ from pre64 > 0 at the three shapes, all within 5 e_l.  The per-case table is in
design/k27_xvec_batch_stats.md.  The twelve tests take 7 s."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fp32_units, xvec_bn_ref as bref, xvec_ref
from tests.xvec_grad_ref import GRAD_KEYS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = {"3x40": ([40, 40, 40], "std"), "ragged": ([57, 130, 24, 301, 33], "std"),
         "17x301 std": ([301] * 17, "std"), "17x301 var": ([301] * 17, "var")}


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


@pytest.fixture(scope="module")
def params():
    return xvec_ref.make_params()


def _extractor(params, pooling="std", momentum=None):
    from neuralplda_amd import models
    m = models.XVectorNet_ETDNN_12Layer(pooling_function=torch.var if pooling == "var" else torch.std)
    xvec_ref.load_into(m, params)
    m = m.to(DEV).train().enable_backward().enable_batch_stats()
    if momentum is not None:
        for t in m.tdnns():
            t.bn.momentum = momentum
    return m


def _inputs(seed, lengths):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((int(sum(lengths)), 30)).astype(np.float32),
            rng.standard_normal((len(lengths), 512)).astype(np.float32))


def _buffers(m):
    return ([t.bn.running_mean.detach().cpu().double().numpy() for t in m.tdnns()],
            [t.bn.running_var.detach().cpu().double().numpy() for t in m.tdnns()])


def _device_run(m, frames, lengths, G, fill=None):
    """One training-mode extract_ragged + backward -> dict(xvec, grads, masks [ten (R, ld) uint8 tables], bufs)."""
    from neuralplda_amd import _lib
    held = {}

    def alloc(n, dev, what):
        held[what] = (torch.empty(n, dtype=torch.uint8, device=dev) if fill is None
                      else torch.full((n,), fill, dtype=torch.uint8, device=dev))
        return held[what]

    m._bn_alloc = alloc
    try:
        m.zero_grad(set_to_none=True)
        xv = m.extract_ragged(torch.from_numpy(frames).to(DEV), lengths)
        (xv * torch.from_numpy(G).to(DEV)).sum().backward()
    finally:
        m._bn_alloc = None
    sd = dict(m.named_parameters())
    lib = _lib.load()
    R, U = int(sum(lengths)), len(lengths)
    masks = []
    off, ld = ctypes.c_size_t(), ctypes.c_int64()
    for l in range(10):
        assert lib.nplda_xvec_bn_mask_layout(R, U, l, ctypes.byref(off), ctypes.byref(ld)) == 0
        masks.append(held["saved"][off.value:off.value + R * ld.value].view(R, ld.value).cpu().numpy())
    return dict(xvec=xv.detach().cpu().double().numpy(), masks=masks,
                grads={k: sd[k].grad.detach().cpu().double().numpy() for k in GRAD_KEYS})


_CACHE = {}


def _case(name, params):
    """The device run (momentum 1: the buffers afterwards ARE the delivered mean and unbiased variance) and the float64 and
    float32 twins with the device's ReLU branches forced, computed once per shape."""
    if name not in _CACHE:
        lengths, pooling = CASES[name]
        frames, G = _inputs(1000 + len(name) + sum(lengths), lengths)
        m = _extractor(params, pooling, momentum=1.0)
        dev = _device_run(m, frames, lengths, G)
        dev["mean"], dev["uvar"] = _buffers(m)
        t64 = bref.run(frames, lengths, params, G, pooling, torch.float64, DEV, masks=dev["masks"])
        t32 = bref.run(frames, lengths, params, G, pooling, torch.float32, DEV, masks=dev["masks"])
        _CACHE[name] = (lengths, dev, t64, t32)
    return _CACHE[name]


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


@pytest.mark.parametrize("name", list(CASES))
def test_relu_branches(params, name):
    lengths, dev, t64, t32 = _case(name, params)
    R = sum(lengths)
    for l in range(10):
        dout = xvec_ref.LAYERS[l][1]
        mask = dev["masks"][l]
        rows = bref.valid_rows(lengths, l)
        outside = np.ones(R, bool)
        outside[rows] = False
        assert not mask[outside].any(), (name, l)
        assert not mask[:, dout:].any(), (name, l)
        assert set(np.unique(mask)) <= {0, 1}, (name, l)
        pre64, pre32 = t64["pre"][l], t32["pre"][l]
        e = np.abs(pre32 - pre64).max()
        differ = (mask[rows][:, :dout] != 0) != (pre64 > 0)
        assert not (differ & (np.abs(pre64) > 5 * e)).any(), (name, l, int(differ.sum()), e)
        print(f"{name} tdnn{l + 1}: {int(differ.sum())} of {differ.size} branches differ from pre64 > 0, e = {e:.2e}")


@pytest.mark.parametrize("name", list(CASES))
def test_accuracy_in_fp32_units_with_the_branches_forced(params, name):
    lengths, dev, t64, t32 = _case(name, params)
    worst = {}

    def note(kind, r):
        w = worst.get(kind, (0.0, 0.0))
        worst[kind] = (max(w[0], max(v[0] for v in r.values())), max(w[1], max(v[1] for v in r.values())))

    note("x-vectors", fp32_units.assert_fp32_level(dev["xvec"], t64["xvec"], t32["xvec"], f"{name} x-vectors"))
    for i, k in enumerate(GRAD_KEYS):
        g, r64, r32 = dev["grads"][k], t64["grads"][k], t32["grads"][k]
        layer = i // 2
        c = xvec_ref.LAYERS[layer][2] if layer < 10 else 1
        reg = _Rows(g.shape, xvec_ref.LAYERS[layer][0] if layer < 10 else None, c if g.ndim == 2 else 1)
        r = fp32_units.assert_fp32_level(g, r64, r32, f"{name} {k}", reg if g.ndim == 2 else None)
        for tap, cols in reg.cols.items():
            t = fp32_units.assert_fp32_level(g[:, cols], r64[:, cols], r32[:, cols], f"{name} {k} {tap}")
            r.update({f"{tap} {q}": v for q, v in t.items()})
        note("gradients", r)
    for l in range(10):
        note("batch mean", fp32_units.assert_fp32_level(dev["mean"][l], t64["mean"][l], t32["mean"][l],
                                                        f"{name} mean of tdnn{l + 1}"))
        note("unbiased variance", fp32_units.assert_fp32_level(dev["uvar"][l], t64["uvar"][l], t32["uvar"][l],
                                                               f"{name} variance of tdnn{l + 1}"))
    print(f"fp32 units {name}: " + "; ".join(f"{k} rms {v[0]:.2f} max {v[1]:.2f}" for k, v in worst.items()))


def test_running_statistics_update_and_a_following_eval_extraction(params):
    from neuralplda_amd import models
    lengths = CASES["ragged"][0]
    frames, G = _inputs(31, lengths)
    m = _extractor(params)  # torch's default momentum 0.1
    dev = _device_run(m, frames, lengths, G)
    t64 = bref.run(frames, lengths, params, G, "std", torch.float64, DEV, masks=dev["masks"])
    t32 = bref.run(frames, lengths, params, G, "std", torch.float32, DEV, masks=dev["masks"])
    mean, var = _buffers(m)
    for l in range(10):
        fp32_units.assert_fp32_level(mean[l], t64["running_mean"][l], t32["running_mean"][l], f"running_mean {l + 1}")
        fp32_units.assert_fp32_level(var[l], t64["running_var"][l], t32["running_var"][l], f"running_var {l + 1}")
        assert not np.array_equal(mean[l], params[f"tdnn{l + 1}.bn.running_mean"])
    assert all(int(t.bn.num_batches_tracked) == 1 for t in m.tdnns())
    X = torch.from_numpy(frames).to(DEV)
    with torch.no_grad():
        after = m.eval().extract_ragged(X, lengths)
        fresh = models.XVectorNet_ETDNN_12Layer()
        fresh.load_state_dict(m.state_dict())
        want = fresh.to(DEV).eval().extract_ragged(X, lengths)
    assert torch.equal(after, want)
    assert all(int(t.bn.num_batches_tracked) == 1 for t in m.tdnns())  # an eval extraction updates nothing


def test_bits(params):
    lengths = CASES["ragged"][0]
    frames, G = _inputs(32, lengths)
    m = _extractor(params, momentum=1.0)
    a = _device_run(m, frames, lengths, G)
    sa = _buffers(m)
    b = _device_run(m, frames, lengths, G)
    sb = _buffers(m)
    c = _device_run(m, frames, lengths, G, fill=0xFF)  # saved and the backward workspace start as 0xFF bytes
    sc = _buffers(m)
    for other, so in ((b, sb), (c, sc)):
        assert np.array_equal(a["xvec"], other["xvec"])
        for k in GRAD_KEYS:
            assert np.array_equal(a["grads"][k], other["grads"][k]), k
        for l in range(10):
            assert np.array_equal(sa[0][l], so[0][l]) and np.array_equal(sa[1][l], so[1][l]), l
            assert np.array_equal(a["masks"][l], other["masks"][l]), l
    assert all(int(t.bn.num_batches_tracked) == 3 for t in m.tdnns())
    # the no_grad forward is the grad-mode forward, statistics included (torch updates them under no_grad too)
    X = torch.from_numpy(frames).to(DEV)
    with torch.no_grad():
        plain = m.extract_ragged(X, lengths)
    assert not plain.requires_grad and np.array_equal(plain.cpu().double().numpy(), a["xvec"])
    sp = _buffers(m)
    assert all(np.array_equal(sa[0][l], sp[0][l]) and np.array_equal(sa[1][l], sp[1][l]) for l in range(10))
    assert all(int(t.bn.num_batches_tracked) == 4 for t in m.tdnns())
    # extract on (1, 30, T) is extract_ragged on the same rows
    x1 = np.random.default_rng(33).standard_normal((1, 30, 77)).astype(np.float32)
    one = m.extract(torch.from_numpy(x1).to(DEV))
    s1 = _buffers(m)
    rag = m.extract_ragged(torch.from_numpy(np.ascontiguousarray(x1[0].T)).to(DEV), [77])
    s2 = _buffers(m)
    assert one.requires_grad and torch.equal(one.detach(), rag.detach())
    assert all(np.array_equal(s1[0][l], s2[0][l]) and np.array_equal(s1[1][l], s2[1][l]) for l in range(10))


def test_switch_and_errors(params):
    from neuralplda_amd import models
    lengths = [40, 57]
    frames, _ = _inputs(34, lengths)
    X = torch.from_numpy(frames).to(DEV)
    old = xvec_ref.load_into(models.XVectorNet_ETDNN_12Layer(), params).to(DEV).eval().enable_backward()
    new = _extractor(params).eval()  # the switch on, all ten batch norms in eval mode: the existing paths
    with torch.no_grad():
        assert torch.equal(new.extract_ragged(X, lengths), old.extract_ragged(X, lengths))
    go, gn = old.extract_ragged(X, lengths), new.extract_ragged(X, lengths)
    assert gn.requires_grad and torch.equal(go.detach(), gn.detach())
    go.sum().backward()
    gn.sum().backward()
    po, pn = dict(old.named_parameters()), dict(new.named_parameters())
    assert all(torch.equal(po[k].grad, pn[k].grad) for k in GRAD_KEYS)
    assert all(int(t.bn.num_batches_tracked) == 0 for t in new.tdnns())
    new.train()
    new.tdnn2.bn.eval()
    with pytest.raises(RuntimeError, match="mixed batch-norm modes"):
        new.extract_ragged(X, lengths)
    new.train()
    with pytest.raises(RuntimeError, match="running-statistics batch norm only"):
        new.extract_windows(X, [[0, 40]])
    with pytest.raises(RuntimeError, match="saved activations"):
        new.extract_ragged(X, lengths, workspace_bytes=1 << 20)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        new.extract_ragged(X[:23], [23])
    new.enable_batch_stats(False)
    with pytest.raises(RuntimeError, match="running-statistics batch norm only"):
        new.extract_ragged(X, lengths)
    assert all(int(t.bn.num_batches_tracked) == 0 for t in new.tdnns())


def test_end_to_end_training_under_a_plain_train(params):
    from neuralplda_amd import models
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    xvec_ref.load_into(e.xvector_extractor, params)
    xvec_ref.load_into(e, xvec_ref.make_head())
    e = e.to(DEV).train()
    ext = e.xvector_extractor.enable_backward().enable_batch_stats()
    assert all(t.bn.training for t in ext.tdnns())
    torch.manual_seed(6)
    clf = models.SpeakerClassifier(4, 150, kind="aam", scale=30.0, margin=0.2).to(DEV)
    x = torch.from_numpy(np.random.default_rng(35).standard_normal((8, 30, 60)).astype(np.float32)).to(DEV)
    spk = [0, 0, 1, 1, 2, 2, 3, 3]
    opt = torch.optim.Adam(list(e.parameters()) + list(clf.parameters()), lr=1e-3)
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = e.loss_classify(x, spk, clf)
        loss.backward()
        if step == 0:
            sd = dict(e.named_parameters())
            keys = ["xvector_extractor." + k for k in GRAD_KEYS] + [
                "centering_and_LDA.weight", "centering_and_LDA.bias", "centering_and_wccn_plda.weight",
                "centering_and_wccn_plda.bias"]
            for k in keys:
                g = sd[k].grad
                assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, k
            assert torch.isfinite(clf.weight.grad).all() and clf.weight.grad.abs().max() > 0
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(e.loss_classify(x, spk, clf).item())
    print("loss_classify over three Adam steps:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(int(t.bn.num_batches_tracked) == 4 for t in ext.tdnns())
    # the other entry points run under the same mode: forward extracts the two sides in two calls (two updates)
    s = e(x, x.flip(0))
    assert s.shape == (8,) and torch.isfinite(s).all() and s.requires_grad
    assert all(int(t.bn.num_batches_tracked) == 6 for t in ext.tdnns())
    lp = e.loss_all_pairs(x, spk)
    lp.backward()
    assert torch.isfinite(lp) and torch.isfinite(e.extract_plda_embeddings(x)).all()
    assert all(int(t.bn.num_batches_tracked) == 8 for t in ext.tdnns())
