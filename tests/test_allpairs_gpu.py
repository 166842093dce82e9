"""The all-pairs training step (csrc/nplda_allpairs.hip, ops.allpairs_loss, NeuralPlda.loss_all_pairs) on the MI355X against
tests/allpairs_ref.py: the dense numpy reference in float64, with its float32 evaluation as the unit (tests/fp32_units.py).

Shapes (allpairs_ref.CASES, T = ops.ALLPAIRS_TILE = 64): N in {2, 3, T - 1, T, T + 1, 2 T + 17, 3 T + 17} — the last with four
row tiles and seven 32-column stages, both ragged — D2 in {150, 160, 170} (padded to 160, 160, 176: six and ten zero features),
SoftCdet with K in {1, 2, 4} and BCE; labels with 1 - 9 utterances per speaker and singletons, one speaker across the first
tile edge, two groups of unequal size, and all rows one speaker but one.  Inputs from tests/synth.py scaled so that the float64
reference has alpha |theta_k - s_ij| < 60 on every trial (asserted), so no element is left out of any comparison.

Checks: N_t, N_n exact; the other sums within allpairs_ref.sum_bound (a rounding count); loss and dtheta equal to the float64
formulas on the device's own sums rounded once; dz (all rows and the first / last full / ragged row tiles), dP_sqrt and dQ at
the default gates 3 (rms) / 5 (max) fp32 units — tests/test_allpairs_cpu.py holds the float32 reference in a second summation
order to the same gates, so none is widened.  N = 2 has one class only under SoftCdet (the gradient is 0 / 0 as for the
pairwise kernels at B = 1): sums only.

Measured on MI355X (each test prints its figures with -s):

    check                                                                        measured
    ---------------------------------------------------------------------------  ---------------------------------
    dz, rms / max fp32 units over the cases and the row-tile regions             0.05 - 0.65 / 0.05 - 0.96
    dP_sqrt, dQ                                                                  <= 0.69 / 0.75, <= 0.68 / 0.88
    sums, share of the rounding bound                                            1.2e-06 - 9.1e-04
    pad rows 1e30 + identical rows: dz, dP_sqrt, dQ; sums                        0.35 / 0.30, 0.32 / 0.34, 0.32 / 0.64; 1.3e-05
    NeuralPlda.loss_all_pairs, worst of the loss and nine gradients              0.21 / 0.21
    loss(forward(x[i], x[j]), t) on the same list, beside it                     0.46 / 0.46
"""
import numpy as np
import pytest
import torch

from tests import allpairs_ref as ar
from tests import fp32_units as fu
from tests import loss_ref as lr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = torch.device("cuda:0")
KIND = {"softcdet": 0, "bce": 1}


def _thetas(c):
    return [torch.tensor([x], dtype=torch.float32, device=DEV) for x in c["theta"]]


def _dev(a):
    return torch.tensor(a).to(DEV)  # (a copy: the shared cases are read-only arrays)


def run(c, z=None, want_grad=True):
    from neuralplda_amd import ops
    z = _dev(c["z"]) if z is None else z
    grp = None if c["grp"] is None else torch.tensor(c["grp"])  # (labels may live on another device than z)
    return ops.allpairs_loss(z, _dev(c["spk"]), _dev(c["P_sqrt"]), _dev(c["Q"]), _thetas(c), c["beta"], c["alpha"],
                             KIND[c["kind"]], grp=grp, want_grad=want_grad)


def host(out):
    return [None if t is None else t.detach().cpu().numpy() for t in out]


def check_sums(sums, c, what):
    r64 = c["r64"]
    assert sums[0] == r64.Nt and sums[1] == r64.Nn, (what, sums[:2], r64.Nt, r64.Nn)
    err = np.abs(sums - r64.sums)[2:]
    assert np.all(err <= c["bound"][2:]), f"{what}: sums off by {err / c['bound'][2:]} of the rounding bound"
    return float((err / c["bound"][2:]).max())


def check_scalars(sums, loss, dth, c, what):
    """loss and dtheta are the float64 formulas on the device's OWN sums, rounded once (as tests/test_loss_fp32_gpu.py)."""
    K = c["K"]
    if c["kind"] == "bce":
        L, d = lr.bce_scalars(sums)
        tol = U * np.abs(d) + 2.0 ** -48 * np.abs(sums[3]) / (sums[0] + sums[1])
    else:
        L, d = lr.softcdet_scalars(sums, c["beta"], c["alpha"], K)
        a = float(np.float32(c["alpha"]))
        b = np.array([float(np.float32(x)) for x in c["beta"]])
        tol = U * np.abs(d) + 2.0 ** -48 * (a * sums[4::4] / sums[0] + b * a * sums[5::4] / sums[1]) / K
    assert abs(loss - L) <= U * abs(L), (what, loss, L)
    assert np.all(np.abs(dth - d) <= tol), (what, dth, d)


def check_grads(dz, dP, dQ, c, what, gates=True):
    from neuralplda_amd import ops
    r64, r32 = c["r64"], c["r32"]
    N = dz.shape[0]
    reg = fu.Regions(N, ops.ALLPAIRS_TILE, full=True)
    out = {}
    for name, got, regions in (("dz", dz, reg), ("dP_sqrt", dP, None), ("dQ", dQ, None)):
        if gates:
            r = fu.assert_fp32_level(got, getattr(r64, name), getattr(r32, name), f"{what} {name}", regions)
        else:
            r = fu.measure(got, getattr(r64, name), getattr(r32, name), regions)
        out[name] = (max(v[0] for v in r.values()), max(v[1] for v in r.values()))
    return out


@pytest.mark.parametrize("cs", ar.CASES, ids=lambda c: "-".join(map(str, c)))
def test_against_the_dense_reference(cs):
    from neuralplda_amd import ops
    assert ar.TILE == ops.ALLPAIRS_TILE
    c = ar.case(*cs)
    assert ar.span_of(c) < 60.0
    loss, dth, sums, dz, dP, dQ = host(run(c))
    assert dz.shape == c["z"].shape and dP.shape == dQ.shape == c["Q"].shape
    share = check_sums(sums, c, cs)
    if c["r64"].Nt == 0 or c["r64"].Nn == 0:
        if c["kind"] == "bce":
            check_scalars(sums, float(loss), dth.astype(np.float64), c, cs)
            ratios = check_grads(dz, dP, dQ, c, str(cs))
            print(f"{cs}: sums {share:.2g} of the bound; fp32 units {ratios}")
        return
    check_scalars(sums, float(loss), dth.astype(np.float64), c, cs)
    ratios = check_grads(dz, dP, dQ, c, str(cs))
    print(f"{cs}: sums {share:.2g} of the bound; fp32 units (rms, max) {ratios}")
    # the loss without gradients: the same sums from the upper tiles alone
    loss0, dth0, sums0, dz0, dP0, dQ0 = run(c, want_grad=False)
    assert dth0 is None and dz0 is None and dP0 is None and dQ0 is None
    assert np.array_equal(sums0.cpu().numpy(), sums) and float(loss0) == float(loss)


def _recase(base, z):
    """`base` with other embeddings: references and bound recomputed."""
    c = dict(base, z=z)
    args = (z, c["spk"], c["P_sqrt"], c["Q"], c["theta"], c["beta"], c["alpha"], c["kind"], c["grp"])
    c["r64"], c["r32"] = ar.allpairs(*args, np.float64), ar.allpairs(*args, np.float32)
    c["bound"] = ar.sum_bound(c["r64"], z, c["P_sqrt"], c["Q"], c["theta"], c["alpha"], c["kind"])
    return c


def test_nothing_leaks_from_pad_rows_or_the_diagonal():
    """z is a view of a larger buffer whose rows beyond N and columns beyond D2 hold 1e30, and two rows (of different tiles
    and different speakers) are identical, so that a trial scores what the diagonal s_ii would: the same gates, everything
    finite, the counts exact (a diagonal or pad element taken for a trial shows there first)."""
    N, D2 = 2 * ar.TILE + 17, 150
    base = ar.case(N, D2, "softcdet", 2, "mixed")
    z = base["z"].copy()
    z[ar.TILE + 2] = z[5]
    assert base["spk"][5] != base["spk"][ar.TILE + 2]
    c = _recase(base, z)
    while ar.span_of(c) >= 58.0:   # (the duplicated row's self score may be the largest of the batch)
        c = _recase(base, (c["z"] * np.float32(0.8)).astype(np.float32))
    assert ar.span_of(c) < 60.0
    buf = torch.full((N + 40, 160), 1e30, dtype=torch.float32, device=DEV)
    buf[:N, :D2] = torch.from_numpy(c["z"]).to(DEV)
    view = buf[:N, :D2]
    assert view.stride(0) == 160 and view.data_ptr() % 16 == 0
    loss, dth, sums, dz, dP, dQ = host(run(c, z=view))
    for a in (loss, dth, sums, dz, dP, dQ):
        assert np.all(np.isfinite(a))
    share = check_sums(sums, c, "padded")
    check_scalars(sums, float(loss), dth.astype(np.float64), c, "padded")
    print(f"pad rows 1e30, identical rows: sums {share:.2g} of the bound; fp32 units", check_grads(dz, dP, dQ, c, "padded"))


def test_saturated_scores_stay_finite():
    """alpha |theta - s| up to 1e3: every output finite, the loss within 2^-20 of the reference; no ratio gate."""
    base = ar.case(ar.TILE + 1, 150, "softcdet", 2, "mixed")
    a = float(np.float32(base["alpha"]))
    smax = np.abs(base["r64"].s_pairs).max()
    f = (950.0 - a * max(abs(x) for x in base["theta"])) / (a * smax)
    c = _recase(base, (base["z"] * np.float32(np.sqrt(f))).astype(np.float32))
    assert 500.0 < ar.span_of(c) <= 1e3
    out = host(run(c))
    for x in out:
        assert np.all(np.isfinite(x))
    assert out[2][0] == c["r64"].Nt and out[2][1] == c["r64"].Nn
    assert abs(float(out[0]) - float(c["r64"].loss)) <= 2.0 ** -20 * abs(float(c["r64"].loss))


def test_degenerate_batches():
    from neuralplda_amd import ops
    ps, Q = torch.rand(150, device=DEV), -torch.rand(150, device=DEV)
    th = [torch.zeros(1, device=DEV), torch.ones(1, device=DEV)]
    for N, spk, grp in ((1, [3], None), (0, [], None), (4, [0, 0, 1, 1], [0, 1, 2, 3])):   # no trial at all
        z = torch.randn(N, 150, device=DEV)
        loss, dth, sums, dz, dP, dQ = ops.allpairs_loss(z, spk, ps, Q, th, [99.0, 199.0], 15.0, 0, grp=grp)
        assert torch.isnan(loss) and not sums.any() and not dz.any() and not dP.any() and not dQ.any()
        assert dz.shape == (N, 150)


def test_repeatable_and_capturable():
    """Two calls give the same bits in every output, and so does one call captured in a graph and replayed once."""
    from neuralplda_amd import ops
    c = ar.case(3 * ar.TILE + 17, 170, "softcdet", 4, "groups")
    a, b = host(run(c)), host(run(c))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    z, spk, grp = _dev(c["z"]), _dev(c["spk"]).to(torch.int32), _dev(c["grp"]).to(torch.int32)
    ps, Q, th = _dev(c["P_sqrt"]), _dev(c["Q"]), _thetas(c)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.allpairs_loss(z, spk, ps, Q, th, c["beta"], c["alpha"], 0, grp=grp)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, host(out)):
        assert np.array_equal(x, y)


# ---- model level --------------------------------------------------------------------------------------------------------------------

class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


THETA0 = (-0.8, -0.6)
HEAD_KEYS = ("centering_and_LDA.weight", "centering_and_LDA.bias", "centering_and_wccn_plda.weight",
             "centering_and_wccn_plda.bias", "P_sqrt", "Q")


def _restated(x, head, ii, jj, t, dtype):
    """The plain formulas (utils/models.py:366-388) on the explicit pair list, torch autograd on the CPU in `dtype`:
    {name: gradient} with the loss under "loss"."""
    X = torch.tensor(x, dtype=dtype, requires_grad=True)
    H = {k: torch.tensor(head[k], dtype=dtype, requires_grad=True) for k in HEAD_KEYS}
    th = [torch.tensor([v], dtype=torch.float32).to(dtype).requires_grad_(True) for v in THETA0]
    u = X @ H["centering_and_LDA.weight"].T + H["centering_and_LDA.bias"]
    y = u / u.norm(dim=1, keepdim=True).clamp_min(1e-12)
    z = y @ H["centering_and_wccn_plda.weight"].T + H["centering_and_wccn_plda.bias"]
    z1, z2 = z[torch.from_numpy(ii)], z[torch.from_numpy(jj)]
    s = (H["Q"] * (z1 * z1 + z2 * z2)).sum(1) + 2 * (H["P_sqrt"] * H["P_sqrt"] * z1 * z2).sum(1)
    T = torch.tensor(t, dtype=dtype)
    L = 0
    for thk, b in zip(th, NC.beta):
        L = L + (torch.sigmoid(NC.alpha * (thk - s)) * T).sum() / T.sum() + b * (torch.sigmoid(NC.alpha * (s - thk)) * (1 - T)).sum() / (1 - T).sum()
    L = L / len(th)
    L.backward()
    out = {k: v.grad.numpy() for k, v in H.items()}
    out.update(x=X.grad.numpy(), loss=np.array([L.item()]), **{f"Th{int(b)}": thk.grad.numpy() for b, thk in zip(NC.beta, th)})
    return out


def _model(head):
    from neuralplda_amd import models
    from tests import xvec_ref
    m = xvec_ref.load_into(models.NeuralPlda(NC()), head).to(DEV).train()
    with torch.no_grad():
        for b, v in zip(m.beta, THETA0):
            m.threshold[b].fill_(v)
    return m


def _grads(m, x, loss):
    m.zero_grad(set_to_none=True)
    x.grad = None
    loss.backward()
    sd = dict(m.named_parameters())
    out = {k: sd[k].grad.cpu().numpy() for k in HEAD_KEYS + tuple(f"Th{int(b)}" for b in m.beta)}
    out.update(x=x.grad.cpu().numpy(), loss=np.array([loss.item()]))
    return out


def test_model_loss_all_pairs_against_autograd_on_the_pair_list():
    from neuralplda_amd import ops
    from tests import synth, xvec_ref
    N = ops.ALLPAIRS_TILE + 1
    head = xvec_ref.make_head()
    D1 = 150
    rng = np.random.default_rng(5)
    x, _ = synth.speaker_structured_xvectors(head["centering_and_LDA.weight"], head["centering_and_LDA.bias"],
                                             np.linalg.qr(rng.standard_normal((D1, D1)))[0], np.zeros(D1),
                                             4.0 / (1 + np.arange(D1)), N // 9 + 1, 9)
    x = np.ascontiguousarray(x[:N])
    spk, _ = ar.labels(N, "mixed")
    trial, target = ar.masks(spk)
    ii, jj = np.nonzero(trial)
    t = target[ii, jj].astype(np.float32)
    ref64, ref32 = _restated(x, head, ii, jj, t, torch.float64), _restated(x, head, ii, jj, t, torch.float32)
    m = _model(head)
    X = torch.from_numpy(x).to(DEV).requires_grad_(True)
    new = _grads(m, X, m.loss_all_pairs(X, spk.tolist()))
    I, J = torch.from_numpy(ii).to(DEV), torch.from_numpy(jj).to(DEV)
    old = _grads(m, X, m.loss(m(X[I], X[J]), torch.from_numpy(t).to(DEV)))
    for name, got in (("loss_all_pairs", new), ("loss(forward(x[i], x[j]), t)", old)):
        worst = (0.0, 0.0)
        for k in ref64:
            r = fu.assert_fp32_level(got[k], ref64[k], ref32[k], f"{name} {k}")["all"]
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        print(f"{name}: worst fp32 units over the loss and nine gradients: rms {worst[0]:.2f} max {worst[1]:.2f}")
    # labels as a tensor on another device than x; a data-parallel model is refused
    again = m.loss_all_pairs(X, torch.from_numpy(spk))
    assert again.item() == new["loss"][0]
    m._reduce_flat = lambda flat: flat
    with pytest.raises(NotImplementedError):
        m.loss_all_pairs(X, spk.tolist())
    m._reduce_flat = None


def test_end_to_end_each_utterance_is_extracted_once():
    from neuralplda_amd import models
    from tests import xvec_grad_ref as gref, xvec_ref
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    xvec_ref.load_into(e.xvector_extractor, xvec_ref.make_params())
    xvec_ref.load_into(e, xvec_ref.make_head())
    e = e.to(DEV).train1(finetune_extractor=True)
    with torch.no_grad():
        for b, v in zip(e.beta, THETA0):
            e.threshold[b].fill_(v)
    rng = np.random.default_rng(11)
    feats = torch.from_numpy(rng.standard_normal((6, 30, 28)).astype(np.float32)).to(DEV)   # 24 is the shortest: plus 4
    spk = [0, 0, 1, 1, 2, 2]
    ii, jj = np.triu_indices(6, 1)
    t = torch.tensor([float(spk[i] == spk[j]) for i, j in zip(ii, jj)], device=DEV)

    def grads(loss):
        e.zero_grad(set_to_none=True)
        loss.backward()
        sd = dict(e.named_parameters())
        return {k: sd["xvector_extractor." + k].grad.cpu().numpy() for k in gref.GRAD_KEYS}, loss.item()

    ext = e.xvector_extractor
    rows, inner = [], ext.extract
    ext.extract = lambda x: (rows.append(x.shape[0]), inner(x))[1]
    try:
        new, lnew = grads(e.loss_all_pairs(feats, spk))
        assert rows == [6]
        del rows[:]
        old, lold = grads(e.loss(e(feats[torch.from_numpy(ii).to(DEV)], feats[torch.from_numpy(jj).to(DEV)]), t))
        assert rows == [15, 15]
    finally:
        del ext.extract
    assert abs(lnew - lold) <= 1e-4 * abs(lold)
    for k in gref.GRAD_KEYS:
        assert np.abs(new[k] - old[k]).max() <= 1e-4 * np.abs(old[k]).max(), k
