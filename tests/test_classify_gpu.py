"""The speaker-classification loss (csrc/nplda_classify.hip, ops.classify_loss, models.SpeakerClassifier,
NeuralPlda.loss_classify) on the MI355X against tests/classify_ref.py: the numpy twin in float64, with its float32 evaluation
as the unit (tests/fp32_units.py).

Shapes (classify_ref.SHAPES) x the three kinds (softmax s = 0.05; AM and AAM s = 30, m = 0.2): (N, C, D) = (1, 1, 150),
(2, 3, 150), (65, 17, 150), (130, 257, 170), (100, 1000, 150), (257, 300, 192), (64, 64, 8) under the plan's chunks and
(70, 100, 150) under class_chunks = 3, row_chunks = 2 (ragged last chunks).  Inputs: class centroids plus noise, one label of
-1 where N > 4, the seed redrawn until the float64 twin's best and second-best inference logits differ by more than 1e-4 of
max |a| in every row.

Checks: counts[0], counts[2] exact; pred and counts[1] equal the twin's; loss equal to the fp64 sum of the device's own rowloss
over the counted rows (in the device's order) divided by their number, rounded once; dX (all rows and the row-tile regions), dW, db
and rowloss at the default gates 3 (rms) / 5 (max) fp32 units where N >= 64 — tests/test_classify_cpu.py holds the float32
twin in a second summation order to the same gates, so none is widened; below 64 rows finiteness and the absolute bounds of
classify_ref.small_bounds (rowloss: 16 * 2^-24 * max(1, max_c |l_ic|); the CPU test holds the float32 twin to a quarter of
each).

Ties (test 3): with two bitwise-equal rows of W the rowloss under label 5 is bitwise the rowloss under label 40 for kind 0,
where both calls sum the same numbers in the same places.  Under a margin the target's logit moves to another place of the
fixed summation order (class 5 and class 40 lie on different lanes and tiles), so the two sums of exponentials are the same
numbers in two orders: equal to a few 2^-24 of lse, which is what is asserted there, not to the bit.

Measured on MI355X (each test prints its figures with -s):

    check                                                                        measured
    ---------------------------------------------------------------------------  ---------------------------------
    dX, rms / max fp32 units over the 24 cases and the row-tile regions          0.44 - 1.16 / 0.46 - 1.10
    dW; db                                                                       0.43 - 1.01 / 0.33 - 1.28; 0.40 - 1.07 / 0.31 - 1.08
    rowloss (N >= 64)                                                            0.41 - 1.36 / 0.27 - 2.18
    below 64 rows, share of the absolute bounds: rowloss; dX, dW, db             <= 0.043; <= 0.010
    chunk plans (1, 1), (3, 2), (7, 2) at (70, 100, 150), worst of all outputs   0.80 / 1.06
    pad columns 1e30, strided views; labels C and -7                             <= 1.00 / 1.27; <= 1.30 / 2.18
    NeuralPlda.loss_classify, worst of the loss and six gradients                1.55 / 1.48
"""
import numpy as np
import pytest
import torch

from tests import classify_ref as cr
from tests import fp32_units as fu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = torch.device("cuda:0")
KNAME = {0: "softmax", 1: "am", 2: "aam"}
CASES = list(cr.cases())
IDS = ["-".join(map(str, c)) for c in CASES]


def _dev(a):
    return None if a is None else torch.tensor(a).to(DEV)  # (a copy: the shared cases are read-only arrays)


def run(c, y=None, X=None, W=None, **kw):
    from neuralplda_amd import ops
    kw.setdefault("class_chunks", c["class_chunks"])
    kw.setdefault("row_chunks", c["row_chunks"])
    return ops.classify_loss(_dev(c["X"]) if X is None else X, _dev(c["y"] if y is None else y),
                             _dev(c["W"]) if W is None else W, _dev(c["b"]), kind=KNAME[c["kind"]], scale=c["s"],
                             margin=c["m"], **kw)


def host(out):
    return type(out)(*[None if t is None else t.detach().cpu().numpy() for t in out])


def device_order_mean(rowloss, valid):
    """The fp64 sum of rowloss over the counted rows as the device forms it — rows in order inside blocks of 256, the blocks
    in order — divided by their number."""
    tot = 0.0
    for o in range(0, rowloss.size, 256):
        acc = 0.0
        for v, ok in zip(rowloss[o:o + 256], valid[o:o + 256]):
            if ok:
                acc += float(v)
        tot += acc
    return tot / int(valid.sum()) if valid.any() else float("nan")


def check(out, c, what, r64=None, r32=None, gates=True):
    """Everything test 1 asserts about one call -> the worst (rms, max) ratios per output."""
    r64 = c["r64"] if r64 is None else r64
    r32 = c["r32"] if r32 is None else r32
    N = r64.rowloss.size
    assert out.counts[0] == r64.counts[0] and out.counts[2] == r64.counts[2], (what, out.counts, r64.counts)
    assert np.array_equal(out.pred, r64.pred), (what, np.flatnonzero(out.pred != r64.pred))
    assert out.counts[1] == r64.counts[1], (what, out.counts, r64.counts)
    for a in (out.rowloss, out.dx, out.dw, out.db):
        assert a is None or np.all(np.isfinite(a)), what
    assert np.all(out.rowloss[~r64.valid] == 0), what
    if r64.valid.any():
        mean = device_order_mean(out.rowloss, r64.valid)
        assert abs(float(out.loss) - float(np.float32(mean))) <= 1e-12 * abs(mean), (what, float(out.loss), mean)
    else:
        assert np.isnan(out.loss), what
    res = {}
    pairs = [("rowloss", out.rowloss, True), ("dX", out.dx, True), ("dW", out.dw, False), ("db", out.db, False)]
    if N >= 64 and gates:
        for name, got, by_rows in pairs:
            if got is None:
                continue
            r = fu.assert_fp32_level(got, getattr(r64, name), getattr(r32, name), f"{what} {name}",
                                     fu.Regions(N, 64) if by_rows else None)
            res[name] = tuple(round(max(v[k] for v in r.values()), 2) for k in (0, 1))
    elif gates:
        rb, gb = cr.small_bounds(c)
        err = np.abs(out.rowloss - r64.rowloss)
        assert np.all(err <= rb), (what, err / rb)   # 16 * 2^-24 * max(1, max_c |l_ic|); the float32 twin uses 0.043 of it
        res["rowloss"] = round(float((err / rb).max()), 3)
        for name, got, _ in pairs[1:]:
            if got is None:
                continue
            e = float(np.abs(got - getattr(r64, name)).max())
            assert e <= gb[name], (what, name, e, gb[name])
            res[name] = round(e / gb[name], 3) if gb[name] > 0 else 0.0
    return res


# ---- 1. against the twin ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_against_the_twin(cs):
    N, C, D, kind, cc, rc = cs
    c = cr.case(N, C, D, kind, cc, rc)
    assert cr.gap_of(c["r64"]) > cr.GAP
    assert (c["y"] == -1).sum() == (1 if N > 4 else 0)
    out = host(run(c))
    assert out.dx.shape == (N, D) and out.dw.shape == (C, D) and out.rowloss.shape == out.pred.shape == (N,)
    assert (out.db is None) == (c["b"] is None)
    print(cs, "fp32 units (rms, max) or share of the absolute bound:", check(out, c, str(cs)))


# ---- 2. chunking --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 1, 2])
def test_chunk_plans_agree_and_calls_repeat(kind):
    c = cr.case(70, 100, 150, kind)
    outs = {plan: host(run(c, class_chunks=plan[0], row_chunks=plan[1])) for plan in ((1, 1), (3, 2), (7, 2))}
    first = outs[(1, 1)]
    for plan, out in outs.items():
        assert np.array_equal(out.pred, first.pred) and np.array_equal(out.counts, first.counts), plan
        print(kind, plan, check(out, c, f"kind {kind} plan {plan}"))
    again = host(run(c, class_chunks=3, row_chunks=2))
    for a, b in zip(outs[(3, 2)], again):
        assert np.array_equal(a, b)


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 1, 2])
def test_equal_classes_resolve_to_the_lower_index(kind):
    N, C, D = 70, 50, 150
    X, W, _, y = cr.draw(N, C, D, seed=77 + kind, bias=False)
    W = W.copy()
    W[40] = W[5]
    y = y.copy()
    y[y == 40] = 7
    y[::7] = 5
    X = (W[np.where(y >= 0, y, 0)] + 1.5 * np.random.default_rng(5).standard_normal((N, D))).astype(np.float32)
    c = dict(X=X, W=W, b=None, y=y, kind=kind, s=cr.SCALE[kind], m=cr.MARGIN[kind], class_chunks=0, row_chunks=0)
    a = host(run(c))
    assert not (a.pred == 40).any() and (a.pred[y == 5] == 5).all()
    y2 = np.where(y == 5, 40, y).astype(np.int32)
    b = host(run(c, y=y2))
    assert not (b.pred == 40).any() and np.array_equal(a.pred, b.pred)
    rows = y == 5
    if kind == 0:
        assert np.array_equal(a.rowloss[rows], b.rowloss[rows])
    else:  # (the module docstring: the same exponentials in two orders)
        r64 = cr.classify(X, y, W, None, kind, c["s"], c["m"])
        tol = 4 * U * np.maximum(1.0, np.abs(r64.lse[rows]))
        assert np.all(np.abs(a.rowloss[rows] - b.rowloss[rows]) <= tol)
    assert np.array_equal(a.rowloss[~rows], b.rowloss[~rows])


# ---- 4. nothing leaks ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 2])
def test_nothing_leaks_from_pad_columns_or_pad_rows(kind):
    """X and W are views with row stride 160 over buffers whose pad columns hold 1e30 (N = 65, C = 17: no multiples of the
    tiles), through the C call with the caller's own dX / dW of stride 160 pre-filled with a sentinel."""
    from neuralplda_amd import _lib
    N, C, D, ld = 65, 17, 150, 160
    c = cr.case(N, C, D, kind)
    lib = _lib.load()
    xb = torch.full((N + 3, ld), 1e30, dtype=torch.float32, device=DEV)
    wb = torch.full((C + 3, ld), 1e30, dtype=torch.float32, device=DEV)
    xb[:N, :D] = _dev(c["X"])
    wb[:C, :D] = _dev(c["W"])
    SENT = -7.5
    dxb = torch.full((N + 3, ld), SENT, dtype=torch.float32, device=DEV)
    dwb = torch.full((C + 3, ld), SENT, dtype=torch.float32, device=DEV)
    db = torch.full((C + 3,), SENT, dtype=torch.float32, device=DEV)
    rowloss = torch.full((N + 3,), SENT, dtype=torch.float32, device=DEV)
    pred = torch.full((N + 3,), -9, dtype=torch.int32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    counts = torch.empty(3, dtype=torch.int64, device=DEV)
    y, b = _dev(c["y"]), _dev(c["b"])
    wsb = lib.nplda_classify_workspace_bytes(N, C, D, 0, 0)
    ws = torch.full((wsb // 4,), float("nan"), dtype=torch.float32, device=DEV)   # every word that is read was written first
    code = lib.nplda_classify_loss_f32(xb.data_ptr(), ld, N, wb.data_ptr(), ld, C, D, b.data_ptr(), y.data_ptr(), kind,
                                       c["s"], c["m"], 0, 0, loss.data_ptr(), counts.data_ptr(), rowloss.data_ptr(),
                                       pred.data_ptr(), dxb.data_ptr(), ld, dwb.data_ptr(), ld, db.data_ptr(), ws.data_ptr(),
                                       wsb, _lib.current_stream())
    assert code == 0
    torch.cuda.synchronize()
    from neuralplda_amd import ops
    out = host(ops.ClassifyResult(loss, counts, rowloss[:N], pred[:N], dxb[:N, :D], dwb[:C, :D], db[:C]))
    print(kind, "pad columns 1e30:", check(out, c, f"padded kind {kind}"))
    for buf, n in ((dxb, N), (dwb, C)):
        buf = buf.cpu().numpy()
        assert np.all(buf[:, D:] == SENT) and np.all(buf[n:] == SENT)
    assert np.all(db.cpu().numpy()[C:] == SENT) and np.all(rowloss.cpu().numpy()[N:] == SENT)
    assert np.all(pred.cpu().numpy()[N:] == -9)


# ---- 5. ignored and bad labels ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 1, 2])
def test_ignored_and_bad_labels(kind):
    c = cr.case(65, 17, 150, kind)
    out = host(run(c, y=np.full(65, -1, np.int32)))
    assert np.isnan(out.loss) and np.array_equal(out.counts, [0, 0, 0])
    assert not out.dx.any() and not out.dw.any() and not out.db.any() and not out.rowloss.any()
    assert np.array_equal(out.pred, c["r64"].pred)
    y = c["y"].copy()
    y[3], y[64] = 17, -7
    r64 = cr.classify(c["X"], y, c["W"], c["b"], kind, c["s"], c["m"], np.float64)
    r32 = cr.classify(c["X"], y, c["W"], c["b"], kind, c["s"], c["m"], np.float32)
    out = host(run(c, y=y))
    assert out.counts[2] == 2 and out.counts[0] == 65 - 3
    assert not out.dx[3].any() and not out.dx[64].any() and out.rowloss[3] == 0 and out.rowloss[64] == 0
    print(kind, "bad labels:", check(out, c, f"bad labels kind {kind}", r64, r32))


def test_empty_problems():
    """N == 0 or C == 0: the C call is a no-op and ops fills in the formulas on an empty problem."""
    from neuralplda_amd import ops
    W = torch.randn(17, 150, device=DEV)
    out = ops.classify_loss(torch.empty(0, 150, device=DEV), [], W, kind="aam")
    assert torch.isnan(out.loss) and not out.counts.any() and out.dx.shape == (0, 150) and out.rowloss.shape == (0,)
    assert out.dw.shape == (17, 150) and not out.dw.any() and out.db is None
    out = ops.classify_loss(torch.randn(5, 150, device=DEV), [-1] * 5, torch.empty(0, 150, device=DEV), kind="softmax", margin=0.0)
    assert torch.isnan(out.loss) and not out.counts.any() and not out.dx.any() and out.dw.shape == (0, 150)


# ---- 6. range -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 1, 2])
def test_large_logits_and_cosines_of_one_stay_finite(kind):
    N, C, D = 70, 33, 150
    rng = np.random.default_rng(31 + kind)
    W = rng.standard_normal((C, D)).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int32)
    if kind == 0:   # <x_i, w_y> about 1e3 with s = 1
        X, s, m = (W[y] * np.float32(1000.0 / D)).astype(np.float32), 1.0, 0.0
    else:           # cosines of +1 and -1 at s = 64
        X, s, m = (W[y] * np.where(np.arange(N) % 2, -1.0, 1.0)[:, None]).astype(np.float32), 64.0, 0.2
    c = dict(X=X, W=W, b=None, y=y, kind=kind, s=s, m=m, class_chunks=0, row_chunks=0)
    r64 = cr.classify(X, y, W, None, kind, s, m, np.float64)
    assert np.abs(r64.l).max() > (900.0 if kind == 0 else 60.0)
    out = host(run(c))
    for a in out:
        assert a is None or np.all(np.isfinite(a))
    assert np.array_equal(out.counts[[0, 2]], r64.counts[[0, 2]])
    assert r64.loss > 1e-3 or kind == 0
    if r64.loss > 1e-3:
        assert abs(float(out.loss) - r64.loss) <= 2.0 ** -20 * abs(r64.loss), (float(out.loss), r64.loss)


# ---- 7. optional outputs ------------------------------------------------------------------------------------------------------------

def test_optional_outputs_do_not_change_the_others():
    c = cr.case(130, 257, 170, 2)
    full = host(run(c))
    for kw in (dict(want_dx=False), dict(want_dw=False), dict(want_dx=False, want_dw=False)):
        out = host(run(c, **kw))
        assert (out.dx is None) == (not kw.get("want_dx", True))
        assert (out.dw is None) == (out.db is None) == (not kw.get("want_dw", True))
        for a, b in zip(full, out):
            assert b is None or np.array_equal(a, b), kw


# ---- 8. capturable ------------------------------------------------------------------------------------------------------------------

def test_repeatable_and_capturable():
    """Two calls give the same bits in every output, and so does one call captured in a graph and replayed twice."""
    from neuralplda_amd import ops
    c = cr.case(257, 300, 192, 2)
    a, b = host(run(c)), host(run(c))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    X, W, bias, lab = _dev(c["X"]), _dev(c["W"]), _dev(c["b"]), _dev(c["y"]).to(torch.int32)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.classify_loss(X, lab, W, bias, kind="aam", scale=c["s"], margin=c["m"])
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(a, host(out)):
            assert np.array_equal(x, y)


# ---- 9. model level -----------------------------------------------------------------------------------------------------------------

class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


LAYER_KEYS = ("centering_and_LDA.weight", "centering_and_LDA.bias", "centering_and_wccn_plda.weight",
              "centering_and_wccn_plda.bias")


def _restated(x, head, Wc, y, dtype):
    """extract_plda_embeddings (utils/models.py:366-370) and the literal classification composition, torch autograd on the
    CPU in `dtype`: {name: gradient} with the loss under "loss"."""
    X = torch.tensor(x, dtype=dtype, requires_grad=True)
    H = {k: torch.tensor(head[k], dtype=dtype, requires_grad=True) for k in LAYER_KEYS}
    Wt = torch.tensor(Wc, dtype=dtype, requires_grad=True)
    u = X @ H["centering_and_LDA.weight"].T + H["centering_and_LDA.bias"]
    yv = u / u.norm(dim=1, keepdim=True).clamp_min(1e-12)
    z = yv @ H["centering_and_wccn_plda.weight"].T + H["centering_and_wccn_plda.bias"]
    L, _ = cr.torch_loss(z, Wt, None, torch.tensor(y, dtype=torch.int64), 2, 30.0, 0.2)
    L.backward()
    out = {k: v.grad.numpy() for k, v in H.items()}
    out.update(x=X.grad.numpy(), weight=Wt.grad.numpy(), loss=np.array([L.item()]))
    return out


def test_model_loss_classify_against_autograd():
    from neuralplda_amd import models
    from tests import synth, xvec_ref
    N, C, D1 = 65, 40, 150
    head = xvec_ref.make_head()
    rng = np.random.default_rng(5)
    x, _ = synth.speaker_structured_xvectors(head["centering_and_LDA.weight"], head["centering_and_LDA.bias"],
                                             np.linalg.qr(rng.standard_normal((D1, D1)))[0], np.zeros(D1),
                                             4.0 / (1 + np.arange(D1)), N // 9 + 1, 9)
    x = np.ascontiguousarray(x[:N]).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int32)
    y[7] = -1
    m = xvec_ref.load_into(models.NeuralPlda(NC()), head).to(DEV).train()
    torch.manual_seed(3)
    clf = models.SpeakerClassifier(C, 150, kind="aam", scale=30.0, margin=0.2).to(DEV)
    assert clf.weight.shape == (C, 150) and clf.bias is None
    Wc = clf.weight.detach().cpu().numpy()
    ref64, ref32 = _restated(x, head, Wc, y, torch.float64), _restated(x, head, Wc, y, torch.float32)
    X = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss = m.loss_classify(X, y.tolist(), clf)
    loss.backward()
    sd = dict(m.named_parameters())
    got = {k: sd[k].grad.cpu().numpy() for k in LAYER_KEYS}
    got.update(x=X.grad.cpu().numpy(), weight=clf.weight.grad.cpu().numpy(), loss=np.array([loss.item()]))
    worst = (0.0, 0.0)
    for k in ref64:
        r = fu.assert_fp32_level(got[k], ref64[k], ref32[k], f"loss_classify {k}")["all"]
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"loss_classify: worst fp32 units over the loss and six gradients: rms {worst[0]:.2f} max {worst[1]:.2f}")
    assert clf.last_counts.is_cuda and clf.last_pred.is_cuda and clf.last_pred.shape == (N,)
    assert clf.last_counts.tolist()[0] == N - 1 and clf.last_counts.tolist()[2] == 0
    # labels as a tensor on another device than x; no gradient wanted; a data-parallel model and DPlda are refused
    with torch.no_grad():
        again = m.loss_classify(X, torch.from_numpy(y), clf)
    assert again.item() == got["loss"][0] and not again.requires_grad
    m._reduce_flat = lambda flat: flat
    with pytest.raises(NotImplementedError):
        m.loss_classify(X, y.tolist(), clf)
    m._reduce_flat = None
    with pytest.raises(NotImplementedError):
        models.DPlda.loss_classify(m, X, y.tolist(), clf)


def test_end_to_end_each_utterance_is_extracted_once():
    from neuralplda_amd import models
    from tests import xvec_ref
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    xvec_ref.load_into(e.xvector_extractor, xvec_ref.make_params())
    xvec_ref.load_into(e, xvec_ref.make_head())
    e = e.to(DEV).train1(finetune_extractor=True)
    torch.manual_seed(4)
    clf = models.SpeakerClassifier(3, 150, kind="aam", bias=True).to(DEV)
    rng = np.random.default_rng(11)
    feats = torch.from_numpy(rng.standard_normal((6, 30, 28)).astype(np.float32)).to(DEV)
    ext = e.xvector_extractor
    rows, inner = [], ext.extract
    ext.extract = lambda x: (rows.append(x.shape[0]), inner(x))[1]
    try:
        loss = e.loss_classify(feats, [0, 0, 1, 1, 2, 2], clf)
        loss.backward()
        assert rows == [6]
    finally:
        del ext.extract
    sd = dict(e.named_parameters())
    for g in (sd["xvector_extractor.tdnn1.kernel.weight"].grad, clf.weight.grad, clf.bias.grad):
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    assert np.isfinite(loss.item())
