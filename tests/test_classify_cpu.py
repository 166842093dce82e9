"""The speaker-classification loss without a GPU: the numpy twin of tests/classify_ref.py against torch autograd, the float32
unit in a second summation order on the inputs tests/test_classify_gpu.py uses, the argument checks of the C entry point,
the workspace size and the register budget of csrc/nplda_classify.hip.

Measured here (float32 twin with every sum in 16-term pieces, in units of the plain float32 twin's error, worst over the 24
cases and the row regions; printed with -s): dX 1.01 rms / 1.07 max, dW 1.02 / 1.03, db 1.10 / 1.05, rowloss (N >= 64)
1.01 / 1.00; below 64 rows the float32 twin's rowloss lies within 0.043 of the absolute bound and its gradients within 0.010
of theirs."""
import ctypes

import numpy as np
import pytest
import torch

from neuralplda_amd import sv_trials_loaders
from tests import classify_ref as cr
from tests import fp32_units as fu
from tests.test_allpairs_cpu import _resources, _table

CASES = list(cr.cases())
IDS = ["-".join(map(str, c)) for c in CASES]


# ---- the float64 twin is the gradient of the literal composition ------------------------------------------------------------------

@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("shape", [(65, 17, 150), (30, 257, 40), (2, 3, 150)])
def test_float64_twin_equals_autograd(shape, kind):
    c = cr.case(*shape, kind)
    r = c["r64"]
    X = torch.tensor(c["X"].astype(np.float64), requires_grad=True)
    W = torch.tensor(c["W"].astype(np.float64), requires_grad=True)
    b = None if c["b"] is None else torch.tensor(c["b"].astype(np.float64), requires_grad=True)
    y = torch.tensor(c["y"].astype(np.int64))
    L, u = cr.torch_loss(X, W, b, y, kind, c["s"], c["m"])
    L.backward()
    if kind == 2:  # the clamp and the floor of the sine are not active: the two definitions coincide
        ut = r.U[r.valid, c["y"][r.valid]]
        assert np.abs(ut).max() <= 0.95
    assert abs(L.item() - r.loss) <= 1e-10 * abs(L.item())
    for name, got, ref in (("dX", r.dX, X.grad), ("dW", r.dW, W.grad)) + ((("db", r.db, b.grad),) if b is not None else ()):
        ref = ref.numpy()
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (shape, kind, name)
    assert np.array_equal(r.pred, (float(np.float32(c["s"])) * u.detach().numpy() + (0 if b is None else c["b"])).argmax(1))
    valid = r.valid
    assert r.counts[0] == valid.sum() and r.counts[2] == 0
    assert np.all(r.rowloss[~valid] == 0)


def test_twin_counts_ignored_and_bad_labels():
    X, W, b, y = cr.draw(20, 7, 16, seed=3)
    y = y.copy()
    y[1], y[2], y[5] = 7, -7, -1
    r = cr.classify(X, y, W, b, 2, 30.0, 0.2)
    assert r.counts[0] == 20 - 3 - (1 if 20 // 3 not in (1, 2, 5) else 0) and r.counts[2] == 2
    for i in (1, 2, 5):
        assert r.rowloss[i] == 0 and not r.dX[i].any()
    r0 = cr.classify(X, np.full(20, -1), W, b, 1, 30.0, 0.2)
    assert np.isnan(r0.loss) and not r0.dX.any() and not r0.dW.any() and not r0.db.any()
    assert np.array_equal(r0.pred, r.pred)   # margin-free: the labels do not enter


# ---- the float32 unit on the GPU test's inputs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", CASES, ids=IDS)
def test_float32_twin_in_a_second_order_meets_the_gates(cs):
    """The float32 twin with every sum in 16-term pieces stays inside the default gates (3 rms / 5 max fp32 units) of the plain
    float32 twin, over all rows and the row-tile regions: no output needs a wider gate on the GPU.  Below 64 rows a ratio
    is a draw: there the float32 twin must lie within a quarter of the absolute bounds the GPU test applies."""
    N, C, D, kind, cc, rc = cs
    c = cr.case(N, C, D, kind, cc, rc)
    r64, r32 = c["r64"], c["r32"]
    assert cr.gap_of(r64) > cr.GAP
    if kind and D >= 100:
        ut = r64.U[r64.valid, c["y"][r64.valid]]
        assert ut.min() > 0.25 and ut.max() < 0.75   # class centroids plus noise: the cosines an extractor's head sees
    alt = cr.classify(c["X"], c["y"], c["W"], c["b"], kind, c["s"], c["m"], np.float32, chunk=16)
    assert np.array_equal(alt.pred, r64.pred) and np.array_equal(r32.pred, r64.pred)
    assert np.array_equal(alt.counts, r64.counts)
    if N >= 64:
        out = {}
        for name, regions in (("dX", fu.Regions(N, 64)), ("dW", None), ("db", None), ("rowloss", fu.Regions(N, 64))):
            if name == "db" and c["b"] is None:
                continue
            r = fu.assert_fp32_level(getattr(alt, name), getattr(r64, name), getattr(r32, name), f"{cs} {name} (16-term pieces)",
                                     regions)
            out[name] = tuple(round(max(v[k] for v in r.values()), 2) for k in (0, 1))
        print(cs, out)
    else:
        rb, gb = cr.small_bounds(c)
        share = {"rowloss": float((np.abs(r32.rowloss - r64.rowloss) / rb).max())}
        for k, bound in gb.items():
            share[k] = float(np.abs(getattr(r32, k) - getattr(r64, k)).max() / bound) if bound > 0 else 0.0
        print(cs, "float32 twin, share of the absolute bounds:", {k: round(v, 3) for k, v in share.items()})
        assert all(v <= 0.25 for v in share.values()), share


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_abi_argument_checks(hip_lib):
    EINVAL, EUNSUP, ENOSPC = -22, -95, -28
    L = hip_lib
    dummy = ctypes.create_string_buffer(4096)
    p16 = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40

    def call(X=p16, ldx=152, N=8, W=p16, ldw=152, C=5, D=150, b=p16, y=p16, kind=2, s=30.0, m=0.2, cc=0, rc=0, loss=p16,
             counts=p16, rowloss=p16, pred=p16, dX=p16, lddx=152, dW=p16, lddw=152, db=p16, ws=p16, wsb=big):
        return L.nplda_classify_loss_f32(X, ldx, N, W, ldw, C, D, b, y, kind, s, m, cc, rc, loss, counts, rowloss, pred, dX,
                                         lddx, dW, lddw, db, ws, wsb, None)

    need = L.nplda_classify_workspace_bytes(8, 5, 150, 0, 0)
    assert need > 2 * 64 * 160 * 4 and need % 256 == 0
    assert call(N=0) == 0 and call(C=0) == 0                   # no-ops: nothing is launched
    for kw in (dict(X=None), dict(W=None), dict(y=None), dict(loss=None), dict(counts=None), dict(ws=None)):
        assert call(**kw) == EINVAL, kw
    assert call(kind=-1) == EINVAL and call(kind=3) == EINVAL
    assert call(s=0.0) == EINVAL and call(s=-1.0) == EINVAL and call(s=float("nan")) == EINVAL
    assert call(m=-0.1) == EINVAL and call(kind=0, m=0.2) == EINVAL and call(kind=2, m=3.2) == EINVAL
    assert call(kind=1, m=3.2, N=0) == 0                        # AM-softmax has no upper limit on the margin
    assert call(N=-1) == EINVAL and call(C=-1) == EINVAL and call(D=0) == EINVAL and call(cc=-1) == EINVAL and call(rc=-1) == EINVAL
    assert call(X=p16 + 4) == EINVAL and call(W=p16 + 8) == EINVAL and call(ws=p16 + 4) == EINVAL
    assert call(ldx=150) == EINVAL and call(ldx=148) == EINVAL and call(ldw=150) == EINVAL and call(ldw=148) == EINVAL
    assert call(dX=p16 + 4) == EINVAL and call(lddx=150) == EINVAL and call(dW=p16 + 8) == EINVAL and call(lddw=148) == EINVAL
    assert call(D=193, ldx=196, ldw=196, lddx=196, lddw=196) == EUNSUP
    assert call(N=(1 << 20) + 1) == EUNSUP and call(C=(1 << 20) + 1) == EUNSUP
    assert call(wsb=need - 1) == ENOSPC and call(wsb=0) == ENOSPC
    assert call(cc=3, rc=2, wsb=L.nplda_classify_workspace_bytes(8, 5, 150, 3, 2) - 1) == ENOSPC
    assert call(b=None, rowloss=None, pred=None, dX=None, dW=None, db=None, N=0) == 0   # every one of them is optional


def test_workspace_size(hip_lib):
    wsb = hip_lib.nplda_classify_workspace_bytes
    assert wsb(-1, 5, 150, 0, 0) == 0 and wsb(5, -1, 150, 0, 0) == 0 and wsb(8, 5, 193, 0, 0) == 0 and wsb(8, 5, 0, 0, 0) == 0
    assert wsb((1 << 20) + 1, 5, 150, 0, 0) == 0 and wsb(5, (1 << 20) + 1, 150, 0, 0) == 0 and wsb(8, 5, 150, -1, 0) == 0
    assert wsb(1 << 20, 1 << 20, 192, 0, 0) > 0
    assert 0 < wsb(0, 5, 150, 0, 0) <= wsb(1, 5, 150, 0, 0) and 0 < wsb(5, 0, 150, 3, 2) <= wsb(5, 1, 150, 3, 2)   # empty problems
    # monotone in N and in C, through every change of the chunk plan
    sizes = sorted(set(list(range(1, 300, 7)) + [2 ** k + d for k in range(6, 21) for d in (-1, 0, 1) if 2 ** k + d <= 1 << 20]
                       + list(range(300, 40000, 611))))
    for other in (1, 1000, 7323, 13539, 1 << 20):
        for D in (8, 150):
            by_n = [wsb(n, other, D, 0, 0) for n in sizes]
            by_c = [wsb(other, n, D, 0, 0) for n in sizes]
            assert all(a <= b for a, b in zip(by_n, by_n[1:])) and all(a <= b for a, b in zip(by_c, by_c[1:])), (other, D)
            assert all(v > 0 and v % 256 == 0 for v in by_n + by_c)
    assert wsb(70, 100, 150, 7, 2) > wsb(70, 100, 150, 3, 2) > wsb(70, 100, 150, 1, 1)
    # nothing grows with N * C: an eighth of the fp32 logits at the reference's class count
    assert wsb(16384, 13539, 150, 0, 0) < 16384 * 13539 * 4 // 8
    assert wsb(1024, 7323, 150, 0, 0) < 1024 * 7323 * 4


def test_speaker_batch_loader_labels_index_its_speakers():
    table, spk2utt = _table()
    ld = sv_trials_loaders.SpeakerBatchLoader(table, spk2utt, 3, 3, seed=5)
    assert ld.num_speakers == len(ld.speakers) > 3
    for _, spk, _ in ld:
        assert spk.min() >= 0 and spk.max() < ld.num_speakers


# ---- kernel resources --------------------------------------------------------------------------------------------------------------

def test_register_budget_of_the_classify_kernels():
    """design/k26_classify.md plans two blocks of four waves per CU for the MFMA kernel, as the all-pairs step does: at most
    256 registers, no scratch, two blocks' LDS within 160 KB; no kernel of the file uses scratch."""
    res = _resources("nplda_classify.hip")
    main = {k: v for k, v in res.items() if "cl_mainILi" in k}
    assert len(main) == 6 * 3, sorted(res)   # NB in {2, 4, 8, 10, 11, 12} x {LSE, GRAD rows own, GRAD classes own}
    for k, v in main.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
        assert 2 * v["LDS"] <= 160 * 1024, (k, v)
    rest = {k: v for k, v in res.items() if k not in main}
    assert len(rest) == 4, sorted(res)       # pad, merge, scalars, finish
    for k, v in rest.items():
        assert v["ScratchSize"] == 0, (k, v)
