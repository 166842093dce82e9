"""ops.topk_scores (csrc/nplda_topk.hip), Gallery / NeuralPlda.identify and mine_hard_trials on the GPU against the numpy
oracle of tests/topk_ref.py: exact cases bit for bit (ties included), float cases at fp32 level with the a-priori selection
tolerance, whatever the chunking."""
import numpy as np
import pytest
import torch

from tests import topk_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = "NPLDA_TOPK_MAX_CHUNKS"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_PACKED = {}


def packed_for(P_sqrt, Q):
    """A parameter image that carries P_sqrt, Q (the layers are not used by the search: D0 = 16, D1 = D2, zero weights)."""
    from neuralplda_amd import ops
    key = (P_sqrt.tobytes(), Q.tobytes())
    if key not in _PACKED:
        D2 = P_sqrt.size
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        _PACKED[key] = ops.pack_params(z(D2, 16), z(D2), z(D2, D2), z(D2), _dev(P_sqrt), _dev(Q))
    return _PACKED[key]


def run(c, largest, k=None, zr=None, zt=None, qt=None):
    from neuralplda_amd import ops
    packed = packed_for(c["P_sqrt"], c["Q"])
    assert packed.ldz == c["zt"].shape[1]
    labels = None if c["mask"] is None else (_dev(c["lab_r"]), _dev(c["lab_t"]))
    groups = None if c["grp_r"] is None else (_dev(c["grp_r"]), _dev(c["grp_t"]))
    sr = None if c["self_rows"] is None else _dev(c["self_rows"])
    vals, idx = ops.topk_scores(_dev(c["zr"]) if zr is None else zr, _dev(c["qr"]), _dev(c["zt"]) if zt is None else zt,
                                _dev(c["qt"]) if qt is None else qt, packed, c["k"] if k is None else k, largest=largest,
                                labels=labels, mask=c["mask"], groups=groups, self_rows=sr)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.is_cuda and idx.is_cuda
    return vals.cpu().numpy(), idx.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                 b.view(np.uint32) if b.dtype == np.float32 else b)


def assert_exact(got, ref, what):
    assert same_bits(got[1], ref[1]), (what, "idx", np.argwhere(got[1] != ref[1])[:5])
    assert same_bits(got[0], ref[0]), (what, "vals")


# ---- 1. exact cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("cs", tr.EXACT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_exact_cases_bit_for_bit(cs, largest):
    c = tr.exact_case(*cs)
    assert_exact(run(c, largest), c["ref"][largest], (cs, largest))


# ---- 2. float cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("cs", tr.FLOAT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_float_cases_at_fp32_level(cs, largest):
    """Measured on an MI355X: the returned values at 0.65 - 0.78 rms / 0.55 - 0.83 max float32 units of the float64 scores
    (the defaults 3 / 5 are asserted); 0 selection violations, the closest left-out column 0.23 of a tolerance BELOW the last
    returned value (a violation is above + 1)."""
    c = tr.float_case(*cs)
    vals, idx = run(c, largest)
    tr.check_float_result(vals, idx, c, largest, f"float case {cs} largest={largest}")


# ---- 3. chunk independence ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("largest", [True, False])
def test_chunking_does_not_change_a_bit(monkeypatch, largest):
    cases = [tr.exact_case(*cs) for cs in tr.EXACT_CASES if cs[3] == 3000] + [tr.float_case(*cs) for cs in tr.FLOAT_CASES]
    for c in cases:
        out = {}
        for cap in ("1", "3", None):     # one chunk, three, the default plan (47 chunks of 64 columns at M = 3000)
            if cap is None:
                monkeypatch.delenv(CAP, raising=False)
            else:
                monkeypatch.setenv(CAP, cap)
            out[cap] = run(c, largest)
        for cap in ("1", "3"):
            assert same_bits(out[cap][0], out[None][0]) and same_bits(out[cap][1], out[None][1]), (c["D2"], c["k"], cap)
        if "ref" in c:
            assert_exact(out["1"], c["ref"][largest], "one chunk")


# ---- 4. adversarial order ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", ["1", None])
def test_every_column_passes_the_threshold(monkeypatch, cap):
    """Row 0's scores ascend with the column (descend for odd rows): with largest = 1 every column beats the running
    threshold; the mirror rows do the same for smallest.  With ONE chunk (cap 1) a block walks all 256 tiles and every
    instantiation of the candidate lists (k = 16, 64, 128: 32, 128, 256 slots) overflows and is cut every k / 16 tiles, as
    often as it can be; the default plan (64 chunks of 64 columns) leaves the cutting of k >= 64 to the merge."""
    if cap is None:
        monkeypatch.delenv(CAP, raising=False)
    else:
        monkeypatch.setenv(CAP, cap)
    D2, M, R = 32, 4096, 17
    P_sqrt, Q = np.ones(D2, np.float32), np.zeros(D2, np.float32)
    zt, zr = np.zeros((M, 32), np.float32), np.zeros((R, 32), np.float32)
    zt[:, 0] = np.arange(M) / 64.0
    zt[:, 1] = (np.arange(M) % 5) / 8.0
    zr[:, 0] = np.where(np.arange(R) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(R) // 2 / 8.0)
    c = dict(D2=D2, k=128, R=R, M=M, mask=None, P_sqrt=P_sqrt, Q=Q, zr=zr, zt=zt, qr=np.zeros(R, np.float32),
             qt=np.zeros(M, np.float32), self_rows=None, lab_r=None, lab_t=None, grp_r=None, grp_t=None)
    S = tr.scores(zr, c["qr"], zt, c["qt"], P_sqrt, np.float32)
    assert np.array_equal(S.astype(np.float64), tr.scores(zr, c["qr"], zt, c["qt"], P_sqrt, np.float64))
    assert (np.diff(S[0]) > 0).all() and (np.diff(S[1]) < 0).all()
    e = np.ones((R, M), bool)
    for largest in (True, False):
        for k in (128, 64, 32, 16):
            assert_exact(run(c, largest, k=k), tr.topk(S, e, k, largest), (cap, largest, k))


# ---- 5. nothing leaks ----------------------------------------------------------------------------------------------------------------

def test_rows_beyond_M_and_pad_columns_do_not_show():
    c = tr.exact_case(150, 32, 17, 63, None, True)
    M, ld = c["M"], c["zt"].shape[1]
    big = torch.full((M + 64, ld), 1e30, device=DEV)
    big[:M] = _dev(c["zt"])
    qbig = torch.full((M + 64,), 1e30, device=DEV)
    qbig[:M] = _dev(c["qt"])
    for largest in (True, False):
        assert_exact(run(c, largest, zt=big[:M], qt=qbig[:M]), c["ref"][largest], "rows beyond M")
    # finite pad columns D2 .. ldz are allowed (include/nplda_hip.h): they meet P = 0
    big[:, c["D2"]:] = 1e30
    zr = _dev(c["zr"]).clone()
    zr[:, c["D2"]:] = -1e30
    for largest in (True, False):
        assert_exact(run(c, largest, zr=zr, zt=big[:M], qt=qbig[:M]), c["ref"][largest], "pad columns")


def test_a_fully_masked_row_is_empty():
    c = dict(tr.exact_case(150, 5, 17, 4, None, False))
    c.update(mask="same", lab_r=np.arange(17, dtype=np.int32) % 3, lab_t=np.array([0, 1, 0, 1], np.int32), k=5)
    S = tr.scores(c["zr"], c["qr"], c["zt"], c["qt"], c["P_sqrt"], np.float32)
    e = tr.eligible(17, 4, "same", c["lab_r"], c["lab_t"])
    assert not e[2].any() and e[0].sum() == 2
    for largest in (True, False):
        vals, idx = run(c, largest)
        assert_exact((vals, idx), tr.topk(S, e, 5, largest), largest)
        assert (idx[2] == -1).all() and (vals[2] == (-np.inf if largest else np.inf)).all()


# ---- 6. degenerate -------------------------------------------------------------------------------------------------------------------

def test_degenerate_shapes_and_arguments():
    from neuralplda_amd import ops
    c = tr.exact_case(170, 5, tr.TILE + 1, 5, "different", False)
    packed = packed_for(c["P_sqrt"], c["Q"])
    zr, qr, zt, qt = _dev(c["zr"]), _dev(c["qr"]), _dev(c["zt"]), _dev(c["qt"])
    vals, idx = ops.topk_scores(zr[:0], qr[:0], zt, qt, packed, 7)
    assert vals.shape == (0, 7) and idx.shape == (0, 7)
    for largest in (True, False):
        vals, idx = ops.topk_scores(zr, qr, zt[:0], qt[:0], packed, 3, largest=largest)
        assert (idx == -1).all() and (vals == (-np.inf if largest else np.inf)).all() and vals.shape == (c["R"], 3)
    vals, idx = ops.topk_scores(zr, qr, zt, qt, packed, 1, labels=(c["lab_r"].tolist(), c["lab_t"].tolist()), mask="different")
    assert_exact((vals.cpu().numpy(), idx.cpu().numpy()), tr.topk(c["S"], c["elig"], 1, True), "k = 1, labels as lists")
    with pytest.raises(ValueError):
        ops.topk_scores(zr, qr, zt, qt, packed, 129)
    with pytest.raises(ValueError):
        ops.topk_scores(zr, qr, zt, qt, packed, 0)
    with pytest.raises(ValueError):
        ops.topk_scores(zr, qr, zt, qt, packed, 3, mask="different")
    with pytest.raises(ValueError):
        ops.topk_scores(zr[:, :170], qr, zt, qt, packed, 3)


# ---- 7. repeatable and capturable ---------------------------------------------------------------------------------------------------

def test_repeatable_and_capturable():
    """Two calls give the same bits, and so does one call captured in a graph (one stream, no branches) and replayed once."""
    from neuralplda_amd import ops
    c = tr.float_case(170, 128)
    a, b = run(c, True), run(c, True)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    packed = packed_for(c["P_sqrt"], c["Q"])
    zr, qr, zt, qt = _dev(c["zr"]), _dev(c["qr"]), _dev(c["zt"]), _dev(c["qt"])
    labels = (_dev(c["lab_r"]), _dev(c["lab_t"]))
    groups = (_dev(c["grp_r"]), _dev(c["grp_t"]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.topk_scores(zr, qr, zt, qt, packed, c["k"], labels=labels, mask="different", groups=groups)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out[0].cpu().numpy(), a[0]) and same_bits(out[1].cpu().numpy(), a[1])


# ---- 8. Gallery / identify ------------------------------------------------------------------------------------------------------------

class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cuda:0", "SoftCdet", "std"


def _model(seed=0):
    from neuralplda_amd import models
    torch.manual_seed(seed)
    m = models.NeuralPlda(NC).to(DEV)
    with torch.no_grad():
        m.Q.copy_(-torch.rand(150, device=DEV))
    return m


def test_gallery_and_identify():
    from neuralplda_amd import models, search
    m = _model()
    g = torch.Generator().manual_seed(3)
    xg = torch.nn.functional.normalize(torch.randn(300, 512, generator=g), dim=1).to(DEV)
    xp = torch.nn.functional.normalize(torch.randn(40, 512, generator=g), dim=1).to(DEV)
    ids = [f"utt{i:03d}" for i in range(300)]
    glab = torch.arange(300) % 25
    gal = search.Gallery.build(m, xg, ids=ids, labels=glab)
    with torch.no_grad():
        zg, zp = m.extract_plda_embeddings(xg).cpu().numpy(), m.extract_plda_embeddings(xp).cpu().numpy()
    P_sqrt, Q = m.P_sqrt.detach().cpu().numpy(), m.Q.detach().cpu().numpy()
    qg, qp = tr.qvec(zg, Q, np.float64), tr.qvec(zp, Q, np.float64)
    c = dict(R=40, M=300, k=10, D2=150)
    c["S64"] = tr.scores(zp, qp, zg, qg, P_sqrt, np.float64)
    c["S32"] = tr.scores(zp, tr.qvec(zp, Q, np.float32), zg, tr.qvec(zg, Q, np.float32), P_sqrt, np.float32)
    c["tol"] = tr.tolerance(150, tr.magnitude(zp, qp, zg, qg, P_sqrt))
    c["elig"] = np.ones((40, 300), bool)
    for how in ("gallery", "xvectors"):
        vals, idx = m.identify(xp, gal if how == "gallery" else xg, k=10)
        vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
        tr.check_float_result(vals, idx, c, True, f"identify via {how}")
        # the embeddings' exact order, wherever the float64 scores are further apart than the tolerance
        ref_idx = tr.topk(c["S64"], c["elig"], 10, True)[1]
        clear = np.abs(np.diff(np.sort(c["S64"], 1)[:, ::-1][:, :11], axis=1)).min(1) > 2 * c["tol"].max(1)
        assert clear.sum() > 20 and np.array_equal(idx[clear], ref_idx[clear])
    assert gal.ids_of(idx[:2, :2]) == [[ids[j] for j in row[:2]] for row in idx[:2]]
    # smallest, and a label mask
    plab = torch.arange(40) % 25
    vals, idx = gal.search(xp, k=10, largest=False, exclude_labels=plab)
    c["elig"] = tr.eligible(40, 300, "different", plab.numpy(), glab.numpy())
    tr.check_float_result(vals.cpu().numpy(), idx.cpu().numpy(), c, False, "Gallery.search smallest, exclude_labels")
    # stale after the parameters change
    gal.check(m)
    with torch.no_grad():
        m.P_sqrt.mul_(1.5)
    with pytest.raises(ValueError):
        gal.check(m)
    with pytest.raises(ValueError):
        gal.search(xp)
    for cls in (models.DPlda, models.GaussianBackend):
        with pytest.raises(NotImplementedError):
            cls(NC).identify(xp, xg)


# ---- 9. mine_hard_trials ----------------------------------------------------------------------------------------------------------------

def test_mine_hard_trials_equals_the_oracle_and_trains():
    """An exact-valued 600-row table, 40 speakers, two groups, 30 utterances no speaker lists: the mined list equals the
    oracle's element for element whatever the row chunking, and one fused index-training step consumes it."""
    from neuralplda_amd import models, ops, sv_trials_loaders
    rng = np.random.default_rng(11)
    n, n_spk, D0, D = 600, 40, 512, 150
    m = _model(1)
    # exact embeddings: x = e_a (a unit vector: the LDA layer's normalisation leaves it alone), W1 = [I 0], b = 0,
    # W2 = integer / 8 entries, so z = W2[:, a] exactly; P_sqrt, Q as in the exact cases
    P_sqrt, Q = tr.exact_params(D, rng)
    W2 = (rng.integers(-16, 17, (D, D)) / 8.0).astype(np.float32)
    with torch.no_grad():
        m.centering_and_LDA.weight.copy_(torch.eye(D, D0))
        m.centering_and_LDA.bias.zero_()
        m.centering_and_wccn_plda.weight.copy_(_dev(W2))
        m.centering_and_wccn_plda.bias.zero_()
        m.P_sqrt.copy_(_dev(P_sqrt))
        m.Q.copy_(_dev(Q))
    a = rng.integers(0, D, n)                    # 600 rows over 150 distinct embeddings: every score occurs several times
    x = np.zeros((n, D0), np.float32)
    x[np.arange(n), a] = 1.0
    ids = [f"u{i:04d}" for i in range(n)]
    table = sv_trials_loaders.XvectorTable.from_matrix(ids, x)
    spk = rng.integers(0, n_spk, n)
    held_out = rng.choice(n, 30, replace=False)   # utterances of the table no speaker lists
    out = set(held_out.tolist())
    spk2utt = {f"s{s:02d}": [ids[i] for i in np.flatnonzero(spk == s) if i not in out] for s in range(n_spk)}
    groups = {f"s{s:02d}": ("a" if s % 3 else "b") for s in range(n_spk)}
    z = np.zeros((n, tr.padded_dim(D)), np.float32)
    z[:, :D] = W2[:, a].T
    with torch.no_grad():
        assert np.array_equal(m.extract_plda_embeddings(table.on(DEV)).cpu().numpy(), z[:, :D])
    q = tr.qvec(z, Q, np.float32)
    rows = np.array(sorted(set(range(n)) - out), np.int64)
    S = tr.scores(z[rows], q[rows], z[rows], q[rows], P_sqrt, np.float32)
    names = sorted(spk2utt)
    spk_id = np.array([names.index(f"s{s:02d}") for s in spk], np.int32)
    grp_id = np.array([0 if s % 3 else 1 for s in spk], np.int32)
    want = tr.mined_pairs(S, spk_id, grp_id, rows, 4, 2)
    for chunk in (None, 97):
        got = sv_trials_loaders.mine_hard_trials(m, table, spk2utt, 4, positives_per_utt=2, groups=groups, device=DEV,
                                                 chunk_rows=chunk)
        assert got[0].is_cuda and got[0].dtype == torch.int64 and got[2].dtype == torch.float32
        for g_, w_ in zip(got, want):
            assert np.array_equal(g_.cpu().numpy(), w_), chunk
    assert 0 < want[2].sum() < want[2].size and not np.isin(want[0], held_out).any()
    # one fused index-training step consumes the list
    r1, r2, t = got
    B = r1.numel()
    prm = [p.detach().clone().contiguous() for p in m._params()]
    packed = ops.pack_params(*prm)
    thetas = [torch.zeros(1, device=DEV) for _ in NC.beta]
    n = int(sum(p.numel() for p in prm)) + len(thetas)
    ea, es, step = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(2, device=DEV)
    loss = torch.zeros((), device=DEV)
    ops.train_step_rows(table.on(DEV), r1, r2, t, prm, thetas, NC.beta, NC.alpha, ops.LOSS_SOFTCDET, ea, es, step, 1e-3, 0.9, 0.999,
                        1e-8, 1e-5, packed, ops.train_step_workspace(B, packed, rows=True), loss)
    assert B > 600 and torch.isfinite(loss).item()


# ---- tools/identify.py -----------------------------------------------------------------------------------------------------------------

def test_identify_tool_writes_the_ranked_tsv(tmp_path):
    """Model pickle + gallery scp + probe archive -> TSV of probe_id, rank, gallery_id, score, equal to Gallery.search."""
    import os
    import pickle
    import sys
    from neuralplda_amd import kaldi_format, search
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import identify
    m = _model(2)
    g = torch.Generator().manual_seed(4)
    xg = torch.nn.functional.normalize(torch.randn(50, 512, generator=g), dim=1)
    xp = torch.nn.functional.normalize(torch.randn(7, 512, generator=g), dim=1)
    gids, pids = [f"g{i:02d}" for i in range(50)], [f"p{i}" for i in range(7)]
    kaldi_format.write_vector_ark(str(tmp_path / "g.ark"), gids, xg.numpy(), scp_path=str(tmp_path / "g.scp"))
    kaldi_format.write_vector_ark(str(tmp_path / "p.ark"), pids, xp.numpy())
    with open(tmp_path / "model.pt", "wb") as fh:
        pickle.dump(m, fh)
    identify.main(["--model", str(tmp_path / "model.pt"), "--gallery", str(tmp_path / "g.scp"), "--probes", str(tmp_path / "p.ark"),
                   "--k", "3", "--out", str(tmp_path / "top.tsv"), "--block", "4"])
    lines = [ln.split("\t") for ln in (tmp_path / "top.tsv").read_text().splitlines()]
    vals, idx = search.Gallery.build(m, xg.to(DEV)).search(xp.to(DEV), k=3)
    assert len(lines) == 7 * 3
    for n, (pid, rank, gid, s) in enumerate(lines):
        r, c = divmod(n, 3)
        assert pid == pids[r] and int(rank) == c + 1 and gid == gids[int(idx[r, c])]
        assert abs(float(s) - float(vals[r, c])) <= 1e-6 + 1e-6 * abs(float(vals[r, c]))
