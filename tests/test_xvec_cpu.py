"""CPU tests of the E-TDNN x-vector extractor's host side: the fp64 restatement against the reference-generated fixture
(g13), state-dict layout, Kaldi pickle loading, pickling through the compat aliases, E2EConf, argument checks, the
workspace restatement and the GEMM kernel's resource budget."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from tests import xvec_ref
from tests.test_allpairs_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = os.path.join(ROOT, "tests", "golden", "g13_etdnn.npz")


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cpu", "SoftCdet", "std"


def test_restatement_reproduces_the_reference_fixture():
    g = np.load(G13)
    p = xvec_ref.make_params()
    for n in range(3):
        x = g[f"x{n}"]
        for pool in ("std", "var"):
            ref, got = g[f"{pool}{n}"], xvec_ref.extract(x, p, pool)
            assert np.array_equal(np.isnan(ref), np.isnan(got)), (n, pool)
            if np.isfinite(ref).any():
                # fp32 reference vs fp64 restatement: fp32 rounding through ten layers (measured 1.6e-6 of max|ref|)
                assert np.nanmax(np.abs(got - ref)) <= 1e-5 * np.nanmax(np.abs(ref)), (n, pool)
    assert np.isnan(g["std1"]).all() and np.isnan(g["var1"]).all()  # T = 23: one pooled frame


def test_state_dict_layout_matches_reference():
    from neuralplda_amd import models
    g = np.load(G13)
    m = models.XVectorNet_ETDNN_12Layer()
    sd = m.state_dict()
    assert len(sd) == 62
    assert list(sd.keys()) == [str(k) for k in g["xvec_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["xvec_shapes"]]
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    esd = e.state_dict()
    assert list(esd.keys()) == [str(k) for k in g["etdnn_keys"]]
    assert [",".join(map(str, v.shape)) for v in esd.values()] == [str(s) for s in g["etdnn_shapes"]]
    assert e.pooling_function is torch.std and e.xvector_extractor.pooling_function is torch.std
    nc = NC()
    nc.pooling_function = "var"
    assert models.Etdnn_Xvec_NeuralPlda(nc).xvector_extractor.pooling_function is torch.var


def test_train1_puts_tdnn_batch_norms_in_eval_mode():
    from neuralplda_amd import models
    e = models.Etdnn_Xvec_NeuralPlda(NC()).train1()
    assert e.training and e.xvector_extractor.training
    assert all(not t.bn.training for t in e.xvector_extractor.tdnns())
    assert e.xvector_extractor.bn11.training


def _kaldi_pickle(path, rng):
    kw = {}
    for i, (din, dout, c, _) in enumerate(xvec_ref.LAYERS, 1):
        kw[f"tdnn{i}.affine"] = {"params": rng.standard_normal((dout, din * c)), "bias": rng.standard_normal(dout)}
        kw[f"tdnn{i}.batchnorm"] = {"stats-mean": rng.standard_normal(dout), "stats-var": rng.random(dout) + 0.5}
    kw["tdnn11.affine"] = {"params": rng.standard_normal((512, 3000)), "bias": rng.standard_normal(512)}
    kw["tdnn11.batchnorm"] = {"stats-mean": rng.standard_normal(512), "stats-var": rng.random(512)}
    kw["tdnn12.affine"] = {"params": rng.standard_normal((512, 512)), "bias": rng.standard_normal(512)}
    kw["tdnn12.batchnorm"] = {"stats-mean": rng.standard_normal(512), "stats-var": rng.random(512)}
    kw["output.affine"] = {"params": rng.standard_normal((40, 512)), "bias": rng.standard_normal(40)}
    with open(path, "wb") as f:
        pickle.dump(kw, f)
    return kw


def test_load_from_kaldi_pickle(tmp_path):
    from neuralplda_amd import models
    kw = _kaldi_pickle(tmp_path / "xvec.pkl", np.random.default_rng(3))
    m = models.XVectorNet_ETDNN_12Layer(noclasses=40)
    m._xvec_cache["key"] = "stale"
    m.LoadFromKaldi(str(tmp_path / "xvec.pkl"))
    sd = m.state_dict()
    f32 = lambda a: torch.from_numpy(a).float()  # noqa: E731
    for i in range(1, 11):
        assert torch.equal(sd[f"tdnn{i}.kernel.weight"], f32(kw[f"tdnn{i}.affine"]["params"]))
        assert torch.equal(sd[f"tdnn{i}.bn.running_var"], f32(kw[f"tdnn{i}.batchnorm"]["stats-var"]))
    assert torch.equal(sd["lin11.bias"], f32(kw["tdnn11.affine"]["bias"]))
    assert torch.equal(sd["bn12.running_mean"], f32(kw["tdnn12.batchnorm"]["stats-mean"]))
    assert torch.equal(sd["finlin.weight"], f32(kw["output.affine"]["params"]))
    assert m._xvec_cache == {}


def test_pickle_roundtrip_through_compat_aliases():
    from neuralplda_amd import compat, models, xvector
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    with torch.no_grad():
        e.xvector_extractor.tdnn3.kernel.weight.fill_(0.25)
    e.xvector_extractor._xvec_cache["buf"] = torch.zeros(3)
    compat.install()
    try:
        import sys
        assert sys.modules["utils.models"].Etdnn_Xvec_NeuralPlda is xvector.Etdnn_Xvec_NeuralPlda
        assert sys.modules["utils.models"].TDNN is xvector.TDNN
        assert sys.modules["utils.NpldaConf"].E2EConf is not None
        classes = (xvector.TDNN, xvector.XVectorNet_ETDNN_12Layer, xvector.Etdnn_Xvec_NeuralPlda)
        old = [c.__module__ for c in classes]
        for c in classes:
            c.__module__ = "utils.models"
        try:
            blob = pickle.dumps(e)
        finally:
            for c, o in zip(classes, old):
                c.__module__ = o
        assert b"utils.models" in blob and b"Etdnn_Xvec_NeuralPlda" in blob
        e2 = pickle.loads(blob)
    finally:
        compat.uninstall()
    assert type(e2) is xvector.Etdnn_Xvec_NeuralPlda and type(e2.xvector_extractor.tdnn1) is xvector.TDNN
    assert e2.xvector_extractor._xvec_cache == {} and e2.pooling_function is torch.std
    assert all(torch.equal(a, b) for a, b in zip(e.state_dict().values(), e2.state_dict().values()))


E2E_CFG = """[Paths]
base_path = /data
train_spk2utt_list = ${base_path}/a/spk2utt,${base_path}/b/spk2utt
training_data_trials_list = t1,t2
validation_trials_list = v1
test_trials_list = e1
mega_mfcc_scp = ${base_path}/mfcc.scp
mega_mfcc_pkl = mfcc.pkl
xvec_model = final.pkl
meanvec = mean.vec
transformmat = transform.mat
kaldiplda = plda
[NPLDA]
xvector_dim = 512
layer1_LDA_dim = 150
layer2_PLDA_spkfactor_dim = 150
initialization = kaldi
pooling_function = var
device = cuda
seed = 1
alpha = 15
[Training]
loss = SoftCdet
cmiss = 1
cfa = 1
target_probs = 0.01,0.005
batch_size = 64
min_num_spks_per_batch = 4
max_num_spks_per_batch = 16
n_epochs = 2
lr = 0.0001
heldout_set_for_lr_decay = v1
heldout_set_for_th_init = v1
train_subsample_factors = None
valid_subsample_factors = 0.5,1
[Logging]
log_interval = 10
[Scoring]
scorefile_format = sre
"""


def test_e2econf_parses_and_builds_the_model(tmp_path):
    from neuralplda_amd import models
    from neuralplda_amd.NpldaConf import E2EConf
    from neuralplda_amd.scorefile_generator import generate_sre_scores
    f = tmp_path / "e2e.cfg"
    f.write_text(E2E_CFG)
    c = E2EConf(str(f))
    assert c.train_spk2utt_list == ["/data/a/spk2utt", "/data/b/spk2utt"] and c.mega_mfcc_scp == "/data/mfcc.scp"
    assert c.pooling_function == "var" and c.min_num_spks_per_batch == 4 and c.max_num_spks_per_batch == 16
    assert c.beta == pytest.approx([99.0, 199.0]) and c.train_subsample_factors is None
    assert c.valid_subsample_factors == [0.5, 1.0] and c.generate_scorefile is generate_sre_scores
    c.device = "cpu"
    assert models.Etdnn_Xvec_NeuralPlda(c).xvector_extractor.pooling_function is torch.var
    with pytest.raises(IOError):
        E2EConf(str(tmp_path / "missing.cfg"))


def test_short_utterances_and_bad_shapes_raise():
    from neuralplda_amd import models
    m = models.XVectorNet_ETDNN_12Layer().eval().requires_grad_(False)
    with pytest.raises(ValueError):
        m.extract(torch.zeros(2, 30, 22))
    with pytest.raises(ValueError):
        m.extract(torch.zeros(2, 23, 40))
    with pytest.raises(ValueError):
        m.extract_ragged(torch.zeros(60, 30), [40, 20])
    with pytest.raises(ValueError):
        m.extract_ragged(torch.zeros(60, 30), [41, 19])
    t = models.XVectorNet_ETDNN_12Layer()  # fresh module: training mode
    with pytest.raises(RuntimeError, match="eval"):
        t.extract(torch.zeros(1, 30, 40))


def test_workspace_restatement_and_chunking(hip_lib):
    from neuralplda_amd import xvector
    for R, U in [(0, 0), (23, 1), (24, 1), (1000, 3), (300_000, 1000), (3_000_000, 10_000)]:
        assert hip_lib.nplda_xvec_workspace_bytes(R, U) == xvector._ws_bytes(R, U)
    lens = list(np.random.default_rng(0).integers(23, 400, 500))
    for limit in (1, 4 << 20, 1 << 30):
        ch = xvector._chunks(lens, limit)
        assert ch[0][0] == 0 and ch[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(u1 - u0 == 1 or xvector._ws_bytes(sum(lens[u0:u1]), u1 - u0) <= limit for u0, u1 in ch)
    assert len(xvector._chunks(lens, 1)) == len(lens)
    assert xvector.flops_per_frame()[0] == 2 * (150 * 512 + 5 * 512 * 512 + 3 * 1536 * 512 + 512 * 1500)


def test_xvec_abi_argument_checks(hip_lib):
    assert hip_lib.nplda_xvec_packed_bytes() > 11 * 1024 * 1024
    # n_utts == 0 is a no-op; bad layout / pooling are refused before anything runs
    assert hip_lib.nplda_xvec_extract_f32(None, 0, 30, None, 0, 0, 0, None, None, 512, None, 0, None) == 0
    assert hip_lib.nplda_xvec_extract_f32(None, 2, 30, None, 0, 0, 0, None, None, 512, None, 0, None) == -22
    assert hip_lib.nplda_xvec_extract_f32(None, 0, 30, None, 0, 0, 2, None, None, 512, None, 0, None) == -22
    assert hip_lib.nplda_xvec_extract_f32(None, 0, 30, None, 1, 40, 0, None, None, 512, None, 0, None) == -22


# ---- status table of the six extractor entry points --------------------------------------------------------------------
# Every row returns before anything is enqueued, so the pointers are fake addresses that nothing dereferences: _A is
# 16-byte aligned, _M is not.  A size argument is given as a difference from what the library asks for at the row's
# (total_frames, n); the base vector passes every check but the last: each buffer is one byte short (-28).  A row changes
# the base in one place, so a check that moved behind the size test would show as -28.
# Rows per entry point (the test asserts these counts, so a row cannot drop out unseen), by expected status:
#   extract, extract_train, backward   29 rows: 20 x -22, 7 x -28, 1 x -95, 1 x 0
#   extract_windows                    27 rows: 18 x -22, 7 x -28, 1 x -95, 1 x 0   (no layout argument)
#   extract_train_bn                   38 rows: 26 x -22, 9 x -28, 2 x -95, 1 x 0   (eps, stats; rows; frame limit)
#   backward_bn                        33 rows: 22 x -22, 8 x -28, 2 x -95, 1 x 0
_ROWS = {"extract": 29, "extract_train": 29, "backward": 29, "extract_windows": 27, "extract_train_bn": 38,
         "backward_bn": 33}
_A, _M = 4096, 4096 + 8
_EPS = (ctypes.c_float * 10)(*[1e-5] * 10)
_FWD = ("x", "layout", "ld_in", "offsets", "n", "total_frames", "pooling", "packed", "out", "ldx")
_BWD = ("saved", "saved_bytes", "offsets", "n", "total_frames", "pooling", "dxvec", "lddx", "packed", "packed_t", "grad",
        "ws", "ws_bytes", "stream")
_ENTRIES = {
    "extract": dict(
        fn="nplda_xvec_extract_f32", args=_FWD + ("ws", "ws_bytes", "stream"),
        sizes={"ws_bytes": "nplda_xvec_workspace_bytes"}, ptrs=("x", "offsets", "packed", "out", "ws"),
        aligned=("packed", "out", "ws"), limit=0x7fffffff // 6),
    "extract_windows": dict(
        fn="nplda_xvec_extract_windows_f32",
        args=("x", "ld_in", "total_frames", "win_begin", "win_end", "n", "pooling", "packed", "out", "ldx", "ws", "ws_bytes",
              "stream"),
        sizes={"ws_bytes": "nplda_xvec_windows_workspace_bytes"},
        ptrs=("x", "win_begin", "win_end", "packed", "out", "ws"), aligned=("packed", "out", "ws"), limit=0x7fffffff // 3),
    "extract_train": dict(
        fn="nplda_xvec_extract_train_f32", args=_FWD + ("saved", "saved_bytes", "stream"),
        sizes={"saved_bytes": "nplda_xvec_train_saved_bytes"}, ptrs=("x", "offsets", "packed", "out", "saved"),
        aligned=("packed", "out", "saved"), limit=0x7fffffff // 6),
    "extract_train_bn": dict(
        fn="nplda_xvec_extract_train_bn_f32",
        args=_FWD[:8] + ("eps",) + _FWD[8:] + ("saved", "saved_bytes", "stats", "stats_bytes", "stream"),
        sizes={"saved_bytes": "nplda_xvec_train_bn_saved_bytes", "stats_bytes": "nplda_xvec_bn_stats_bytes"},
        ptrs=("x", "offsets", "packed", "eps", "out", "saved", "stats"), aligned=("packed", "out", "saved", "stats"),
        limit=0x7fffffff // 6, batch_stats=True),
    "backward": dict(
        fn="nplda_xvec_backward_f32", args=_BWD,
        sizes={"saved_bytes": "nplda_xvec_train_saved_bytes", "ws_bytes": "nplda_xvec_backward_workspace_bytes"},
        ptrs=("saved", "offsets", "dxvec", "packed", "packed_t", "grad", "ws"),
        aligned=("saved", "packed", "packed_t", "grad", "ws"), limit=0x7fffffff // 6),
    "backward_bn": dict(
        fn="nplda_xvec_backward_bn_f32", args=_BWD,
        sizes={"saved_bytes": "nplda_xvec_train_bn_saved_bytes", "ws_bytes": "nplda_xvec_backward_bn_workspace_bytes"},
        ptrs=("saved", "offsets", "dxvec", "packed", "packed_t", "grad", "ws"),
        aligned=("saved", "packed", "packed_t", "grad", "ws"), limit=0x7fffffff // 6, batch_stats=True),
}


def _status_rows(e):
    """(what, changes to the base vector, expected status), from reading the checks of the entry point in order."""
    fwd, layout, bn = "ldx" in e["args"], "layout" in e["args"], e.get("batch_stats", False)
    big = e["limit"] + 1
    rows = [("base: every buffer one byte short", {}, -28),
            ("negative n", {"n": -1}, -22),
            ("negative total_frames", {"total_frames": -1}, -22),
            ("bad pooling", {"pooling": 2}, -22),
            ("bad pooling comes before the n == 0 return", {"pooling": 2, "n": 0, "total_frames": 0}, -22),
            ("n == 0: nothing to do, no pointer is looked at",
             dict({p: None for p in e["ptrs"]}, n=0, total_frames=0), 0),
            ("n above the grid limit", {"n": big, "total_frames": 25 * big}, -95),
            ("null pointer and n above the grid limit: the pointer check wins",
             {e["ptrs"][0]: None, "n": big, "total_frames": 25 * big}, -22)]
    if layout:
        rows += [("bad layout", {"layout": 2}, -22),
                 ("bad layout comes before the n == 0 return", {"layout": 2, "n": 0, "total_frames": 0}, -22),
                 ("ld_in of 29", {"ld_in": 29}, -22),
                 ("BCT ignores ld_in", {"layout": 1, "total_frames": 735, "ld_in": 29}, -28),
                 ("BCT, total_frames % n != 0", {"layout": 1, "total_frames": 734}, -22)]
    elif fwd:
        rows += [("ld_in of 29", {"ld_in": 29}, -22)]
    rows += [(f"null {p}", {p: None}, -22) for p in e["ptrs"]]
    rows += [(f"misaligned {p}", {p: _M}, -22) for p in e["aligned"]]
    rows += [(f"{p} needs no alignment", {p: _M}, -28) for p in e["ptrs"] if p not in e["aligned"] and p != "eps"]
    if fwd:
        rows += [("ldx of 511", {"ldx": 511}, -22), ("ldx of 514", {"ldx": 514}, -22), ("ldx of 516", {"ldx": 516}, -28)]
    else:
        rows += [("lddx of 511", {"lddx": 511}, -22), ("lddx of 514", {"lddx": 514}, -28)]
    if bn:
        rows += [("too few rows: R - 22 n == 1", {"total_frames": 111}, -22),
                 ("just enough rows", {"total_frames": 112}, -28),
                 ("too few rows and n above the grid limit: the row count wins", {"n": big, "total_frames": 22 * big}, -22),
                 ("total_frames above the grid limit of the row kernels", {"total_frames": 0x7fffffff * 16 - 127}, -95),
                 ("total_frames at that limit", {"total_frames": 0x7fffffff * 16 - 128}, -28)]
    else:
        rows += [("no lower bound on the rows", {"total_frames": 111}, -28)]
    for s in e["sizes"]:
        rows.append((f"only {s} one byte short", {k: (-1 if k == s else 0) for k in e["sizes"]}, -28))
        rows.append((f"null pointer and {s} short: the pointer check wins",
                     dict({k: (-1 if k == s else 0) for k in e["sizes"]}, **{e["ptrs"][-1]: None}), -22))
    return rows


@pytest.mark.parametrize("entry", sorted(_ENTRIES))
def test_xvec_entry_point_status_table(hip_lib, entry):
    """Every argument check of the six extractor entry points, in the order the entry point makes them: one row per check
    with everything before it passing, and rows where two fail and the earlier one must win."""
    e = _ENTRIES[entry]
    fn = getattr(hip_lib, e["fn"])
    rows = _status_rows(e)
    assert len(rows) == _ROWS[entry], (entry, len(rows))
    for what, change, want in rows:
        v = dict({p: _A for p in e["ptrs"]}, eps=_EPS, layout=0, ld_in=30, n=5, total_frames=733, pooling=0, ldx=512,
                 lddx=512, stream=None)
        v.update({k: -1 for k in e["sizes"]})
        v.update(change)
        R, n = max(v["total_frames"], 0), max(v["n"], 0)
        for k, size_fn in e["sizes"].items():
            f = getattr(hip_lib, size_fn)
            v[k] = max((f(R, n) if f.argtypes else f()) + v[k], 0)
        assert fn(*[v[a] for a in e["args"]]) == want, (entry, what)


def test_xvec_gemm_kernel_resources():
    """The TDNN GEMM keeps two blocks per CU (64 KB of LDS each, <= 256 registers) with nothing in scratch."""
    res = _resources("nplda_xvec.hip")
    gemm = [v for k, v in res.items() if "xvec_gemm_kernel" in k]
    assert len(gemm) == 1, sorted(res)
    g = gemm[0]
    assert g["ScratchSize"] == 0 and g["Occupancy"] >= 2 and g["VGPRs"] + g["AGPRs"] <= 256 and g["LDS"] == 65536, g
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
