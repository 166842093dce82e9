"""CPU tests of the extractor backward's host side: the new C entry points' argument checks and sizes, the resource
budget of csrc/nplda_xvec_bwd.hip's kernels, the opt-in switch (XVectorNet_ETDNN_12Layer.enable_backward,
Etdnn_Xvec_NeuralPlda.train1(finetune_extractor=...)) and the fp64 torch restatement (tests/xvec_grad_ref.py) against the
reference-generated fixture g14."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import xvec_grad_ref as gref, xvec_ref
from tests.test_allpairs_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = os.path.join(ROOT, "tests", "golden", "g13_etdnn.npz")
G14 = os.path.join(ROOT, "tests", "golden", "g14_etdnn_grads.npz")


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cpu", "SoftCdet", "std"


def test_switch_semantics():
    from neuralplda_amd import models
    e = models.Etdnn_Xvec_NeuralPlda(NC())
    ext = e.xvector_extractor
    assert ext.backward_enabled is False and "backward_enabled" not in ext.__dict__
    keys = list(e.state_dict().keys())
    assert e.train1() is e and ext.backward_enabled is False
    assert e.train1(finetune_extractor=True) is e and ext.backward_enabled is True
    assert all(not t.bn.training for t in ext.tdnns())
    assert e.train1() is e and ext.backward_enabled is True  # None leaves it alone
    assert list(e.state_dict().keys()) == keys
    g = np.load(G13)
    assert list(e.state_dict().keys()) == [str(k) for k in g["etdnn_keys"]]
    back = pickle.loads(pickle.dumps(e))
    assert back.xvector_extractor.backward_enabled is True
    e.train1(finetune_extractor=False)
    assert ext.backward_enabled is False
    assert ext.enable_backward() is ext and ext.backward_enabled is True
    # a model pickled before the switch existed: no attribute in its state -> off
    old = models.XVectorNet_ETDNN_12Layer()
    state = old.__getstate__()
    state.pop("backward_enabled", None)
    fresh = models.XVectorNet_ETDNN_12Layer.__new__(models.XVectorNet_ETDNN_12Layer)
    fresh.__setstate__(state)
    assert fresh.backward_enabled is False


def test_switch_off_errors_unchanged():
    from neuralplda_amd import models
    m = models.XVectorNet_ETDNN_12Layer().eval()
    with pytest.raises(RuntimeError, match="backward"):
        m.extract(torch.zeros(1, 30, 40))
    m.enable_backward()
    with pytest.raises(RuntimeError, match="its input must not require grad"):
        m.extract(torch.zeros(1, 30, 40, requires_grad=True))
    m.tdnn2.bn.train()
    with pytest.raises(RuntimeError, match="train1"):
        m.extract(torch.zeros(1, 30, 40))


def test_backward_abi_argument_checks(hip_lib):
    lib = hip_lib
    # flat gradient: W (Dout, c Din) + b (Dout) of tdnn1..tdnn10 and lin11
    want = sum(dout * (din * c + 1) for din, dout, c, _ in xvec_ref.LAYERS) + 512 * 3001
    assert lib.nplda_xvec_grad_floats() == want
    assert lib.nplda_xvec_packed_t_bytes() > 10 * 1024 * 1024
    assert lib.nplda_xvec_train_saved_bytes(-1, 1) == 0 and lib.nplda_xvec_backward_workspace_bytes(1, -1) == 0
    per_frame = (lib.nplda_xvec_train_saved_bytes(1_280_000, 1) - lib.nplda_xvec_train_saved_bytes(128_000, 1)) / 1_152_000
    assert 29_000 < per_frame < 32_000  # ~30 KB per frame, as documented
    assert lib.nplda_xvec_train_saved_bytes(1000, 3) < lib.nplda_xvec_train_saved_bytes(1000, 300)
    assert lib.nplda_xvec_backward_workspace_bytes(300_000, 1000) > 300_000 * 10_000
    # n_utts == 0 is a no-op; bad layout / pooling / null pointers are EINVAL; small buffers ENOSPC
    assert lib.nplda_xvec_extract_train_f32(None, 0, 30, None, 0, 0, 0, None, None, 512, None, 0, None) == 0
    assert lib.nplda_xvec_extract_train_f32(None, 2, 30, None, 0, 0, 0, None, None, 512, None, 0, None) == -22
    assert lib.nplda_xvec_extract_train_f32(None, 0, 30, None, 0, 0, 2, None, None, 512, None, 0, None) == -22
    assert lib.nplda_xvec_extract_train_f32(None, 0, 30, None, 1, 40, 0, None, None, 512, None, 0, None) == -22
    assert lib.nplda_xvec_backward_f32(None, 0, None, 0, 0, 0, None, 512, None, None, None, None, 0, None) == 0
    assert lib.nplda_xvec_backward_f32(None, 0, None, 0, 0, 2, None, 512, None, None, None, None, 0, None) == -22
    assert lib.nplda_xvec_backward_f32(None, 0, None, 1, 40, 0, None, 512, None, None, None, None, 0, None) == -22
    assert lib.nplda_xvec_pack_t_f32(None, None, 0, None) == -22
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    p16 = p + (-p) % 16
    assert lib.nplda_xvec_extract_train_f32(p16, 0, 30, p16, 1, 40, 0, p16, p16, 512, p16, 16, None) == -28
    assert lib.nplda_xvec_backward_f32(p16, 16, p16, 1, 40, 0, p16, 512, p16, p16, p16, p16, 16, None) == -28
    assert lib.nplda_xvec_backward_f32(p16, 1 << 40, p16, 1, 40, 0, p16, 511, p16, p16, p16, p16, 1 << 40, None) == -22


def test_backward_kernel_resources():
    """Every kernel of nplda_xvec_bwd.hip runs without scratch; the GEMMs keep at least two blocks per CU."""
    res = _resources("nplda_xvec_bwd.hip")
    gemms = {k: v for k, v in res.items() if "xvtr_gemm_kernel" in k or "xvbwd_wgrad_kernel" in k}
    assert len(gemms) == 4, sorted(res)  # EpiTrain, EpiBwd, EpiExtract, wgrad
    for k, v in gemms.items():
        assert v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256 and v["LDS"] <= 65536, (k, v)
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)


def test_restatement_reproduces_the_reference_fixture():
    g = np.load(G14)
    params, head = xvec_ref.make_params(), xvec_ref.make_head()
    lr = float(g["lr"])
    for n in range(int(g["ncases"])):
        P = gref.torch_params(params)
        H = {k: torch.tensor(head[k], dtype=torch.float64, requires_grad=True) for k in gref.HEAD_KEYS}
        th = [torch.full((1,), float(g[f"th{n}"]), dtype=torch.float64, requires_grad=True) for _ in range(2)]
        x1, x2, t = (torch.from_numpy(g[f"{k}{n}"]).double() for k in ("xa", "xb", "t"))
        loss = gref.e2e_loss(x1, x2, t, P, H, th, str(g[f"pool{n}"]), float(g["alpha"]))
        loss.backward()
        assert abs(loss.item() - float(g[f"loss{n}"])) <= 1e-5 * abs(float(g[f"loss{n}"])), n
        for k in gref.HEAD_KEYS:
            ref = g[f"hgrad{n}/{k}"]
            got = H[k].grad.numpy().ravel()[g[f"hidx{n}/{k}"]]
            assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (n, k)
        leaves = [P[k] for k in gref.GRAD_KEYS] + [H[k] for k in gref.HEAD_KEYS] + th
        for k in gref.GRAD_KEYS:
            gg = P[k].grad.numpy().ravel()
            ref = g[f"grad{n}/{k}"]
            assert abs(np.linalg.norm(gg) - float(g[f"norm{n}/{k}"])) <= 1e-4 * float(g[f"norm{n}/{k}"]), (n, k)
            assert np.abs(gg[g[f"idx{n}/{k}"]] - ref).max() <= 1e-4 * np.abs(ref).max(), (n, k)
        torch.optim.Adam(leaves, lr=lr).step()
        for k in gref.GRAD_KEYS:
            ref = g[f"step{n}/{k}"]
            got = P[k].detach().numpy().ravel()[g[f"idx{n}/{k}"]]
            assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (n, k)
