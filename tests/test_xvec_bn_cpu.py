"""CPU-side tests of the batch-statistics extractor (design/k27_xvec_batch_stats.md): the twin (tests/xvec_bn_ref.py)
against ten stacked nn.BatchNorm1d(affine=False).train() modules and against the reference-generated fixture g15, the
host logic of XVectorNet_ETDNN_12Layer.enable_batch_stats, the C names, and the kernels' resource budget."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import xvec_bn_ref as bref, xvec_ref
from tests.test_allpairs_cpu import _resources
from tests.xvec_grad_ref import GRAD_KEYS, torch_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G15 = os.path.join(ROOT, "tests", "golden", "g15_etdnn_bn.npz")


def _stacked_batchnorm(frames, lengths, params, G):
    """utils/models.py:67-95 ten times with real nn.BatchNorm1d modules in float64, autograd gradients."""
    P = torch_params(params, torch.float64)
    bns = []
    for i, (_, dout, _, _) in enumerate(xvec_ref.LAYERS, 1):
        bn = nn.BatchNorm1d(dout, affine=False).double().train()
        with torch.no_grad():
            bn.running_mean.copy_(P[f"tdnn{i}.bn.running_mean"])
            bn.running_var.copy_(P[f"tdnn{i}.bn.running_var"])
        bns.append(bn)
    off = np.concatenate([[0], np.cumsum(lengths)])
    X = torch.as_tensor(frames, dtype=torch.float64)
    hs = [X[off[u]:off[u + 1]] for u in range(len(lengths))]
    for i, (_, _, c, d) in enumerate(xvec_ref.LAYERS, 1):
        ys = []
        for h in hs:
            Tn = h.shape[0] - d * (c - 1)
            U = torch.cat([h[j * d:j * d + Tn] for j in range(c)], dim=1)
            ys.append(torch.relu(U @ P[f"tdnn{i}.kernel.weight"].T + P[f"tdnn{i}.kernel.bias"]))
        hs = list(torch.split(bns[i - 1](torch.cat(ys)), [y.shape[0] for y in ys]))
    xv = torch.stack([torch.cat([h.mean(0), torch.std(h, 0)]) @ P["lin11.weight"].T + P["lin11.bias"] for h in hs])
    g = torch.autograd.grad((xv * torch.as_tensor(G, dtype=torch.float64)).sum(), [P[k] for k in GRAD_KEYS])
    return xv.detach().numpy(), dict(zip(GRAD_KEYS, (t.numpy() for t in g))), bns


def _close(got, ref, what, rel=1e-10):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    assert np.abs(got - ref).max() <= rel * np.abs(ref).max(), (what, np.abs(got - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("lengths", [[40, 40, 40], [57, 130, 24, 301, 33]])
def test_float64_twin_equals_stacked_batchnorm_modules(lengths):
    params = xvec_ref.make_params()
    rng = np.random.default_rng(sum(lengths))
    frames = rng.standard_normal((sum(lengths), 30)).astype(np.float32)
    G = rng.standard_normal((len(lengths), 512)).astype(np.float32)
    xv, grads, bns = _stacked_batchnorm(frames, lengths, params, G)
    twin = bref.run(frames, lengths, params, G, "std", torch.float64)
    _close(twin["xvec"], xv, "x-vectors")
    for k in GRAD_KEYS:
        _close(twin["grads"][k], grads[k], k)
    for l, bn in enumerate(bns):
        _close(twin["running_mean"][l], bn.running_mean.numpy(), f"running_mean {l}")
        _close(twin["running_var"][l], bn.running_var.numpy(), f"running_var {l}")
        assert int(bn.num_batches_tracked) == 1
        assert twin["n"][l] == sum(T - bref.CTX[l] for T in lengths)


def test_twin_with_its_own_masks_forced_is_the_same_run():
    lengths = [40, 31]
    params = xvec_ref.make_params()
    rng = np.random.default_rng(5)
    frames = rng.standard_normal((sum(lengths), 30)).astype(np.float32)
    G = rng.standard_normal((2, 512)).astype(np.float32)
    free = bref.run(frames, lengths, params, G)
    masks = []
    for l in range(10):
        m = np.zeros((sum(lengths), 1504), np.uint8)
        m[bref.valid_rows(lengths, l), :free["pre"][l].shape[1]] = free["pre"][l] > 0
        masks.append(m)
    forced = bref.run(frames, lengths, params, G, masks=masks)
    assert np.array_equal(forced["xvec"], free["xvec"])
    for k in GRAD_KEYS:
        assert np.array_equal(forced["grads"][k], free["grads"][k]), k


def test_twin_reproduces_the_reference_fixture():
    g = np.load(G15)
    params = xvec_ref.make_params()
    x = g["x"]
    B, _, T = x.shape
    frames = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(B * T, 30)
    for pool in ("std", "var"):
        twin = bref.run(frames, [T] * B, params, np.zeros((B, 512), np.float32), pool)
        ref = g[pool]
        # fp32 reference vs fp64 twin: the gate of the g13 test
        assert np.abs(twin["xvec"] - ref).max() <= 1e-5 * np.abs(ref).max(), pool
    for i in range(1, 11):
        for k in ("running_mean", "running_var"):
            ref = g[f"{k}{i}"]
            assert np.abs(twin[k][i - 1] - ref).max() <= 1e-5 * np.abs(ref).max(), (k, i)
        assert int(g[f"num_batches_tracked{i}"]) == 1


# ---- host logic ------------------------------------------------------------------------------------------------------

def _module():
    from neuralplda_amd import models
    return xvec_ref.load_into(models.XVectorNet_ETDNN_12Layer(), xvec_ref.make_params())


def test_switch_defaults_off_and_old_pickles_load():
    m = _module()
    assert m.batch_stats_enabled is False and "batch_stats_enabled" not in m.__dict__
    assert m.enable_batch_stats() is m and m.batch_stats_enabled is True
    assert m.enable_batch_stats(False).batch_stats_enabled is False
    del m.__dict__["batch_stats_enabled"]  # a pickle written before the switch existed has no such attribute
    back = pickle.loads(pickle.dumps(m))
    assert back.batch_stats_enabled is False and back.backward_enabled is False
    assert "batch_stats_enabled" not in m.state_dict() and len(m.state_dict()) == 62


def test_switch_off_keeps_the_training_mode_error():
    m = _module().train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="running-statistics batch norm only"):
        m.extract(torch.zeros(2, 30, 40))


def test_mixed_modes_momentum_none_and_too_few_frames_raise():
    m = _module().train().enable_batch_stats()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.zeros(2, 30, 40)
    m.tdnn4.bn.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="mixed batch-norm modes"):
        m.extract(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="mixed batch-norm modes"):
        m.extract_ragged(torch.zeros(80, 30), [40, 40])
    m.tdnn4.bn.train()
    m.tdnn7.bn.momentum = None
    with torch.no_grad(), pytest.raises(RuntimeError, match="momentum is None"):
        m.extract(x)
    m.tdnn7.bn.momentum = 0.1
    with torch.no_grad(), pytest.raises(ValueError, match="more than 1 value per channel"):
        m.extract_ragged(torch.zeros(23, 30), [23])
    with torch.no_grad(), pytest.raises(ValueError, match="more than 1 value per channel"):
        m.extract(torch.zeros(1, 30, 23))
    # a trainable extractor under grad mode without enable_backward() stays an error, as on the running-statistics path
    with pytest.raises(RuntimeError, match="no backward through the x-vector extractor"):
        m.extract(x)
    # windows: training-mode batch norm is still refused
    with torch.no_grad(), pytest.raises(RuntimeError, match="running-statistics batch norm only"):
        m.extract_windows(torch.zeros(80, 30), [[0, 40]])
    # none of the refused calls touched a buffer
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert all(int(t.bn.num_batches_tracked) == 0 for t in m.tdnns())


def test_c_names_and_abi_version(hip_lib):
    import ctypes
    from neuralplda_amd import _lib
    assert hip_lib.nplda_abi_version() == 4
    for name in ("nplda_xvec_train_bn_saved_bytes", "nplda_xvec_bn_stats_bytes", "nplda_xvec_bn_mask_layout",
                 "nplda_xvec_extract_train_bn_f32", "nplda_xvec_backward_bn_workspace_bytes",
                 "nplda_xvec_backward_bn_f32"):
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name), name
    R, U = 545, 5
    base = hip_lib.nplda_xvec_train_saved_bytes(R, U)
    assert hip_lib.nplda_xvec_train_bn_saved_bytes(R, U) > base
    assert hip_lib.nplda_xvec_backward_bn_workspace_bytes(R, U) > hip_lib.nplda_xvec_backward_workspace_bytes(R, U)
    assert hip_lib.nplda_xvec_bn_stats_bytes() == 2 * (9 * 512 + 1504) * 4 + 10 * 8
    off, ld = ctypes.c_size_t(), ctypes.c_int64()
    ends = []
    for l in range(10):
        assert hip_lib.nplda_xvec_bn_mask_layout(R, U, l, ctypes.byref(off), ctypes.byref(ld)) == 0
        assert ld.value == (1504 if l == 9 else 512) and off.value % 256 == 0
        ends.append((off.value, off.value + (640 + 16) * ld.value))
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= base
    assert hip_lib.nplda_xvec_bn_mask_layout(R, U, 10, ctypes.byref(off), ctypes.byref(ld)) == -22
    # too few valid rows: a status, before any pointer is looked at (nothing is launched)
    one = ctypes.c_void_p(16)
    eps = (ctypes.c_float * 10)(*[1e-5] * 10)
    assert hip_lib.nplda_xvec_extract_train_bn_f32(one, 0, 30, one, 1, 23, 0, one, eps, one, 512, one, 1 << 30, one,
                                                   1 << 20, None) == -22
    assert hip_lib.nplda_xvec_backward_bn_f32(one, 1 << 30, one, 1, 23, 0, one, 512, one, one, one, one, 1 << 30,
                                              None) == -22


# ---- kernel resources ------------------------------------------------------------------------------------------------

def test_register_budget_of_the_batch_stats_kernels():
    """The two new GEMM instantiations (raw training forward, raw data gradient) keep the extraction kernel's budget: no
    scratch, two blocks of four waves per CU (at most 256 registers, 64 KB LDS each); no kernel of the file uses scratch."""
    res = _resources("nplda_xvec_bn.hip")
    main = {k: v for k, v in res.items() if "xvbn_gemm_kernel" in k}
    assert len(main) == 2, sorted(res)
    for k, v in main.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
        assert v["LDS"] <= 64 * 1024, (k, v)
    rest = {k: v for k, v in res.items() if k not in main}
    # sums x 2, two finishes, normalise, apply, pooling backward, and the header's input and pooling kernels
    assert len(rest) == 9, sorted(res)
    for k, v in rest.items():
        assert v["ScratchSize"] == 0, (k, v)
