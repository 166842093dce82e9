#!/usr/bin/env python3
"""Generate tests/golden/g14_etdnn_grads.npz by RUNNING THE REFERENCE's Etdnn_Xvec_NeuralPlda (utils/models.py:216-300)
with autograd, in the mode the reference trains it in: `train1()` (tdnn batch norms on their running statistics), SoftCdet
loss, every parameter trainable, one torch.optim.Adam step.

Runs only where the reference is available (like make_golden_xvec.py).  Weights are not stored: the generator and the
tests build them from a seed through tests/xvec_ref.py.  Stored per case: the features of both sides, the targets, the
pooling, the thresholds (set to the median score), the loss, the head's gradients (sampled), and per extractor tensor (tdnn1..tdnn10 weight / bias, lin11 weight / bias) the
gradient's norm, 256 seeded flat indices, the gradient there and the parameter there after one Adam step.

    python tests/golden/make_golden_xvec_grads.py

Reference symbols executed: Etdnn_Xvec_NeuralPlda.{__init__, train1, forward, extract_plda_embeddings,
forward_from_plda_embeddings, loss, softcdet}, XVectorNet_ETDNN_12Layer.{extract, statspooling}, TDNN.forward.
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.modules.setdefault("kaldi_io", types.ModuleType("kaldi_io"))

from utils import models as refm  # noqa: E402

from tests import xvec_grad_ref, xvec_ref  # noqa: E402

# (pairs, T of side 1, T of side 2, pooling): the last case has sides of different lengths
CASES = ((3, 40, 40, "std"), (2, 30, 30, "var"), (4, 35, 61, "std"))
LR = 1e-3
NSAMPLE = 256
ALPHA = 1.0  # with alpha = 15 and zero thresholds the sigmoids saturate and the gradients are fp32 round-off


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], ALPHA, "cpu", "SoftCdet", "std"


def main():
    torch.manual_seed(0)
    params, head = xvec_ref.make_params(), xvec_ref.make_head()
    rng = np.random.default_rng(1415)
    out = {"ncases": np.array(len(CASES)), "lr": np.array(LR), "alpha": np.array(ALPHA)}
    for n, (B, T1, T2, pool) in enumerate(CASES):
        nc = NC()
        nc.pooling_function = pool
        e = refm.Etdnn_Xvec_NeuralPlda(nc)
        xvec_ref.load_into(e.xvector_extractor, params)
        xvec_ref.load_into(e, head)
        e.train1()
        xa = rng.standard_normal((B, 30, T1)).astype(np.float32)
        xb = rng.standard_normal((B, 30, T2)).astype(np.float32)
        t = np.zeros(B, np.float32)
        t[::2] = 1.0
        with torch.no_grad():  # thresholds at the median score: the loss is not saturated
            th = float(e(torch.from_numpy(xa), torch.from_numpy(xb)).median())
            for b in nc.beta:
                e.threshold[b].fill_(th)
        out[f"th{n}"] = np.array(th, np.float32)
        opt = torch.optim.Adam(e.parameters(), lr=LR)
        opt.zero_grad()
        loss = e.loss(e(torch.from_numpy(xa), torch.from_numpy(xb)), torch.from_numpy(t))
        loss.backward()
        out.update({f"pool{n}": np.array(pool), f"xa{n}": xa, f"xb{n}": xb, f"t{n}": t, f"loss{n}": np.array(loss.item())})
        sd = dict(e.named_parameters())
        for k in xvec_grad_ref.HEAD_KEYS:  # the two head matrices sampled like the extractor's tensors
            g = sd[k].grad.numpy().ravel()
            hidx = np.sort(rng.choice(g.size, min(NSAMPLE, g.size), replace=False)).astype(np.int64)
            out[f"hidx{n}/{k}"] = hidx
            out[f"hgrad{n}/{k}"] = g[hidx].copy()
        idx = {}
        for k in xvec_grad_ref.GRAD_KEYS:
            g = sd["xvector_extractor." + k].grad.numpy().ravel()
            idx[k] = np.sort(rng.choice(g.size, min(NSAMPLE, g.size), replace=False)).astype(np.int64)
            out[f"idx{n}/{k}"] = idx[k]
            out[f"grad{n}/{k}"] = g[idx[k]].copy()
            out[f"norm{n}/{k}"] = np.array(float(np.linalg.norm(g.astype(np.float64))))
        opt.step()
        for k in xvec_grad_ref.GRAD_KEYS:
            out[f"step{n}/{k}"] = sd["xvector_extractor." + k].detach().numpy().ravel()[idx[k]].copy()
    path = os.path.join(HERE, "g14_etdnn_grads.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
