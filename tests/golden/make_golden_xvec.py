#!/usr/bin/env python3
"""Generate tests/golden/g13_etdnn.npz by RUNNING THE REFERENCE's E-TDNN extractor (utils/models.py:29-345).

Runs only where the reference is available (like make_golden.py).  Weights are not stored: the generator and the tests
both build them from a seed through tests/xvec_ref.py.  Stored: the input features of three shapes, the reference's
XVectorNet_ETDNN_12Layer.extract output with std and with var pooling, Etdnn_Xvec_NeuralPlda.forward scores for the
features against their time-reversed copies with a seeded head, and the reference's state-dict keys and shapes.

    python tests/golden/make_golden_xvec.py

Reference symbols executed: XVectorNet_ETDNN_12Layer.{__init__, extract, state_dict}, TDNN.forward,
Etdnn_Xvec_NeuralPlda.{__init__, train1, forward, extract_plda_embeddings, forward_from_plda_embeddings}.
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

from tests import xvec_ref  # noqa: E402

SHAPES = ((3, 30, 40), (2, 30, 23), (1, 30, 97))


class NC:
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, 150, 150
    beta, alpha, device, loss, pooling_function = [99.0, 199.0], 15.0, "cpu", "SoftCdet", "std"


def main():
    torch.manual_seed(0)
    params, head = xvec_ref.make_params(), xvec_ref.make_head()
    out = {}
    ext = {}
    for pool, fn in (("std", torch.std), ("var", torch.var)):
        m = refm.XVectorNet_ETDNN_12Layer(pooling_function=fn)
        xvec_ref.load_into(m, params).eval()
        ext[pool] = m
    sd = ext["std"].state_dict()
    out["xvec_keys"] = np.array(list(sd.keys()))
    out["xvec_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    e = refm.Etdnn_Xvec_NeuralPlda(NC())
    xvec_ref.load_into(e.xvector_extractor, params)
    xvec_ref.load_into(e, head)
    e.train1()
    esd = e.state_dict()
    out["etdnn_keys"] = np.array(list(esd.keys()))
    out["etdnn_shapes"] = np.array([",".join(map(str, v.shape)) for v in esd.values()])
    rng = np.random.default_rng(1313)
    for n, shp in enumerate(SHAPES):
        x = rng.standard_normal(shp).astype(np.float32)
        X = torch.from_numpy(x)
        with torch.no_grad():
            out[f"x{n}"] = x
            out[f"std{n}"] = ext["std"].extract(X).numpy()
            out[f"var{n}"] = ext["var"].extract(X).numpy()
            out[f"score{n}"] = e(X, torch.from_numpy(np.ascontiguousarray(x[:, :, ::-1]))).numpy()
    path = os.path.join(HERE, "g13_etdnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
