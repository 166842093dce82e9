#!/usr/bin/env python3
"""Generate tests/golden/g15_etdnn_bn.npz by RUNNING THE REFERENCE's E-TDNN extractor under a plain .train()
(utils/models.py:29-186: every tdnn batch norm on the statistics of the batch, running statistics updated).

Runs only where the reference is available (like make_golden_xvec.py).  Weights are not stored: the generator and the
tests both build them from a seed through tests/xvec_ref.py.  Stored: the input features (3 utterances of 40 frames),
the reference's XVectorNet_ETDNN_12Layer.extract output with std and with var pooling, and the ten running means and
variances and num_batches_tracked after that one call.

    python tests/golden/make_golden_xvec_bn.py

Reference symbols executed: XVectorNet_ETDNN_12Layer.{__init__, extract, state_dict}, TDNN.forward.
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

SHAPE = (3, 30, 40)


def main():
    torch.manual_seed(0)
    params = xvec_ref.make_params()
    x = np.random.default_rng(1515).standard_normal(SHAPE).astype(np.float32)
    out = {"x": x}
    for pool, fn in (("std", torch.std), ("var", torch.var)):
        m = refm.XVectorNet_ETDNN_12Layer(pooling_function=fn)
        xvec_ref.load_into(m, params).train()
        with torch.no_grad():
            out[pool] = m.extract(torch.from_numpy(x)).numpy()
        if pool == "std":  # the statistics do not depend on the pooling
            sd = m.state_dict()
            for i in range(1, 11):
                out[f"running_mean{i}"] = sd[f"tdnn{i}.bn.running_mean"].numpy()
                out[f"running_var{i}"] = sd[f"tdnn{i}.bn.running_var"].numpy()
                out[f"num_batches_tracked{i}"] = sd[f"tdnn{i}.bn.num_batches_tracked"].numpy()
    path = os.path.join(HERE, "g15_etdnn_bn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
