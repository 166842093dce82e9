"""Seeded E-TDNN extractor parameters and an fp64 (or fp32) NumPy restatement of XVectorNet_ETDNN_12Layer.extract
(utils/models.py:29-186), shared by tests/golden/make_golden_xvec.py and the x-vector tests.  A plain helper, not a
conftest.

Weights come from numpy's default_rng (PCG64) at a scale that keeps every layer's activations O(1): W ~ N(0, 1/K), small
biases, running means and variances near the mean and variance of a ReLU of a unit normal."""
import numpy as np

LAYERS = ((30, 512, 5, 1), (512, 512, 1, 1), (512, 512, 3, 2), (512, 512, 1, 1), (512, 512, 3, 3), (512, 512, 1, 1),
          (512, 512, 3, 4), (512, 512, 1, 1), (512, 512, 1, 1), (512, 1500, 1, 1))
EPS = 1e-5
CONTEXT = 22


def make_params(seed=13):
    """{state-dict key: float32 array} for tdnn1..tdnn10 (kernel.weight, kernel.bias, bn.running_mean, bn.running_var) and
    lin11."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (din, dout, c, _) in enumerate(LAYERS, 1):
        K = din * c
        p[f"tdnn{i}.kernel.weight"] = (rng.standard_normal((dout, K)) / np.sqrt(K)).astype(np.float32)
        p[f"tdnn{i}.kernel.bias"] = (0.1 * rng.standard_normal(dout)).astype(np.float32)
        p[f"tdnn{i}.bn.running_mean"] = rng.uniform(0.2, 0.6, dout).astype(np.float32)
        p[f"tdnn{i}.bn.running_var"] = rng.uniform(0.2, 0.6, dout).astype(np.float32)
    p["lin11.weight"] = (rng.standard_normal((512, 3000)) / np.sqrt(3000)).astype(np.float32)
    p["lin11.bias"] = (0.1 * rng.standard_normal(512)).astype(np.float32)
    return p


def make_head(seed=14, D0=512, D1=150, D2=150):
    """{key: float32 array} of the NPLDA head (centering_and_LDA, centering_and_wccn_plda, P_sqrt, Q)."""
    rng = np.random.default_rng(seed)
    return {"centering_and_LDA.weight": (rng.standard_normal((D1, D0)) / np.sqrt(D0)).astype(np.float32),
            "centering_and_LDA.bias": (0.1 * rng.standard_normal(D1)).astype(np.float32),
            "centering_and_wccn_plda.weight": (rng.standard_normal((D2, D1)) / np.sqrt(D1)).astype(np.float32),
            "centering_and_wccn_plda.bias": (0.1 * rng.standard_normal(D2)).astype(np.float32),
            "P_sqrt": rng.uniform(0.2, 1.0, D2).astype(np.float32),
            "Q": rng.uniform(-0.5, 0.1, D2).astype(np.float32)}


def load_into(module, params, prefix=""):
    """Copy `params` into a torch module's state dict (keys prefixed by `prefix`)."""
    import torch
    sd = module.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            sd[prefix + k].copy_(torch.from_numpy(v))
    return module


def extract_one(x, params, pooling="std", dtype=np.float64):
    """One utterance: x (T, 30) frames -> (512,) x-vector, every operation in `dtype`."""
    h = np.asarray(x, dtype=dtype)
    for i, (din, dout, c, d) in enumerate(LAYERS, 1):
        Tn = h.shape[0] - d * (c - 1)
        if Tn < 1:
            raise ValueError("utterance shorter than the context")
        U = np.concatenate([h[j * d:j * d + Tn] for j in range(c)], axis=1)  # column j Din + i = x[t + j d, i]
        W = params[f"tdnn{i}.kernel.weight"].astype(dtype)
        y = U @ W.T + params[f"tdnn{i}.kernel.bias"].astype(dtype)
        y = np.maximum(y, dtype(0))
        m = params[f"tdnn{i}.bn.running_mean"].astype(dtype)
        v = params[f"tdnn{i}.bn.running_var"].astype(dtype)
        h = (y - m) / np.sqrt(v + dtype(EPS))
    with np.errstate(invalid="ignore", divide="ignore"):
        var = h.var(axis=0, ddof=1) if h.shape[0] > 1 else np.full(h.shape[1], np.nan, dtype)
    s = var if pooling == "var" else np.sqrt(var)
    pooled = np.concatenate([h.mean(axis=0), s]).astype(dtype)
    return pooled @ params["lin11.weight"].astype(dtype).T + params["lin11.bias"].astype(dtype)


def extract(x, params, pooling="std", dtype=np.float64):
    """utils/models.py:170-186 on x (B, 30, T) -> (B, 512)."""
    x = np.asarray(x)
    return np.stack([extract_one(x[b].T, params, pooling, dtype) for b in range(x.shape[0])]) if x.shape[0] else \
        np.zeros((0, 512), dtype)


def extract_ragged(frames, lengths, params, pooling="std", dtype=np.float64):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.stack([extract_one(frames[off[u]:off[u + 1]], params, pooling, dtype) for u in range(len(lengths))])


def head_scores(z1, z2, head, dtype=np.float64):
    """Etdnn_Xvec_NeuralPlda.forward_from x-vectors (utils/models.py:244-261)."""
    def emb(x):
        y = x @ head["centering_and_LDA.weight"].astype(dtype).T + head["centering_and_LDA.bias"].astype(dtype)
        y = y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)
        return y @ head["centering_and_wccn_plda.weight"].astype(dtype).T + head["centering_and_wccn_plda.bias"].astype(dtype)
    a, b = emb(np.asarray(z1, dtype)), emb(np.asarray(z2, dtype))
    P = head["P_sqrt"].astype(dtype) ** 2
    Q = head["Q"].astype(dtype)
    return (a * Q * a).sum(1) + (b * Q * b).sum(1) + 2 * (a * P * b).sum(1)
