"""A torch restatement (any dtype, any device) of XVectorNet_ETDNN_12Layer.extract (utils/models.py:29-186) with
autograd, of the NPLDA head and of the SoftCdet loss (utils/models.py:251-300), shared by the x-vector gradient tests and
tests/golden/make_golden_xvec_grads.py.  A plain helper, not a conftest.

Every frame of an utterance is computed as the reference does it: per utterance, unfold c frames at dilation d
(column j Din + i = h[t + j d, i]), Linear, ReLU, (y - running_mean) / sqrt(running_var + eps), then mean and unbiased
std / var over time and lin11."""
import numpy as np
import torch

from tests import xvec_ref

# the 22 tensors the extractor backward produces, in the order of nplda_xvec_backward_f32's flat gradient
GRAD_KEYS = [f"tdnn{i}.kernel.{w}" for i in range(1, 11) for w in ("weight", "bias")] + ["lin11.weight", "lin11.bias"]
HEAD_KEYS = ["centering_and_LDA.weight", "centering_and_LDA.bias", "centering_and_wccn_plda.weight",
             "centering_and_wccn_plda.bias", "P_sqrt", "Q"]


def torch_params(params, dtype=torch.float64, device="cpu"):
    """{key: tensor}: the GRAD_KEYS tensors require grad, the batch-norm statistics do not."""
    out = {}
    for k, v in params.items():
        t = torch.tensor(np.asarray(v), dtype=dtype, device=device)
        out[k] = t.requires_grad_(k in GRAD_KEYS)
    return out


def extract_one(x, P, pooling="std"):
    """x (T, 30) tensor -> (512,)."""
    h = x
    for i, (din, dout, c, d) in enumerate(xvec_ref.LAYERS, 1):
        Tn = h.shape[0] - d * (c - 1)
        U = torch.cat([h[j * d:j * d + Tn] for j in range(c)], dim=1)
        y = torch.relu(U @ P[f"tdnn{i}.kernel.weight"].T + P[f"tdnn{i}.kernel.bias"])
        h = (y - P[f"tdnn{i}.bn.running_mean"]) / torch.sqrt(P[f"tdnn{i}.bn.running_var"] + xvec_ref.EPS)
    s = torch.var(h, 0) if pooling == "var" else torch.std(h, 0)
    pooled = torch.cat([h.mean(0), s])
    return pooled @ P["lin11.weight"].T + P["lin11.bias"]


def extract_ragged(frames, lengths, P, pooling="std"):
    """frames (sum T_u, 30) tensor -> (U, 512)."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return torch.stack([extract_one(frames[off[u]:off[u + 1]], P, pooling) for u in range(len(lengths))])


def extractor_grads(frames, lengths, params, G, pooling="std", dtype=torch.float64, device="cpu"):
    """{key: float64 ndarray} of d(sum(extract * G))/d(parameter) for the 22 GRAD_KEYS."""
    P = torch_params(params, dtype, device)
    X = torch.as_tensor(np.asarray(frames), dtype=dtype, device=device)
    xv = extract_ragged(X, lengths, P, pooling)
    g = torch.autograd.grad((xv * torch.as_tensor(np.asarray(G), dtype=dtype, device=device)).sum(),
                            [P[k] for k in GRAD_KEYS])
    return {k: v.detach().cpu().double().numpy() for k, v in zip(GRAD_KEYS, g)}


def head_scores(z1, z2, H):
    """Etdnn_Xvec_NeuralPlda.forward from x-vectors: H maps HEAD_KEYS to tensors."""
    def emb(x):
        y = x @ H["centering_and_LDA.weight"].T + H["centering_and_LDA.bias"]
        y = torch.nn.functional.normalize(y)
        return y @ H["centering_and_wccn_plda.weight"].T + H["centering_and_wccn_plda.bias"]
    a, b = emb(z1), emb(z2)
    P = H["P_sqrt"] * H["P_sqrt"]
    Q = H["Q"]
    return (a * Q * a).sum(1) + (b * Q * b).sum(1) + 2 * (a * P * b).sum(1)


def softcdet(s, t, thresholds, betas=(99.0, 199.0), alpha=15.0):
    """utils/models.py:274-279; thresholds: one tensor per beta."""
    losses = [(torch.sigmoid(alpha * (th - s)) * t).sum() / t.sum() +
              b * (torch.sigmoid(alpha * (s - th)) * (1 - t)).sum() / (1 - t).sum() for b, th in zip(betas, thresholds)]
    return sum(losses) / len(losses)


def e2e_loss(x1, x2, t, P, H, thresholds, pooling="std", alpha=15.0):
    """SoftCdet loss of Etdnn_Xvec_NeuralPlda on features x1, x2 (B, 30, T) tensors."""
    z1 = torch.stack([extract_one(x1[b].T, P, pooling) for b in range(x1.shape[0])])
    z2 = torch.stack([extract_one(x2[b].T, P, pooling) for b in range(x2.shape[0])])
    return softcdet(head_scores(z1, z2, H), t, thresholds, alpha=alpha)
