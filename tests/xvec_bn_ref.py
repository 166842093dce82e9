"""The twin of the batch-statistics extractor (csrc/nplda_xvec_bn.hip): a torch restatement (any dtype, any device) of
XVectorNet_ETDNN_12Layer.extract (utils/models.py:170-186) under a plain model.train(), where each tdnn is unfold, Linear,
ReLU, then nn.BatchNorm1d(affine=False) on the statistics of the batch, with torch's running-statistics update.  Shared
by the batch-statistics tests.  A plain helper, not a conftest.

For tdnn layer l, V_l is the set of valid rows (index inside the utterance < T_u - ctx_l), n_l = |V_l|:

    R_l = ReLU(unfold(O_{l-1}) W_l^T + b_l)        mu_l = mean over V_l, v_l = biased variance over V_l
    O_l = (R_l - mu_l) / sqrt(v_l + eps)           running_mean <- (1 - m) running_mean + m mu_l
                                                   running_var  <- (1 - m) running_var  + m v_l n_l / (n_l - 1)

`masks`: None takes the ReLU branch from the twin's own pre-activation (pre > 0); a list of ten (total frames, >= Dout)
0/1 tables (rows in the caller's frame order) forces R_l = pre_l * mask_l, so that a float64 and a float32 run and the
device all take the same branches (pre-activations within rounding of 0 otherwise flip between them, and under batch
statistics one flip moves a gradient by 1e-3 to 5e-2 of its largest entry).  The gradients come from autograd through
these formulas, which yields dL/dR_l = (G_l - mean(G_l) - O_l mean(G_l O_l)) / sqrt(v_l + eps) on V_l."""
import numpy as np
import torch

from tests import xvec_ref
from tests.xvec_grad_ref import GRAD_KEYS, torch_params

CTX = (4, 4, 8, 8, 14, 14, 22, 22, 22, 22)
MOMENTUM = 0.1


def valid_rows(lengths, layer):
    """Indices (into the caller's frame order) of V_layer, utterance after utterance."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate([np.arange(off[u], off[u] + max(0, lengths[u] - CTX[layer])) for u in range(len(lengths))])


def forward(X, lengths, P, pooling="std", masks=None, momentum=MOMENTUM, eps=xvec_ref.EPS):
    """X (sum T_u, 30) tensor, P {key: tensor} -> dict(xvec (U, 512), pre [ten (n_l, Dout) pre-activations, V_l order],
    mean / uvar [ten batch means / unbiased variances], n [ten n_l], running_mean / running_var [ten updated buffers])."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    hs = [X[off[u]:off[u + 1]] for u in range(len(lengths))]
    out = {k: [] for k in ("pre", "mean", "uvar", "n", "running_mean", "running_var")}
    for l, (din, dout, c, d) in enumerate(xvec_ref.LAYERS):
        W, b = P[f"tdnn{l + 1}.kernel.weight"], P[f"tdnn{l + 1}.kernel.bias"]
        pres = []
        for h in hs:
            Tn = h.shape[0] - d * (c - 1)
            pres.append(torch.cat([h[j * d:j * d + Tn] for j in range(c)], dim=1) @ W.T + b)
        pre = torch.cat(pres)
        if masks is None:
            R = torch.relu(pre)
        else:
            m = torch.as_tensor(np.asarray(masks[l])[valid_rows(lengths, l)][:, :dout] != 0, device=pre.device)
            R = pre * m.to(pre.dtype)
        n = R.shape[0]
        mu = R.mean(0)
        v = ((R - mu) ** 2).mean(0)
        O = (R - mu) / torch.sqrt(v + eps)
        rm, rv = P[f"tdnn{l + 1}.bn.running_mean"], P[f"tdnn{l + 1}.bn.running_var"]
        out["pre"].append(pre)
        out["mean"].append(mu)
        out["uvar"].append(v * (n / (n - 1)))
        out["n"].append(n)
        out["running_mean"].append((1 - momentum) * rm + momentum * mu.detach())
        out["running_var"].append((1 - momentum) * rv + momentum * (v * (n / (n - 1))).detach())
        hs = list(torch.split(O, [p.shape[0] for p in pres]))
    xs = []
    for h in hs:
        s = torch.var(h, 0) if pooling == "var" else torch.std(h, 0)
        xs.append(torch.cat([h.mean(0), s]) @ P["lin11.weight"].T + P["lin11.bias"])
    out["xvec"] = torch.stack(xs)
    return out


def run(frames, lengths, params, G, pooling="std", dtype=torch.float64, device="cpu", masks=None, momentum=MOMENTUM):
    """float64 ndarrays of one training-mode call: dict(xvec, grads {GRAD_KEYS: d(sum(xvec * G)) / d(parameter)}, pre,
    mean, uvar, n, running_mean, running_var)."""
    P = torch_params(params, dtype, device)
    X = torch.as_tensor(np.asarray(frames), dtype=dtype, device=device)
    r = forward(X, lengths, P, pooling, masks, momentum)
    g = torch.autograd.grad((r["xvec"] * torch.as_tensor(np.asarray(G), dtype=dtype, device=device)).sum(),
                            [P[k] for k in GRAD_KEYS])
    num = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    res = {k: [num(t) for t in r[k]] for k in ("pre", "mean", "uvar", "running_mean", "running_var")}
    res.update(xvec=num(r["xvec"]), n=list(r["n"]), grads={k: num(v) for k, v in zip(GRAD_KEYS, g)})
    return res
