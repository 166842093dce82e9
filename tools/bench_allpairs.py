#!/usr/bin/env python
"""All-pairs training step (ops.allpairs_loss, csrc/nplda_allpairs.hip) against what it replaces, on one GPU.

For N in {1024, 4096, 16384} utterances of D2 in {150, 170} features, SoftCdet with K = 2, the time of
  (a) allpairs   ops.allpairs_loss: loss, dtheta, dz, dP_sqrt, dQ over the N (N - 1) / 2 trials of the batch
  (b) dense      the same loss in dense torch fp32 with autograd on the same GPU (what a user would write today)
  (c) pairwise   N <= 4096: the project's pairwise route on the explicit i < j list: forward_from_plda_embeddings + loss +
                 backward
Device events around windows of about 20 ms of calls; every variant is warmed up, then the variants alternate inside each
round of one process and the median and the minimum over the rounds are reported.  One JSON line per (N, D2, variant), and one summary line.

FLOP: the algorithm needs 6 D2 per unordered pair (2 D2 for the score, 2 D2 for each of the two rows of A it feeds);
(a) walks the full square on features padded to Dp = nplda_padded_dim: 8 Dp per unordered pair executed.  Both are reported as
shares of the fp32-input MFMA peak (157.3 TFLOP/s, MI355X_MICROARCH: 256 CUs x 4 SIMDs x 64 FLOP/clk at 2.4 GHz)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
BETA, ALPHA, THETA = [99.0, 199.0], 15.0, [-0.8, -0.6]


def make(N, D2, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = (torch.randn(N, D2, generator=g) * 0.08).to(dev)
    ps = (torch.rand(D2, generator=g) * 0.7 + 0.3).to(dev)
    Q = (-(torch.rand(D2, generator=g) * 0.5 + 0.1)).to(dev)
    spk = torch.from_numpy(np.repeat(np.arange((N + 7) // 8), 8)[:N].astype(np.int32)).to(dev)   # 8 utterances per speaker
    th = [torch.tensor([v], device=dev) for v in THETA]
    return z, ps, Q, spk, th


def masks(spk):
    """Target / non-target masks of the upper triangle: labels only, built once outside the timed call."""
    N = spk.shape[0]
    trial = torch.ones(N, N, dtype=torch.bool, device=spk.device).triu(1)
    tgt = (trial & (spk[:, None] == spk[None, :])).float()
    return tgt, trial.float() - tgt


def dense_torch(z, ps, Q, th, tgt, non):
    z, ps, Q = z.detach().requires_grad_(True), ps.detach().requires_grad_(True), Q.detach().requires_grad_(True)
    th = [t.detach().requires_grad_(True) for t in th]
    q = (Q * z * z).sum(1)
    S = q[:, None] + q[None, :] + 2 * (z * (ps * ps)) @ z.T
    L = 0
    for t, b in zip(th, BETA):
        L = L + (torch.sigmoid(ALPHA * (t - S)) * tgt).sum() / tgt.sum() + b * (torch.sigmoid(ALPHA * (S - t)) * non).sum() / non.sum()
    L = L / len(th)
    L.backward()
    return L.detach(), z.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096, 16384])
    ap.add_argument("--dims", type=int, nargs="*", default=[150, 170])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairwise-max", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_allpairs: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import _lib, models, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    summary = {}
    for D2 in args.dims:
        Dp = lib.nplda_padded_dim(D2, D2)

        class NC:
            xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim = 512, D2, D2
            beta, alpha, device, loss = BETA, ALPHA, "cuda:0", "SoftCdet"

        for N in args.sizes:
            z, ps, Q, spk, th = make(N, D2, dev)
            trials = N * (N - 1) // 2
            tgt, non = masks(spk)
            variants = {"allpairs": lambda: ops.allpairs_loss(z, spk, ps, Q, th, BETA, ALPHA, ops.LOSS_SOFTCDET),
                        "dense": lambda: dense_torch(z, ps, Q, th, tgt, non)}
            if N <= args.pairwise_max:
                m = models.NeuralPlda(NC()).to(dev)
                with torch.no_grad():
                    m.P_sqrt.copy_(ps)
                    m.Q.copy_(Q)
                    for b, v in zip(m.beta, THETA):
                        m.threshold[b].fill_(v)
                ii, jj = torch.triu_indices(N, N, 1, device=dev)
                t = (spk[ii] == spk[jj]).float()

                def pairwise():
                    zz = z.detach().requires_grad_(True)
                    m.zero_grad(set_to_none=True)
                    L = m.loss(m.forward_from_plda_embeddings(zz[ii], zz[jj]), t)
                    L.backward()
                    return L.detach(), zz.grad

                variants["pairwise"] = pairwise
            # the three routes compute the same thing (Section 6 of the measuring guide): loss and dz agree
            ref = variants["allpairs"]()
            for name, fn in variants.items():
                out = fn()
                loss, dz = (out[0], out[3]) if name == "allpairs" else out
                assert abs(loss.item() - ref[0].item()) <= 1e-4 * abs(ref[0].item()), (name, loss.item(), ref[0].item())
                assert (dz - ref[3]).abs().max().item() <= 1e-3 * ref[3].abs().max().item(), name
            def timed(fn, reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e-3 / reps

            # warm-up; then as many calls per timed window as fill about 20 ms
            reps = {name: max(1, min(200, int(0.02 / max(timed(fn, 2), 1e-6)))) for name, fn in variants.items()}
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    times[name].append(timed(fn, reps[name]))
            for name, ts in times.items():
                med, lo = statistics.median(ts), min(ts)
                rec = {"N": N, "D2": D2, "variant": name, "trials": trials, "rounds": args.rounds, "calls_per_round": reps[name], "median_s": med, "min_s": lo,
                       "trials_per_s": trials / med, "needed_flop": 6 * D2 * trials,
                       "needed_share_of_f32_mfma_peak": 6 * D2 * trials / med / PEAK_F32_MFMA}
                if name == "allpairs":
                    rec["executed_flop"] = 4 * Dp * N * N
                    rec["executed_share_of_f32_mfma_peak"] = 4 * Dp * N * N / med / PEAK_F32_MFMA
                print(json.dumps(rec), flush=True)
                summary[f"{name}_N{N}_D{D2}_ms"] = round(med * 1e3, 4)
            del variants
            torch.cuda.empty_cache()
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
