#!/usr/bin/env python
"""Top-k search over an embedding table (ops.topk_scores, csrc/nplda_topk.hip) against the route a user has today, on one GPU.

Shapes, at D2 in {150, 170} and k in {10, 64}:
  search   R in {1, 1024, 16384} probes against a table of M = 1.2 M embeddings
  self     a 100 000-row table against itself under mask="different" (8 utterances per speaker, each row excluded from its own list)
Variants:
  (a) topk    ops.topk_scores: the R x M matrix is never written
  (b) torch   chunked torch.matmul + torch.topk with the same mask on the same GPU, the row chunk sized so that the fp32 score
              block stays within --block-bytes (default 2 GiB).  The self terms ride in the GEMM ([2 P z_r, q_r, 1] against
              [z_j, 1, q_j]; the table side is augmented once, outside the timed call), so the score block is written once and
              read by the mask and by topk only: the tightest composition of library calls, not the naive one
Device events around windows of about 20 ms of calls (one call where a call is longer); every variant is warmed up, then the
variants alternate inside each round of one process and the median and the minimum over the rounds are reported.  One JSON
line per (shape, D2, k, variant), and one summary line.

FLOP: 2 Dp per score executed (features padded to Dp = nplda_padded_dim), reported as a share of the fp32-input MFMA peak
(157.3 TFLOP/s, MI355X_MICROARCH: 256 CUs x 4 SIMDs x 64 FLOP/clk at 2.4 GHz), as the README's other fractions are."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12


def make_table(N, D2, ldz, dev, seed):
    """An embedding table as embed() leaves it: (N, ldz) with zero pad columns, q (N,)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.zeros(N, ldz, device=dev)
    step = 1 << 18
    for lo in range(0, N, step):
        n = min(step, N - lo)
        z[lo:lo + n, :D2] = (torch.randn(n, D2, generator=g) * 0.08).to(dev)
    return z


def augment_table(zt, qt, D2):
    """[z_j, 1, q_j] (M, D2 + 2): the table side of the one-GEMM score, built once per table."""
    return torch.cat([zt[:, :D2], torch.ones_like(qt)[:, None], qt[:, None]], dim=1)


def torch_route(zr, qr, aug_t, P, k, D2, block_bytes, lab_r=None, lab_t=None, self0=None):
    """What a user can write today: row chunks of [2 P z_r, q_r, 1] [z_j, 1, q_j]^T (one GEMM), the mask, torch.topk."""
    R, M = zr.shape[0], aug_t.shape[0]
    rows = max(1, min(R, block_bytes // (4 * M)))
    vals = torch.empty(R, k, device=zr.device)
    idx = torch.empty(R, k, dtype=torch.int64, device=zr.device)
    aug_r = torch.cat([zr[:, :D2] * (2.0 * P), qr[:, None], torch.ones_like(qr)[:, None]], dim=1)
    augT = aug_t.T
    for lo in range(0, R, rows):
        hi = min(R, lo + rows)
        S = torch.matmul(aug_r[lo:hi], augT)
        if lab_r is not None:
            S.masked_fill_(lab_r[lo:hi, None] == lab_t[None, :], float("-inf"))
        if self0 is not None:
            S[torch.arange(hi - lo, device=S.device), self0[lo:hi]] = float("-inf")
        vals[lo:hi], idx[lo:hi] = torch.topk(S, k, dim=1)
        del S
    return vals, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", type=int, default=1_200_000)
    ap.add_argument("--probes", type=int, nargs="*", default=[1, 1024, 16384])
    ap.add_argument("--self-rows", type=int, default=100_000)
    ap.add_argument("--dims", type=int, nargs="*", default=[150, 170])
    ap.add_argument("--ks", type=int, nargs="*", default=[10, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-bytes", type=int, default=2 << 30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import ops
    dev = torch.device("cuda:0")
    summary = {}

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / reps

    for D2 in args.dims:
        g = torch.Generator(device="cpu").manual_seed(D2)
        ps = (torch.rand(D2, generator=g) * 0.7 + 0.3).to(dev)
        Q = (-(torch.rand(D2, generator=g) * 0.5 + 0.1)).to(dev)
        zero = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        packed = ops.pack_params(zero(D2, 16), zero(D2), zero(D2, D2), zero(D2), ps, Q)  # (the search reads P only)
        Dp, P = packed.ldz, ps * ps
        zt = make_table(max(args.table, args.self_rows), D2, Dp, dev, 1)
        qt = (zt[:, :D2] * zt[:, :D2]) @ Q
        zp = make_table(max(args.probes), D2, Dp, dev, 2)
        qp = (zp[:, :D2] * zp[:, :D2]) @ Q
        lab = torch.from_numpy((np.arange(args.self_rows) // 8).astype(np.int32)).to(dev)
        me = torch.arange(args.self_rows, dtype=torch.int64, device=dev)
        shapes = [("search", R, args.table) for R in args.probes] + [("self", args.self_rows, args.self_rows)]
        for what, R, M in shapes:
            for k in args.ks:
                if what == "search":
                    a_r, a_q, a_t, a_tq = zp[:R], qp[:R], zt[:M], qt[:M]
                    aug = augment_table(a_t, a_tq, D2)
                    variants = {"topk": lambda: ops.topk_scores(a_r, a_q, a_t, a_tq, packed, k),
                                "torch": lambda: torch_route(a_r, a_q, aug, P, k, D2, args.block_bytes)}
                else:
                    a_t, a_tq = zt[:M], qt[:M]
                    aug = augment_table(a_t, a_tq, D2)
                    variants = {"topk": lambda: ops.topk_scores(a_t, a_tq, a_t, a_tq, packed, k, labels=(lab, lab),
                                                                mask="different", self_rows=me),
                                "torch": lambda: torch_route(a_t, a_tq, aug, P, k, D2, args.block_bytes, lab, lab)}
                # the two routes select the same columns, up to the rounding of two float32 evaluation orders at rank k
                got, ref = variants["topk"](), variants["torch"]()
                n = min(R, 256)
                same = sum(len(set(got[1][r].tolist()) & set(ref[1][r].tolist())) for r in range(n)) / (n * k)
                assert same >= 0.99, (what, R, D2, k, same)
                assert (got[0][:n] - ref[0][:n]).abs().max().item() <= 1e-4 * ref[0][:n].abs().max().item()
                del got, ref
                reps = {name: max(1, min(200, int(0.02 / max(timed(fn, 1), 1e-6)))) for name, fn in variants.items()}
                times = {name: [] for name in variants}
                for _ in range(args.rounds):
                    for name, fn in variants.items():
                        times[name].append(timed(fn, reps[name]))
                for name, ts in times.items():
                    med = statistics.median(ts)
                    rec = {"shape": what, "R": R, "M": M, "D2": D2, "k": k, "variant": name, "rounds": args.rounds,
                           "calls_per_round": reps[name], "median_s": med, "min_s": min(ts), "scores_per_s": R * M / med,
                           "index_agreement_with_other_route": same}
                    if name == "topk":
                        rec["executed_flop"] = 2 * Dp * R * M
                        rec["executed_share_of_f32_mfma_peak"] = 2 * Dp * R * M / med / PEAK_F32_MFMA
                    print(json.dumps(rec), flush=True)
                    summary[f"{name}_{what}_R{R}_D{D2}_k{k}_ms"] = round(med * 1e3, 4)
                del variants, aug
                torch.cuda.empty_cache()
        del zt, zp
        torch.cuda.empty_cache()
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
