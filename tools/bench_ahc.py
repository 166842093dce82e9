#!/usr/bin/env python
"""Score matrix and agglomerative clustering (ops.score_matrix / ops.ahc, csrc/nplda_ahc.hip) against the route a user has
today, on one GPU.

Shapes at D2 = 150, average linkage, full dendrogram:
  one problem of n in {1024, 4096, 16384};  256 and 2048 problems of n = 300
Score matrix and clustering are timed separately.  Baselines on the same machine:
  matrix      torch.matmul in its tightest form: the self terms ride in the GEMM ([2 P z_i, q_i, 1] against [z_j, 1, q_j], the
              second side augmented once outside the timed call), one bmm over the problems of a batch
  clustering  the device-to-host copy of the matrix plus scipy.cluster.hierarchy.linkage(method="average") on -S, problem after
              problem; skipped with a note where scipy is not importable, and above --scipy-max-n rows (minutes per call)
Device events around windows of about 20 ms of calls (one call where a call is longer); every variant is warmed up, then the
variants alternate inside each round of one process; medians and minima over the rounds.  One JSON line per (shape, variant)
and one summary line.

FLOP of the matrix kernel: 2 Dp per score of every 16 x 16 piece it forms (the pieces that hold some i < j), as a share of
the fp32-input MFMA peak (157.3 TFLOP/s).  The clustering of ONE problem runs on ONE workgroup, so one CU: us per merge is
reported for those shapes."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", type=int, nargs="*", default=[1024, 4096, 16384])
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--batch-n", type=int, default=300)
    ap.add_argument("--dim", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-max-n", type=int, default=4096)
    ap.add_argument("--scipy-max-problems", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ahc: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import ops
    try:
        from scipy.cluster.hierarchy import linkage as scipy_linkage
    except ImportError:
        scipy_linkage = None
        print(json.dumps({"note": "scipy is not importable here: no clustering baseline"}), flush=True)
    dev = torch.device("cuda:0")
    D2 = args.dim
    g = torch.Generator(device="cpu").manual_seed(D2)
    ps = (torch.rand(D2, generator=g) * 0.7 + 0.3).to(dev)
    Q = (-(torch.rand(D2, generator=g) * 0.5 + 0.1)).to(dev)
    zero = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    packed = ops.pack_params(zero(D2, 16), zero(D2), zero(D2, D2), zero(D2), ps, Q)
    Dp, P = packed.ldz, ps * ps
    summary = {}

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / reps

    shapes = [(1, n) for n in args.single] + [(p, args.batch_n) for p in args.batches]
    for nprob, n in shapes:
        N = nprob * n
        z = torch.zeros(N, Dp, device=dev)
        z[:, :D2] = (torch.randn(N, D2, generator=g) * 0.08).to(dev)
        q = (z[:, :D2] * z[:, :D2]) @ Q
        offs = ops.RaggedOffsets(np.arange(nprob + 1, dtype=np.int64) * n, dev)
        aug_l = torch.cat([z[:, :D2] * (2.0 * P), q[:, None], torch.ones_like(q)[:, None]], dim=1).view(nprob, n, D2 + 2)
        aug_r = torch.cat([z[:, :D2], torch.ones_like(q)[:, None], q[:, None]], dim=1).view(nprob, n, D2 + 2).transpose(1, 2)
        S = ops.score_matrix(z, q, packed, offs)
        ref = torch.bmm(aug_l, aug_r)
        off = ~torch.eye(n, dtype=torch.bool, device=dev)
        assert ((S.view(nprob, n, n) - ref).abs()[:, off].max() <= 1e-4 * ref.abs().max()).item()
        del ref, off
        variants = {"score_matrix": lambda: ops.score_matrix(z, q, packed, offs), "torch_bmm": lambda: torch.bmm(aug_l, aug_r),
                    "ahc": lambda: ops.ahc(S, offs, "average")}
        if scipy_linkage is not None and n <= args.scipy_max_n and nprob <= args.scipy_max_problems:
            iu = np.triu_indices(n, 1)

            def scipy_route():
                host = S.view(nprob, n, n).cpu().numpy()
                for p in range(nprob):
                    scipy_linkage(-host[p][iu].astype(np.float64), method="average")
            variants["copy_scipy"] = scipy_route
        elif scipy_linkage is not None:
            print(json.dumps({"note": f"scipy baseline skipped at {nprob} x {n} (--scipy-max-n / --scipy-max-problems)"}), flush=True)
        out = ops.ahc(S, offs, "average")
        assert (out[1] == n - 1).all().item() and (out[2] == 1).all().item()
        del out

        def wall(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        times = {name: [] for name in variants}
        reps = {}
        for name, fn in variants.items():
            if name == "copy_scipy":
                reps[name] = 1
            else:
                reps[name] = max(1, min(200, int(0.02 / max(timed(fn, 1), 1e-6))))
        rounds = args.rounds if n < 16384 else min(args.rounds, 3)
        for _ in range(rounds):
            for name, fn in variants.items():
                times[name].append(wall(fn) if name == "copy_scipy" else timed(fn, reps[name]))
        pieces = (n + 15) // 16
        flop = nprob * (pieces * (pieces + 1) // 2) * 256 * 2 * Dp
        for name, ts in times.items():
            med = statistics.median(ts)
            rec = {"problems": nprob, "n": n, "D2": D2, "variant": name, "rounds": rounds, "calls_per_round": reps[name],
                   "median_s": med, "min_s": min(ts)}
            if name == "score_matrix":
                rec["executed_flop"] = flop
                rec["executed_share_of_f32_mfma_peak"] = flop / med / PEAK_F32_MFMA
            if name == "ahc":
                rec["merges"] = nprob * (n - 1)
                rec["us_per_merge_of_one_problem" if nprob == 1 else "us_per_merge_over_the_batch"] = med * 1e6 / (nprob * (n - 1))
            print(json.dumps(rec), flush=True)
            summary[f"{name}_{nprob}x{n}_ms"] = round(med * 1e3, 4)
        del variants, S, z, q, aug_l, aug_r
        torch.cuda.empty_cache()
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
