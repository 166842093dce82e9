#!/usr/bin/env python
"""Spectral clustering with an auto-tuned neighbour count (ops.spectral, csrc/nplda_spectral.hip) against the route a user has
without it, on one GPU.

Shapes: --batches problems of --batch-n rows (default 256 and 2048 of 300) with the first 1 and the first 6 candidates of the
default ladder; one problem of each --single size (default 1024 and nplda_spectral_max_n()) with one candidate.  Scores are
planted: (G + G^T) / 2 + 3 [same cluster], four clusters of equal size.
Baseline, on one host core: the device-to-host copy of the matrices, then per problem and candidate the k-nearest-neighbour
Laplacian in numpy, numpy.linalg.eigh, the eigengap count, and the k-means of the twin (tests/spectral_ref.py) on the chosen
cell.  It is timed on --baseline-problems problems and EXTRAPOLATED to the batch where the batch is larger; the record says so.
Device events around every call, a warm-up call per variant, the variants alternating inside each round, medians and minima
over the rounds.  A call above --long-call seconds is timed once after its warm-up, one above five times that not again
at all (rounds = 0: the first call is the measurement).  One JSON line per (shape, variant) and
one summary line.  To split a call by kernel run this tool once under `rocprofv3 --kernel-trace --stats -- python ...` with
--rounds 1 --baseline-problems 0.

FLOP of the eigensolver, an upper bound that counts no skipped piece: a sweep is ne - 1 steps of (ne / 2)^2 pieces of 32
operations and ne^2 / 2 row elements of 6, about 11 ne^3; times the sweeps the call reports; as a share of the fp64 vector
rate of the CUs the call can use (min(cells, 256) CUs of 128 FLOP per clock at 2.4 GHz: the 78.6 TFLOP/s of AMD's MI355X
data sheet over its 256 CUs)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CU_FP64 = 78.6e12 / 256


def host_route(S, cands, max_clusters):
    """One problem on the host: numpy graph, numpy.linalg.eigh per candidate, eigengap count, the twin's k-means."""
    from tests import spectral_ref as sr
    n = S.shape[0]
    best = None
    for c in cands:
        m = min(c, n - 1)
        T = S.astype(np.float64).copy()
        np.fill_diagonal(T, -np.inf)
        idx = np.argsort(-T, axis=1, kind="stable")[:, :m]
        B = np.zeros((n, n))
        B[np.arange(n)[:, None], idx] = 1.0
        A = (B + B.T) / 2
        lam, V = np.linalg.eigh(np.diag(A.sum(1)) - A)
        K = min(max_clusters, n - 1)
        gaps = np.diff(lam[:K + 1])
        k = int(np.argmax(gaps)) + 1
        r = c / (gaps[k - 1] / lam[-1])
        if best is None or r < best[0]:
            best = (r, k, V[:, :k])
    return sr.kmeans(best[2], best[1])[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", type=int, nargs="*", default=None)
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--batch-n", type=int, default=300)
    ap.add_argument("--candidates", type=int, nargs="*", default=[1, 6], help="how many candidates of the ladder, per variant")
    ap.add_argument("--max-clusters", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long-call", type=float, default=2.0)
    ap.add_argument("--baseline-problems", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    single = [1024, lib.nplda_spectral_max_n()] if args.single is None else args.single
    ladder = [c for c in ops.SPECTRAL_NEIGHBOURS if c >= 4]
    g = torch.Generator(device="cpu").manual_seed(25)
    summary = {}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    shapes = [(p, args.batch_n, args.candidates) for p in args.batches] + [(1, n, [1]) for n in single]
    for nprob, n, ncands in shapes:
        truth = (torch.arange(n) * 4) // n
        same = (truth[:, None] == truth[None, :]).float()
        S = torch.empty(nprob, n, n)
        for p in range(nprob):
            G = torch.randn(n, n, generator=g)
            S[p] = (G + G.T) / 2 + 3.0 * same
            S[p].fill_diagonal_(0.0)
        Sd = S.to(dev).view(-1)
        offs = ops.RaggedOffsets(np.arange(nprob + 1, dtype=np.int64) * n, dev)
        variants = {}
        for nc in ncands:
            cands = ladder[:nc] if nc > 1 else [8]
            variants[f"spectral_C{nc}"] = (cands, lambda cands=cands: ops.spectral(Sd, offs, cands, 1, args.max_clusters))
        times, info = {name: [] for name in variants}, {}
        for name, (cands, fn) in variants.items():
            t, out = timed(fn)                                       # warm-up, and the call's own report
            assert (out.converged == 1).all().item()
            lab = out.labels.view(nprob, n).cpu().numpy()
            ok = sum(np.array_equal(a[:, None] == a[None, :], same.numpy() > 0) for a in lab)
            info[name] = dict(first_call_s=t, sweeps=int(out.n_sweeps.sum().item()), cells=nprob * len(cands), recovered=int(ok),
                              workspace_bytes=ops.spectral_workspace_bytes(offs.host, len(cands)))
            del out
        for name, (cands, fn) in variants.items():
            rounds = 1 if info[name]["first_call_s"] > args.long_call else args.rounds
            if info[name]["first_call_s"] > 5 * args.long_call:      # a very long call: its first run is the measurement
                rounds, times[name] = 0, [info[name]["first_call_s"]]
            info[name]["rounds"] = rounds
        for r in range(max(v["rounds"] for v in info.values())):
            for name, (cands, fn) in variants.items():
                if r < info[name]["rounds"]:
                    times[name].append(timed(fn)[0])
        ne = n + (n & 1)
        for name, ts in times.items():
            med, v = statistics.median(ts), info[name]
            flop = 11.0 * ne ** 3 * v["sweeps"]
            cus = min(v["cells"], 256)
            rec = {"problems": nprob, "n": n, "variant": name, "candidates": variants[name][0], "rounds": v["rounds"],
                   "median_s": med, "min_s": min(ts), "first_call_s": v["first_call_s"], "sweeps_per_cell": v["sweeps"] / v["cells"],
                   "workspace_bytes": v["workspace_bytes"], "problems_recovered": v["recovered"],
                   "eigensolver_flop_upper_bound": flop, "whole_call_share_of_fp64_vector_rate_of_its_cus": flop / med / (cus * CU_FP64)}
            print(json.dumps(rec), flush=True)
            summary[f"{name}_{nprob}x{n}_ms"] = round(med * 1e3, 3)
        nb = min(args.baseline_problems, nprob) if n <= 1024 else 0
        if nb:
            host_route(Sd.view(nprob, n, n)[0].cpu().numpy(), [8], args.max_clusters)   # (LAPACK's first call is not the route's cost)
            for name, (cands, fn) in variants.items():
                t0 = time.perf_counter()
                host = Sd.view(nprob, n, n)[:nb].cpu().numpy()
                t_copy = (time.perf_counter() - t0) * nprob / nb
                t0 = time.perf_counter()
                for p in range(nb):
                    host_route(host[p], cands, args.max_clusters)
                t_host = (time.perf_counter() - t0) / nb
                rec = {"problems": nprob, "n": n, "variant": "host_" + name, "timed_problems": nb, "extrapolated": nb < nprob,
                       "seconds_per_problem": t_host, "copy_s": t_copy, "total_s": t_copy + t_host * nprob}
                print(json.dumps(rec), flush=True)
                summary[f"host_{name}_{nprob}x{n}_ms"] = round(rec["total_s"] * 1e3, 3)
        else:
            print(json.dumps({"note": f"host baseline not measured at {nprob} x {n}"}), flush=True)
        del Sd, S, variants
        torch.cuda.empty_cache()
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
