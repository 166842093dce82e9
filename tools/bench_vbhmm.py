#!/usr/bin/env python
"""VB-HMM resegmentation (ops.vbhmm, csrc/nplda_vbhmm.hip) against the route a user has today, on one GPU.

Shapes at D2 = 150, S = 16 speaker slots, max_iters = 10 with epsilon = -inf (ten iterations whatever the data):
  256 and 2048 problems of 300 rows;  one problem of 2048 and one of 16384 rows
Baseline on the same machine: the float64 numpy twin of tests/vbhmm_ref.py (the published log-domain form) on ONE host core
(the BLAS and OpenMP pools are held to one thread), problem after problem; for a batch it is timed on --twin-problems of the
problems and scaled to the batch (marked "extrapolated").
Device events around windows of about 20 ms of calls (one call where a call is longer); the kernel is warmed up; medians and
minima over the rounds.  One JSON line per (shape, variant) and one summary line.

A problem runs on ONE workgroup, so one CU: us per iteration is reported for the single problems, and the fp64 FMAs of the
two products per iteration (2 T S D) as a share of ONE CU's vector fp64 rate (64 FMA per clock at 2.4 GHz: an estimate from
the peak figures, not a measured roof)."""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # before numpy loads its BLAS: the baseline is one host core

import argparse  # noqa: E402
import json  # noqa: E402
import statistics  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CU_F64_FMA_PER_S = 64 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", type=int, nargs="*", default=[2048, 16384])
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--batch-n", type=int, default=300)
    ap.add_argument("--speakers", type=int, default=16)
    ap.add_argument("--dim", type=int, default=150)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--twin-problems", type=int, default=4)
    ap.add_argument("--twin-max-rows", type=int, default=16384)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vbhmm: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import ops
    from tests import vbhmm_ref as vr
    dev = torch.device("cuda:0")
    D2, S, iters = args.dim, args.speakers, args.iters
    ld = (D2 + 15) // 16 * 16
    summary = {}

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / reps

    shapes = [(p, args.batch_n) for p in args.batches] + [(1, n) for n in args.single]
    for nprob, n in shapes:
        nsrc = min(nprob, 8)                                   # distinct recordings; a batch repeats them
        src = [vr.make_problem(100 + k, n, S, D2, 2.0, K=6) for k in range(nsrc)]
        psi = src[0][1]
        x = np.zeros((nprob * n, ld), np.float32)
        lab = np.empty(nprob * n, np.int32)
        for p in range(nprob):
            x[p * n:(p + 1) * n, :D2], lab[p * n:(p + 1) * n] = src[p % nsrc][0], src[p % nsrc][2]
        z, labd, psid = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(psi).to(dev)
        offs = ops.RaggedOffsets(np.arange(nprob + 1, dtype=np.int64) * n, dev)
        spk = ops.RaggedOffsets(np.arange(nprob + 1, dtype=np.int64) * S, dev)
        run = lambda: ops.vbhmm(z, offs, spk, psid, labels_init=labd, epsilon=float("-inf"), max_iters=iters)  # noqa: E731
        out = run()
        assert (out[3] == iters).all().item() and torch.isfinite(out[2]).all().item()
        ntw = min(nprob, args.twin_problems) if n <= args.twin_max_rows else 0
        twin_s = []
        for p in range(ntw):
            t0 = time.perf_counter()
            tw = vr.vbhmm(src[p % nsrc][0], psi, vr.gamma_from_labels(src[p % nsrc][2], S), eps=-np.inf, max_iters=iters)
            twin_s.append(time.perf_counter() - t0)
            got = out[0][p * n * S:(p + 1) * n * S].cpu().numpy().reshape(n, S)
            assert np.abs(got - tw.gamma).max() <= 1e-6, float(np.abs(got - tw.gamma).max())
        del out
        reps = max(1, min(200, int(0.02 / max(timed(run, 1), 1e-6))))
        ts = [timed(run, reps) for _ in range(args.rounds)]
        med = statistics.median(ts)
        fma = 2.0 * nprob * n * S * D2 * iters
        rec = {"problems": nprob, "rows": n, "S": S, "D2": D2, "iters": iters, "variant": "vbhmm", "rounds": args.rounds,
               "calls_per_round": reps, "median_s": med, "min_s": min(ts)}
        if nprob == 1:
            rec["us_per_iteration"] = med * 1e6 / iters
            rec["product_fma_share_of_one_cu_f64_estimate"] = fma / med / CU_F64_FMA_PER_S
        print(json.dumps(rec), flush=True)
        summary[f"vbhmm_{nprob}x{n}_ms"] = round(med * 1e3, 4)
        if twin_s:
            per = statistics.median(twin_s)
            rec = {"problems": nprob, "rows": n, "S": S, "D2": D2, "iters": iters, "variant": "numpy_twin_one_core",
                   "problems_timed": ntw, "median_s_per_problem": per, "batch_s": per * nprob, "extrapolated": ntw < nprob}
            print(json.dumps(rec), flush=True)
            summary[f"numpy_twin_{nprob}x{n}_ms"] = round(per * nprob * 1e3, 2)
        del z, labd, run
        torch.cuda.empty_cache()
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
