#!/usr/bin/env python3
"""Measure the group-bootstrap kernels (csrc/nplda_bootstrap.hip) on one GPU; one JSON line per measurement.

    python tools/bench_bootstrap.py [--n 1000000,10000000] [--b 100,1000] [--groups 7323] [--p-target 0.01]
                                    [--betas 99,199] [--reps 5] [--warmup 1] [--no-host] [--no-torch] [--ref-reps 3]

Workload: N fp32 scores with a share p-target of targets (Gaussian classes 3 standard deviations apart), `groups` x
`groups` random groups.  Per (N, B), with and without is_llr:
  * the C call nplda_bootstrap_f32 on a preallocated workspace: device events around each of `reps` calls after `warmup`,
    median and minimum; the trial-replicate updates per second (N (B + 1) / time) and the bytes the two walks imply: per
    tile of 64 replicates and pass every position costs two 64-byte look-ups in the draw-count tables (L2) and its
    per-position fields from HBM (9 bytes, + 12 in pass 1 with is_llr);
  * (b) the same computation composed of torch operations on the same GPU, per replicate: w = c1[g1] * c2[g2] in sorted
    order, two cumsums, the cost at the tie starts, min (the sort is done once, outside the timing); `ref-reps`
    replicates are timed and the figure for B is EXTRAPOLATED linearly;
  * (a) unless --no-host, the numpy twin (tests/bootstrap_ref.py) on the host: the sort once plus `ref-reps` replicates,
    EXTRAPOLATED linearly to B.
The stages (sort + gather, count tables, pass 1, reduce, pass 2, finish) are separate kernels: their times are read from
a kernel trace of a run of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_bootstrap.py --no-host
--no-torch ...), not measured here.  No pass mark.  Device-event timings are wall times of the stream; the GPU clock is
whatever the card runs at under this load.  No GPU: the measurements fail (there is no fall-back).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def device_time(fn, reps, warmup):
    """Median and minimum milliseconds per call over `reps` separately timed calls."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def torch_replicate(ks_start, lab_t, lab_n, g1s, g2s, G, betas):
    """One replicate of baseline (b): fresh multinomial counts, weights, two cumsums, costs at the tie starts, min."""
    import torch
    dev = g1s.device
    c1 = torch.bincount(torch.randint(G, (G,), device=dev), minlength=G)
    c2 = torch.bincount(torch.randint(G, (G,), device=dev), minlength=G)
    w = (c1[g1s] * c2[g2s]).to(torch.float64)
    wt, wn = w * lab_t, w * lab_n
    ct, cn = torch.cumsum(wt, 0) - wt, torch.cumsum(wn, 0) - wn
    Nt, Nn = wt.sum(), wn.sum()
    pm, pf = ct / Nt, (Nn - cn) / Nn
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    return torch.stack([torch.where(ks_start, pm + b * pf, inf).min() for b in betas])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", default="1000000,10000000")
    ap.add_argument("--b", default="100,1000")
    ap.add_argument("--groups", type=int, default=7323)
    ap.add_argument("--p-target", type=float, default=0.01)
    ap.add_argument("--betas", default="99,199")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from neuralplda_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    betas = [float(b) for b in a.betas.split(",")]
    K, G = len(betas), a.groups
    barr = (ctypes.c_double * K)(*betas)
    T = lib.nplda_bootstrap_tile()
    for N in [int(x) for x in a.n.split(",")]:
        rg = np.random.default_rng(N % 1000)
        y = (rg.random(N) < a.p_target).astype(np.float32)
        s = (rg.standard_normal(N) + 3.0 * y).astype(np.float32)
        g1 = rg.integers(0, G, N).astype(np.int32)
        g2 = rg.integers(0, G, N).astype(np.int32)
        S, Y, A, C = (torch.from_numpy(x).to(dev) for x in (s, y, g1, g2))
        for B in [int(x) for x in a.b.split(",")]:
            nbytes = lib.nplda_bootstrap_workspace_bytes(N, G, G, B)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            for llr in (0, 1):
                ncol = K + 1 + (K + 1 if llr else 0)
                out = torch.empty((B + 1, ncol), dtype=torch.float64, device=dev)
                tot = torch.empty((B + 1, 2), dtype=torch.int64, device=dev)

                def call():
                    with _lib.on_device(dev):
                        code = lib.nplda_bootstrap_f32(_lib.ptr(S), _lib.ptr(Y), _lib.ptr(A), _lib.ptr(C), N, G, G, B, 1, barr, K,
                                                       llr, _lib.ptr(out), _lib.ptr(tot), _lib.ptr(ws), nbytes,
                                                       _lib.current_stream())
                    _lib.check(code, "nplda_bootstrap_f32")

                med, mn = device_time(call, a.reps, a.warmup)
                tiles = (B + 1 + T - 1) // T
                point = out[0].tolist()
                print(json.dumps(dict(what="bootstrap_c_call", n=N, b=B, groups=G, k=K, is_llr=llr, reps=a.reps, ms_median=med,
                                      ms_min=mn, updates_per_s=N * (B + 1) / (med * 1e-3),
                                      l2_table_gb=N * tiles * 2 * 128 / 1e9,
                                      hbm_field_gb=N * tiles * (2 * 9 + (12 if llr else 0)) / 1e9,
                                      workspace_mb=nbytes / 2 ** 20, flags=ws[:2].tolist(), point=point,
                                      std=out[1:].std(dim=0).tolist(), degenerate=int(torch.isnan(out[:, 0]).sum()))), flush=True)
        if not a.no_torch:
            order = torch.argsort(S, stable=True)
            ks = S[order]
            start = torch.cat([torch.ones(1, dtype=torch.bool, device=dev), ks[1:] != ks[:-1]])
            lab = Y[order]
            lab_t, lab_n = (lab > 0.5).to(torch.float64), (lab < 0.5).to(torch.float64)
            g1s, g2s = A[order].long(), C[order].long()
            med, mn = device_time(lambda: torch_replicate(start, lab_t, lab_n, g1s, g2s, G, betas), a.ref_reps, 1)
            print(json.dumps(dict(what="baseline_torch_per_replicate", n=N, groups=G, k=K, reps=a.ref_reps, ms_median=med,
                                  ms_min=mn, **{f"ms_extrapolated_b{B}": med * int(B) for B in a.b.split(",")})), flush=True)
            del order, ks, start, lab, lab_t, lab_n, g1s, g2s
        if not a.no_host:
            from tests import bootstrap_ref as br
            t0 = time.perf_counter()
            order, key, code, st = br.sort_trials(s, y)
            h1, h2 = g1.astype(np.int64)[order], g2.astype(np.int64)[order]
            t1 = time.perf_counter()
            for b in range(1, a.ref_reps + 1):
                w = br.counts(1, b, 0, G)[h1] * br.counts(1, b, 1, G)[h2]
                br.sweep(key, code, st, w, betas)
            t2 = time.perf_counter()
            per = (t2 - t1) / a.ref_reps
            print(json.dumps(dict(what="baseline_numpy_twin", n=N, groups=G, k=K, reps=a.ref_reps, s_sort=t1 - t0,
                                  s_per_replicate=per,
                                  **{f"s_extrapolated_b{B}": (t1 - t0) + per * int(B) for B in a.b.split(",")})), flush=True)


if __name__ == "__main__":
    main()
