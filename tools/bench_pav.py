#!/usr/bin/env python3
"""Measure the PAV / ROC-convex-hull kernels (csrc/nplda_pav.hip) on one GPU; one JSON line per measurement.

    python tools/bench_pav.py [--n 10000000] [--p-target 0.01] [--seps 2,3,4] [--reps 10] [--warmup 2] [--no-host]

Workload: N fp32 scores, a fraction p-target of targets, Gaussian classes `sep` standard deviations apart.  Per sep:
  * metrics.min_cllr as a call (device events around `reps` calls after `warmup`; its allocations and the read-back of
    the summary are inside), and its stages, from nplda_pav_fit_stages_f32 cut short after the sort and scan, the
    binning and the hull — each a difference of two event timings of the C call on a preallocated workspace;
  * score_calibration.fit_pav + an apply of the N scores; the apply kernel alone;
  * two yardsticks from the same process on the same data: metrics.minc_exact (the same sort and scan with a one-pass
    sweep: the floor a sort-bound call can reach) and, unless --no-host, the host route numpy.argsort +
    scipy.optimize.isotonic_regression + the fp64 sums (time.perf_counter).
No pass mark.  Device-event timings are wall times of the stream; the GPU clock is whatever the card runs at under this load
(read it from rocm-smi next to the run when quoting numbers).  No GPU: the measurements fail (there is no fall-back).
"""
import argparse
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--p-target", type=float, default=0.01)
    ap.add_argument("--seps", default="2,3,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from neuralplda_amd import _lib, metrics, ops, score_calibration as sc
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    N = a.n
    for sep in [float(x) for x in a.seps.split(",")]:
        rg = np.random.default_rng(int(10 * sep))
        y = (rg.random(N) < a.p_target).astype(np.float32)
        s = (rg.standard_normal(N) + sep * y).astype(np.float32)
        S, T = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
        base = dict(n=N, p_target=a.p_target, sep=sep, reps=a.reps)
        mc = metrics.min_cllr(S, T)
        med, mn = device_time(lambda: metrics.min_cllr(S, T), a.reps, a.warmup)
        print(json.dumps(dict(base, what="min_cllr_call", ms_median=med, ms_min=mn, min_cllr=mc,
                              rocch_eer=metrics.rocch_eer(S, T))), flush=True)
        # stages: the C call alone on a preallocated workspace
        nbytes = lib.nplda_pav_workspace_bytes(N, 0)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        cap = 1 << 16
        fl = torch.empty(3 * cap + 8, dtype=torch.float64, device=dev)
        it = torch.empty(2 * cap, dtype=torch.int64, device=dev)

        def staged(stop):
            with _lib.on_device(dev):
                code = lib.nplda_pav_fit_stages_f32(_lib.ptr(S), _lib.ptr(T), N, 0, fl.data_ptr(), fl.data_ptr() + 8 * cap,
                                                    it.data_ptr(), it.data_ptr() + 8 * cap, fl.data_ptr() + 16 * cap, cap,
                                                    fl.data_ptr() + 24 * cap, _lib.ptr(ws), nbytes, stop,
                                                    _lib.current_stream())
            _lib.check(code, "nplda_pav_fit_stages_f32")

        cum = {}
        for name, stop in (("sort", 1), ("binning", 2), ("hull", 3), ("finish", 0)):
            cum[name] = device_time(lambda: staged(stop), a.reps, a.warmup)[0]
        rep = dict(zip(ops.PAV_SUMMARY, fl[3 * cap:].tolist()))
        print(json.dumps(dict(base, what="min_cllr_stages", ms_sort=cum["sort"], ms_binning=cum["binning"] - cum["sort"],
                              ms_hull=cum["hull"] - cum["binning"], ms_finish=cum["finish"] - cum["hull"],
                              ms_c_call=cum["finish"], bins=rep["bins"], blocks=rep["blocks"],
                              workspace_mb=nbytes / 2 ** 20)), flush=True)
        model = sc.fit_pav(S, T)
        med, mn = device_time(lambda: sc.fit_pav(S, T).apply(S), a.reps, a.warmup)
        lo, hi, llr = (torch.from_numpy(x).to(dev) for x in (model.lo, model.hi, model.llr))
        amed, _ = device_time(lambda: ops.pav_apply(S, lo, hi, llr), a.reps, a.warmup)
        print(json.dumps(dict(base, what="fit_pav_plus_apply", ms_median=med, ms_min=mn, ms_apply_kernel=amed,
                              blocks=int(model.llr.size))), flush=True)
        med, mn = device_time(lambda: metrics.minc_exact(S, T, [99.0]), a.reps, a.warmup)
        print(json.dumps(dict(base, what="yardstick_minc_exact", ms_median=med, ms_min=mn)), flush=True)
        if not a.no_host:
            import scipy.optimize
            t0 = time.perf_counter()
            order = np.argsort(s, kind="stable")
            t1 = time.perf_counter()
            p = scipy.optimize.isotonic_regression(y[order].astype(np.float64)).x
            t2 = time.perf_counter()
            yt = y[order] > 0.5
            nt, nn = float(yt.sum()), float((~yt).sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                ct = np.where(p[yt] > 0, np.log1p((1 - p[yt]) / p[yt] * nt / nn), np.inf)
                cn = np.where(p[~yt] < 1, np.log1p(p[~yt] / (1 - p[~yt]) * nn / nt), np.inf)
            host = (ct.sum() / nt + cn.sum() / nn) / (2 * np.log(2))
            t3 = time.perf_counter()
            print(json.dumps(dict(base, what="yardstick_host_numpy_scipy", ms_total=1e3 * (t3 - t0), ms_argsort=1e3 * (t1 - t0),
                                  ms_isotonic=1e3 * (t2 - t1), ms_sums=1e3 * (t3 - t2), min_cllr=float(host),
                                  abs_diff_to_device=abs(float(host) - mc))), flush=True)


if __name__ == "__main__":
    main()
