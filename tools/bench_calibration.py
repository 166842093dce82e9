#!/usr/bin/env python3
"""Measure the calibration kernels (csrc/nplda_calib.hip) on one GPU and print one JSON line per measurement.

    python tools/bench_calibration.py [--n 10000000] [--ks 1,4] [--reps 20] [--warmup 3] [--numpy-fit]

At N recipe trials (tests/calib_ref.recipe, fp32 scores) and each K:
  * one logistic pass: the CALL time of ops.calib_logreg_pass (device events around `reps` calls, after `warmup`; its four
    launches and its workspace / output allocations are inside), with the share of two lower bounds it reaches:
      HBM:   4 N (K + 1) bytes (scores + labels) at 8.0 TB/s (spec) and at 6.3 TB/s (what a streaming read achieves);
      fp64:  N x (fp64 VALU instructions per trial) / (256 CUs x 64 lanes x 2.4 GHz = 39.3e12 lane-instructions / s).
    The instruction count is read off the ISA of the built kernel: `--count-isa` compiles csrc/nplda_calib.hip with
    --save-temps and counts the instructions whose mnemonic contains "f64" inside the innermost loop of
    pass_kernel<K, float> that holds the exp / log1p sequences (the per-trial body); FP64_INSTS below records the result.
    Every such instruction is charged one issue slot per lane (v_rcp_f64 and the divide helpers are slower: the bound is
    a lower bound).
  * a whole fit_linear: passes used; the time with the whole budget of 64 launch pairs enqueued at once, in chunks of 8
    with a look at the flags in between (the default), and with a budget of exactly the passes used — the difference to the
    first is the no-op tail;
  * the Gaussian fit, both apply kernels and calib_costs at three thresholds;
  * two baselines: the same Newton iteration composed of torch fp64 operations on the same GPU (a transcription of
    tests/calib_ref.py, what a user would write today), and tests/calib_ref.py in numpy on the host (one pass timed; the
    whole fit with --numpy-fit).
No GPU: the measurements fail (there is no fall-back); --count-isa needs none.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# fp64 VALU instructions in the per-trial loop body of pass_kernel<K, float> (hipcc 7.x, -O3, gfx950; --count-isa)
FP64_INSTS = {1: 158, 2: 165, 3: 173, 4: 182, 5: 192, 6: 203, 7: 215, 8: 228}
FP64_LANE_RATE = 256 * 64 * 2.4e9
HBM_SPEC, HBM_STREAM = 8.0e12, 6.3e12


def count_isa():
    import shutil
    from collections import Counter
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "neuralplda_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-c", os.path.join(csrc, "nplda_calib.hip"), "-o", os.path.join(tmp, "calib.o"), "--save-temps"],
                       cwd=tmp, check=True, capture_output=True)
        asm = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f][0]
        with open(os.path.join(tmp, asm)) as fh:
            txt = fh.read()
    out = {}
    for K in range(1, 9):
        name = re.search(r"^(_ZN\S*pass_kernelILi%dEfE\S*):" % K, txt, re.M).group(1)
        body = txt[txt.index("\n" + name + ":"):]
        lines = [ln.split(";")[0].strip() for ln in body[:body.index(".Lfunc_end")].splitlines()]
        lines = [ln for ln in lines if ln and (ln.startswith(".LBB") or not ln.startswith("."))]
        labels = {ln[:-1]: i for i, ln in enumerate(lines) if ln.startswith(".LBB") and ln.endswith(":")}
        best = None
        for i, ln in enumerate(lines):
            m = re.match(r"s_c?branch\w*\s+(\.LBB\S+)", ln)
            if m and labels.get(m.group(1), i) < i:  # a backward branch closes a loop
                seg = lines[labels[m.group(1)]:i + 1]
                c = Counter(s.split()[0] for s in seg)
                if any("rndne_f64" in k for k in c) and (best is None or len(seg) < best[0]):  # exp's range reduction
                    best = (len(seg), sum(v for k, v in c.items() if "f64" in k), sum(v for k, v in c.items() if k[:2] == "v_"))
        out[K] = {"loop_instructions": best[0], "fp64_instructions": best[1], "valu_instructions": best[2]}
    print(json.dumps({"what": "isa_count", "per_K": out}))


def device_time(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def host_time(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def torch_newton(X, t, p_target, l2, max_passes=64, tol=1e-10):
    """tests/calib_ref.newton with its pass composed of torch fp64 operations on the device of X."""
    import torch
    import torch.nn.functional as F
    N, K = X.shape
    A = torch.cat([X.double(), torch.ones(N, 1, dtype=torch.float64, device=X.device)], dim=1)
    tg = t > 0.5
    nt = int(tg.sum().item())
    f64 = dict(dtype=torch.float64, device=X.device)
    w = torch.where(tg, torch.tensor(p_target / nt, **f64), torch.tensor((1.0 - p_target) / (N - nt), **f64))
    tau = float(torch.logit(torch.tensor(p_target, dtype=torch.float64)))
    ridge = torch.cat([torch.ones(K), torch.zeros(1)]).double().to(X.device) * l2

    def one_pass(theta):
        z = A @ theta + tau
        sp, sn = torch.sigmoid(z), torch.sigmoid(-z)
        J = (w * torch.where(tg, F.softplus(-z), F.softplus(z))).sum() + 0.5 * (ridge * theta * theta).sum()
        g = A.T @ (w * torch.where(tg, -sn, sp)) + ridge * theta
        H = (A * (w * sp * sn)[:, None]).T @ A + torch.diag(ridge)
        return J, g, H

    acc = torch.cat([torch.full((K,), 1.0 / K), torch.zeros(1)]).double().to(X.device)
    trial, have, j_acc, alpha, halvings, passes, d = acc.clone(), False, float("nan"), 1.0, 0, 0, None
    while passes < max_passes:
        J, g, H = one_pass(trial)
        passes += 1
        Jv = J.item()
        if not have or Jv <= j_acc + 8 * 2.220446049250313e-16 * abs(j_acc):
            acc, have, j_acc = trial, True, Jv
            if g.abs().max().item() <= tol:
                break
            d = torch.cholesky_solve(g[:, None], torch.linalg.cholesky(H))[:, 0]
            alpha, halvings = 1.0, 0
        else:
            if halvings >= 20:
                break
            halvings += 1
            alpha *= 0.5
        trial = acc - alpha * d
    return acc, passes, one_pass


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--ks", default="1,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--p-target", type=float, default=0.05)
    ap.add_argument("--numpy-fit", action="store_true", help="time the whole numpy fit, not one pass")
    ap.add_argument("--count-isa", action="store_true", help="count the fp64 instructions per trial from the ISA and exit")
    args = ap.parse_args()
    if args.count_isa:
        return count_isa()
    import numpy as np
    import torch
    from neuralplda_amd import metrics, ops, score_calibration as sc
    from tests import calib_ref as cr
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration needs a HIP device")
    dev = torch.device("cuda", 0)
    N, p = args.n, args.p_target

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    for K in [int(k) for k in args.ks.split(",")]:
        Xh, th = cr.recipe(N, K)
        X, T = torch.from_numpy(Xh).to(dev), torch.from_numpy(th).to(dev)
        theta0 = torch.from_numpy(np.append(np.full(K, 1.0 / K), 0.0)).to(dev)
        t_pass = device_time(lambda: ops.calib_logreg_pass(X, T, theta0, p_target=p), args.reps, args.warmup)
        nbytes = 4 * N * (K + 1)
        insts = FP64_INSTS.get(K)
        emit(what="pass", N=N, K=K, call_seconds=t_pass, bytes=nbytes, hbm_bound_spec_s=nbytes / HBM_SPEC,
             hbm_bound_stream_s=nbytes / HBM_STREAM, share_of_hbm_spec=nbytes / HBM_SPEC / t_pass,
             share_of_hbm_stream=nbytes / HBM_STREAM / t_pass, fp64_insts_per_trial=insts,
             fp64_bound_s=None if insts is None else N * insts / FP64_LANE_RATE,
             share_of_fp64_bound=None if insts is None else N * insts / FP64_LANE_RATE / t_pass,
             note="call time of ops.calib_logreg_pass: 4 launches (clear, count, pass, finish) plus its workspace and output allocations")
        # the whole fit
        model = sc.fit_linear(X, T, p_target=p)
        used = model.passes

        def fit(max_passes, chunk):
            th0 = theta0.clone()
            return ops.calib_logreg_fit(X, T, th0, p_target=p, max_passes=max_passes, chunk=chunk)

        reps = max(3, args.reps // 4)
        t_full = host_time(lambda: fit(64, None), reps, 1)
        t_chunk = host_time(lambda: fit(64, 8), reps, 1)
        t_exact = host_time(lambda: fit(used, None), reps, 1)
        t_user = host_time(lambda: sc.fit_linear(X, T, p_target=p), reps, 1)
        emit(what="fit", N=N, K=K, passes=used, iterations=model.iterations, converged=model.converged,
             objective=model.objective, grad_inf=model.grad_inf, seconds_budget64_one_call=t_full,
             seconds_budget64_chunks_of_8=t_chunk, seconds_budget_exact=t_exact, seconds_fit_linear=t_user,
             noop_tail_seconds=t_full - t_exact, noop_tail_share=(t_full - t_exact) / t_full)
        # baselines
        tw = time.perf_counter()
        acc_t, passes_t, one_pass = torch_newton(X, T, p, 0.0)
        torch.cuda.synchronize()
        t_torch_first = time.perf_counter() - tw
        t_torch = host_time(lambda: torch_newton(X, T, p, 0.0), max(2, reps // 2), 0)
        t_torch_pass = device_time(lambda: one_pass(acc_t), max(3, reps // 2), 1)
        emit(what="baseline_torch_fp64", N=N, K=K, passes=passes_t, seconds_fit=t_torch, seconds_fit_first_call=t_torch_first,
             seconds_pass=t_torch_pass, max_abs_dtheta_vs_kernel=float(np.abs(acc_t.cpu().numpy() - np.append(model.a, model.b)).max()),
             fit_speedup=t_torch / t_user, pass_speedup=t_torch_pass / t_pass)
        t0 = time.perf_counter()
        if args.numpy_fit:
            _, info = cr.newton(Xh, th, p, 0.0)
            t_np = time.perf_counter() - t0
            emit(what="baseline_numpy", N=N, K=K, passes=info["passes"], seconds_fit=t_np, fit_speedup=t_np / t_user)
        else:
            cr.logreg_pass(Xh, th, np.append(model.a, model.b), p, 0.0)
            t_np = time.perf_counter() - t0
            emit(what="baseline_numpy", N=N, K=K, seconds_pass=t_np, pass_speedup=t_np / t_pass,
                 seconds_fit_extrapolated=t_np * used, note="one pass timed; fit = passes x pass")
        if K == 1:
            s = X[:, 0].contiguous()
            t_gfit = device_time(lambda: ops.calib_gauss_fit(s, T), args.reps, args.warmup)
            g = sc.calibrate_train(s, T)
            t_gapp = device_time(lambda: ops.calib_apply_gauss(s, g.mu_tgt, g.std_tgt, g.mu_imp, g.std_imp), args.reps, args.warmup)
            emit(what="gauss", N=N, seconds_fit=t_gfit, seconds_apply_f64_out=t_gapp, fit_bytes=2 * 8 * N,
                 fit_share_of_hbm_stream=2 * 8 * N / HBM_STREAM / t_gfit, apply_bytes=12 * N,
                 apply_share_of_hbm_stream=12 * N / HBM_STREAM / t_gapp)
            llr = model.apply(X)
            ths = [float(np.log(b)) for b in (99.0, 199.0, 9.9)]
            t_cost = device_time(lambda: ops.calib_costs(llr, T, ths), args.reps, args.warmup)
            emit(what="costs", N=N, thresholds=3, seconds=t_cost, cllr=metrics.cllr(llr, T),
                 act_cost=metrics.act_cost(llr, T, [99.0, 199.0, 9.9])[0])
        theta = torch.from_numpy(np.append(model.a, model.b)).to(dev)
        t_lin64 = device_time(lambda: ops.calib_apply_linear(X, theta), args.reps, args.warmup)
        t_lin32 = device_time(lambda: ops.calib_apply_linear(X, theta, out_dtype=torch.float32), args.reps, args.warmup)
        emit(what="apply_linear", N=N, K=K, seconds_f64_out=t_lin64, seconds_f32_out=t_lin32,
             share_of_hbm_stream_f32_out=4 * N * (K + 1) / HBM_STREAM / t_lin32)
        del X, T


if __name__ == "__main__":
    main()
