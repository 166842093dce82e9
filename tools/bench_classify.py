#!/usr/bin/env python
"""Fused speaker-classification loss (ops.classify_loss, csrc/nplda_classify.hip) against dense torch, on one GPU.

For N in {1024, 4096, 16384} embeddings of D = 150 features against C in {7323, 13539} classes, AAM-softmax (s = 30, m = 0.2):
  (a) fused       ops.classify_loss with every gradient (dx, dw)
  (b) fused_loss  ops.classify_loss without any gradient (loss, rowloss, pred, counts)
  (c) dense       the same loss in dense torch fp32 with autograd on the same GPU (F.normalize, F.linear, the margin on the
                  target, F.cross_entropy), with its peak memory beside the fused call's workspace
Device events around windows of about 20 ms of calls; every variant is warmed up, then the variants alternate inside each round
of one process and the median and the minimum over the rounds are reported.  Every (N, C) runs in a child process of its own
under a time limit; the first child that fails ends the run.  One JSON line per (N, C, variant), and one summary line.

FLOP: the fused form recomputes the logits in both gradient passes — five products of 2 N C D (one for the loss pass, two in
each gradient pass) where a dense route does three (logits, dX, dW); the executed count is taken on the padded shapes
(N and C to 64, D to nplda_padded_dim) and reported as a share of the fp32-input MFMA peak (157.3 TFLOP/s: 256 CUs x 4 SIMDs x
64 FLOP/clk at 2.4 GHz)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
SCALE, MARGIN = 30.0, 0.2


def one(N, C, D, rounds):
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import _lib, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(0)
    W = torch.randn(C, D, generator=g).to(dev)
    y = torch.randint(0, C, (N,), generator=g).to(dev)
    x = (W[y] + 1.5 * torch.randn(N, D, generator=g).to(dev)).contiguous()
    y32 = y.to(torch.int32)
    rows = torch.arange(N, device=dev)
    cm, sm = math.cos(MARGIN), math.sin(MARGIN)

    def dense():
        xx, ww = x.detach().requires_grad_(True), W.detach().requires_grad_(True)
        u = F.linear(F.normalize(xx), F.normalize(ww))
        ut = u[rows, y]
        phi = torch.where(ut > -cm, ut * cm - torch.sqrt((1 - ut * ut).clamp_min(2.0 ** -24)) * sm, ut - MARGIN * sm)
        L = F.cross_entropy((SCALE * u).index_put((rows, y), SCALE * phi), y)
        L.backward()
        return L.detach(), xx.grad, ww.grad

    variants = {"fused": lambda: ops.classify_loss(x, y32, W, kind="aam", scale=SCALE, margin=MARGIN),
                "fused_loss": lambda: ops.classify_loss(x, y32, W, kind="aam", scale=SCALE, margin=MARGIN, want_dx=False,
                                                        want_dw=False),
                "dense": dense}
    # the routes compute the same thing: loss and both gradients agree
    ref, d = variants["fused"](), dense()
    assert abs(d[0].item() - ref.loss.item()) <= 1e-4 * abs(ref.loss.item()), (d[0].item(), ref.loss.item())
    assert (d[1] - ref.dx).abs().max().item() <= 1e-3 * ref.dx.abs().max().item()
    assert (d[2] - ref.dw).abs().max().item() <= 1e-3 * ref.dw.abs().max().item()
    assert variants["fused_loss"]().loss.item() == ref.loss.item()
    del ref, d
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dense()
    dense_peak = torch.cuda.max_memory_allocated() - base

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / reps

    reps = {name: max(1, min(200, int(0.02 / max(timed(fn, 2), 1e-6)))) for name, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps[name]))
    Dp = lib.nplda_padded_dim(D, D)
    Np, Cp = (N + 63) // 64 * 64, (C + 63) // 64 * 64
    wsb = lib.nplda_classify_workspace_bytes(N, C, D, 0, 0)
    for name, ts in times.items():
        med, lo = statistics.median(ts), min(ts)
        rec = {"N": N, "C": C, "D": D, "variant": name, "rounds": rounds, "calls_per_round": reps[name], "median_s": med,
               "min_s": lo, "logits_bytes": 4 * N * C}
        if name == "dense":
            rec["peak_bytes"] = dense_peak
        else:
            products = 5 if name == "fused" else 1
            rec["workspace_bytes"] = wsb
            rec["executed_products_of_2NCD"] = products
            rec["executed_flop"] = products * 2 * Np * Cp * Dp
            rec["executed_share_of_f32_mfma_peak"] = rec["executed_flop"] / med / PEAK_F32_MFMA
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096, 16384])
    ap.add_argument("--classes", type=int, nargs="*", default=[7323, 13539])
    ap.add_argument("--dim", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds for the child process of one (N, C)")
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "C"), help="run this shape in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one[0], args.one[1], args.dim, args.rounds)
        return
    summary = {}
    for C in args.classes:
        for N in args.sizes:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(N), str(C), "--dim", str(args.dim), "--rounds",
                   str(args.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
                sys.stderr.write(r.stderr)
                raise SystemExit(f"bench_classify: N = {N}, C = {C} ended with status {r.returncode}")
            for line in r.stdout.splitlines():
                rec = json.loads(line)
                summary[f"{rec['variant']}_N{N}_C{C}_ms"] = round(rec["median_s"] * 1e3, 4)
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
