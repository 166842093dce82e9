#!/usr/bin/env python3
"""Forward + backward time of the HIP E-TDNN extractor (XVectorNet_ETDNN_12Layer with enable_backward()) on one MI355X.

    python tools/bench_xvec_train.py [--pairs 64] [--big-utts 1000] [--iters 5] [--json OUT] [--profile-only]

Timed cases: a training batch of --pairs pairs x 2 sides of 200..400-frame utterances (one extract_ragged per side, as
Etdnn_Xvec_NeuralPlda.forward runs them), and one ragged batch of --big-utts utterances (~300 k frames), each followed
by backward of sum(x-vectors * G).  Reported: ms per forward + backward, frames/s, and the algorithmic FLOP rate as a
fraction of the fp32 MFMA peak (forward 2 K N per layer; backward the data gradients of tdnn2..tdnn10 and lin11 plus the
weight gradients of all eleven layers).  The comparison is torch autograd on the same GPU over the reference's
arithmetic (unfold + Linear per utterance, tests/xvec_grad_ref.py) for the training batch.  --profile-only runs the
large case once (for `rocprofv3 --kernel-trace --stats -- python tools/bench_xvec_train.py --profile-only`).

--batch-stats compares, in this process, the batch-statistics path (enable_batch_stats() under .train(),
csrc/nplda_xvec_bn.hip) with the running-statistics path on the same two cases: forward + backward in alternating rounds,
device events, medians; and sets the overhead against the time the added memory traffic would take at --stream-tbps
(per frame, from the layer widths S = 9 x 2 KB + 6 KB: forward one statistics read and one read-modify-write, 3 S;
backward the two-sum pass over G and O and the apply pass over G, O, the mask bytes and dA, 5.25 S).  With --profile-only
it runs the large case once on the batch-statistics path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12  # FLOP/s


def flops(lengths):
    from neuralplda_amd import xvector
    frame, utt = xvector.flops_per_frame()
    din, dout, c, _ = xvector.LAYERS[0]
    tdnn1 = 2 * c * din * dout
    R, U = sum(lengths), len(lengths)
    fwd = frame * R + utt * U
    bwd = (2 * frame - tdnn1) * R + 2 * utt * U  # dgrad of tdnn2..10 + wgrad of all; lin11 dpooled + dW11
    return fwd, bwd


def make(dev, batch_stats=False):
    from neuralplda_amd import xvector
    from tests import xvec_ref
    m = xvector.XVectorNet_ETDNN_12Layer()
    xvec_ref.load_into(m, xvec_ref.make_params())
    if batch_stats:
        return m.to(dev).train().enable_backward().enable_batch_stats()
    return m.to(dev).eval().enable_backward()


def run_hip(m, sides, G, dev):
    m.zero_grad(set_to_none=True)
    loss = 0
    for (frames, lengths), g in zip(sides, G):
        loss = loss + (m.extract_ragged(frames, lengths) * g).sum()
    loss.backward()


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def added_traffic_bytes(frames):
    S = sum(4 * ((dout + 15) // 16 * 16) for dout in [512] * 9 + [1500])
    return (3 + 5.25) * S * frames


def compare_batch_stats(m, mb, cases, dev, rounds, tbps):
    """{case: medians of forward + backward on both paths, their ratio, and the overhead in units of the traffic time}."""
    out = {}
    for name, s, g in cases:
        ms = {"running": [], "batch": []}
        for model in (m, mb):  # warm-up: allocator, packed images
            run_hip(model, s, g, dev)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for key, model in (("running", m), ("batch", mb)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run_hip(model, s, g, dev)
                b.record()
                torch.cuda.synchronize()
                ms[key].append(a.elapsed_time(b))
        frames = sum(sum(l) for _, l in s)
        run_ms, bn_ms = float(np.median(ms["running"])), float(np.median(ms["batch"]))
        traffic_ms = added_traffic_bytes(frames) / (tbps * 1e12) * 1e3
        out[name] = {"frames": frames, "rounds": rounds, "ms_running_stats": round(run_ms, 3),
                     "ms_batch_stats": round(bn_ms, 3), "ratio": round(bn_ms / run_ms, 3),
                     "added_traffic_gb": round(added_traffic_bytes(frames) / 1e9, 2), "traffic_ms": round(traffic_ms, 3),
                     "overhead_over_traffic": round((bn_ms - run_ms) / traffic_ms, 2),
                     "ms_running_all": [round(v, 3) for v in ms["running"]],
                     "ms_batch_all": [round(v, 3) for v in ms["batch"]]}
    return out


def case(rng, n, dev):
    lengths = [int(v) for v in rng.integers(200, 401, n)]
    frames = torch.from_numpy(rng.standard_normal((sum(lengths), 30)).astype(np.float32)).to(dev)
    return frames, lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--big-utts", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--batch-stats", action="store_true")
    ap.add_argument("--stream-tbps", type=float, default=4.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    m = make(dev)
    big = case(rng, a.big_utts, dev)
    Gbig = [torch.from_numpy(rng.standard_normal((a.big_utts, 512)).astype(np.float32)).to(dev)]
    if a.profile_only:
        run_hip(make(dev, True) if a.batch_stats else m, [big], Gbig, dev)
        torch.cuda.synchronize()
        return
    sides = [case(rng, a.pairs, dev) for _ in range(2)]
    G = [torch.from_numpy(rng.standard_normal((a.pairs, 512)).astype(np.float32)).to(dev) for _ in range(2)]
    out = {"gpu": torch.cuda.get_device_name(0), "iters": a.iters}
    if a.batch_stats:
        out.update(compare_batch_stats(m, make(dev, True), (("train_batch", sides, G), ("big", [big], Gbig)), dev,
                                       a.iters, a.stream_tbps))
        line = json.dumps(out)
        print(line)
        if a.json:
            with open(a.json, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    for name, s, g in (("train_batch", sides, G), ("big", [big], Gbig)):
        lengths = sum((l for _, l in s), [])
        ms = timed(lambda: run_hip(m, s, g, dev), a.iters)
        fwd, bwd = flops(lengths)
        out[name] = {"utterances": len(lengths), "frames": sum(lengths), "ms_fwd_bwd": round(ms, 3),
                     "frames_per_s": round(sum(lengths) / ms * 1e3), "gflop": round((fwd + bwd) / 1e9, 1),
                     "frac_fp32_peak": round((fwd + bwd) / (ms * 1e-3) / PEAK_F32_MFMA, 3)}
        msf = timed(lambda: [m.extract_ragged(f, l) for f, l in s], a.iters)
        out[name]["ms_fwd_only_train"] = round(msf, 3)
        out[name]["frac_bwd_fp32_peak"] = round(bwd / ((ms - msf) * 1e-3) / PEAK_F32_MFMA, 3)
    # torch autograd over the reference's arithmetic on the same GPU (fp32), the training batch only
    from tests import xvec_grad_ref as gref, xvec_ref
    P = gref.torch_params(xvec_ref.make_params(), torch.float32, dev)

    def run_torch():
        for p in P.values():
            p.grad = None
        loss = 0
        for (frames, lengths), g in zip(sides, G):
            loss = loss + (gref.extract_ragged(frames, lengths, P) * g).sum()
        loss.backward()
    ms_t = timed(run_torch, max(1, a.iters // 2))
    out["torch_autograd_train_batch_ms"] = round(ms_t, 3)
    out["speedup_vs_torch_autograd"] = round(ms_t / out["train_batch"]["ms_fwd_bwd"], 1)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
