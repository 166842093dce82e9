#!/usr/bin/env python3
"""Throughput of the HIP E-TDNN x-vector extractor (XVectorNet_ETDNN_12Layer.extract) on one MI355X.

    python tools/bench_xvec.py [--utts 1000] [--cohort 10000] [--json OUT]
    python tools/bench_xvec.py --layers-from-trace <rocprofv3 kernel_trace.csv>

The timed run reports frames/s and x-vectors/s of the HIP path for a ragged batch (--utts utterances of 200..400 frames)
and a cohort of --cohort 3-second (300-frame) utterances, the algorithmic FLOP (from the layer shapes), and, on identical
(B, 30, 300) inputs, torch's own GPU path (F.unfold + matmul, the reference's arithmetic) and the CPU path (torch, thread
count stated).  Per-layer times come from a separate `rocprofv3 --kernel-trace` run of `--profile-only`: the second mode
reads its trace and prints each layer's time and share of the fp32 MFMA peak."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12  # FLOP/s, 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def make_model(dev):
    from neuralplda_amd import xvector
    m = xvector.XVectorNet_ETDNN_12Layer()
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for t in m.tdnns():
            K = t.kernel.in_features
            t.kernel.weight.copy_(torch.from_numpy(rng.standard_normal(t.kernel.weight.shape) / np.sqrt(K)))
            t.kernel.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(t.kernel.bias.shape)))
            t.bn.running_mean.copy_(torch.from_numpy(rng.uniform(0.2, 0.6, t.bn.running_mean.shape)))
            t.bn.running_var.copy_(torch.from_numpy(rng.uniform(0.2, 0.6, t.bn.running_var.shape)))
        m.lin11.weight.copy_(torch.from_numpy(rng.standard_normal((512, 3000)) / np.sqrt(3000)))
    return m.to(dev).eval().requires_grad_(False)


def torch_extract(m, x):
    """The reference's arithmetic (utils/models.py:29-96, 170-186) with torch ops on x's device."""
    h = x.transpose(1, 2)
    for t in m.tdnns():
        u = F.unfold(h.unsqueeze(1), (t.context_size, t.input_dim), stride=(1, t.input_dim), dilation=(t.dilation, 1))
        y = torch.relu(torch.matmul(u.transpose(1, 2), t.kernel.weight.t()) + t.kernel.bias)
        h = (y - t.bn.running_mean) / torch.sqrt(t.bn.running_var + t.bn.eps)
    pooled = torch.cat([h.mean(1), h.std(1)], 1)
    return pooled @ m.lin11.weight.t() + m.lin11.bias


def timed(fn, dev, reps):
    fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        best = min(best, e0.elapsed_time(e1) / 1e3)
    return best


def layer_table(trace_csv):
    from neuralplda_amd import xvector
    rows = list(csv.DictReader(open(trace_csv)))
    g = [r for r in rows if "xvec_gemm_kernel" in r.get("Kernel_Name", "")]
    durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in g]
    grid = [int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0) for r in g]
    n = len(durs) // 11 * 11
    per = np.array(durs[:n]).reshape(-1, 11)
    rows_per_call = np.array(grid[:n]).reshape(-1, 11)[:, 0] // 256 * 128  # tdnn1 grid.x = tiles (x 256 threads)
    out = []
    names = [f"tdnn{i}" for i in range(1, 11)] + ["lin11"]
    for li, (din, dout, c, _) in enumerate(list(xvector.LAYERS) + [(3000, 512, 1, 1)]):
        f = 2 * din * c * dout
        t = per[:, li].sum()
        work = (rows_per_call.sum() if li < 10 else None)
        out.append({"layer": names[li], "K": din * c, "N": dout, "s": float(t),
                    "frac_peak_rows_computed": (float(work * f / t / PEAK_F32_MFMA) if work is not None else None)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--cohort", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-utts", type=int, default=8)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true", help="one ragged extraction (for rocprofv3)")
    ap.add_argument("--layers-from-trace", default=None)
    a = ap.parse_args()
    if a.layers_from_trace:
        print(json.dumps({"layers": layer_table(a.layers_from_trace)}, indent=1))
        return
    from neuralplda_amd import xvector
    dev = torch.device("cuda:0")
    m = make_model(dev)
    rng = np.random.default_rng(1)
    lengths = rng.integers(200, 401, a.utts)
    frames = torch.from_numpy(rng.standard_normal((int(lengths.sum()), 30)).astype(np.float32)).to(dev)
    if a.profile_only:
        m.extract_ragged(frames, lengths)
        torch.cuda.synchronize(dev)
        return
    frame_flop, utt_flop = xvector.flops_per_frame()
    res = {"gpu": torch.cuda.get_device_name(dev), "flop_per_frame": frame_flop, "lin11_flop_per_utt": utt_flop}
    # ragged batch
    t = timed(lambda: m.extract_ragged(frames, lengths), dev, a.reps)
    F_ = int(lengths.sum())
    valid = int((lengths - xvector.CONTEXT).sum())
    res["ragged"] = {"utts": a.utts, "frames": F_, "s": t, "frames_per_s": F_ / t, "xvectors_per_s": a.utts / t,
                     "algorithmic_tflops": (F_ * frame_flop + a.utts * utt_flop) / t / 1e12,
                     "frac_fp32_mfma_peak": (F_ * frame_flop + a.utts * utt_flop) / t / PEAK_F32_MFMA,
                     "valid_frame_fraction": valid / F_}
    # cohort of 3-second utterances: HIP, torch GPU, CPU on the same (B, 30, 300) features
    T = 300
    x = torch.randn(a.cohort, 30, T, device=dev)
    t_hip = timed(lambda: m.extract(x), dev, a.reps)
    chunk = 1000
    t_torch = timed(lambda: [torch_extract(m, x[i:i + chunk]) for i in range(0, a.cohort, chunk)], dev, a.reps)
    with torch.no_grad():
        d = (m.extract(x[:64]) - torch_extract(m, x[:64])).abs().max().item()
    mc = make_model(torch.device("cpu"))
    xc = x[:a.cpu_utts].cpu()
    torch_extract(mc, xc[:1])
    t0 = time.perf_counter()
    torch_extract(mc, xc)
    t_cpu = (time.perf_counter() - t0) / a.cpu_utts * a.cohort
    flop = a.cohort * (T * frame_flop + utt_flop)
    res["cohort"] = {"utts": a.cohort, "T": T, "frames": a.cohort * T, "algorithmic_flop": flop,
                     "hip_s": t_hip, "hip_frames_per_s": a.cohort * T / t_hip, "hip_xvectors_per_s": a.cohort / t_hip,
                     "hip_frac_fp32_mfma_peak": flop / t_hip / PEAK_F32_MFMA,
                     "torch_gpu_s": t_torch, "torch_gpu_xvectors_per_s": a.cohort / t_torch,
                     "speedup_vs_torch_gpu": t_torch / t_hip, "max_abs_diff_vs_torch_gpu": d,
                     "cpu_threads": torch.get_num_threads(), "cpu_s_extrapolated": t_cpu,
                     "cpu_measured_utts": a.cpu_utts}
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
