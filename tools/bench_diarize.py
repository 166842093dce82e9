#!/usr/bin/env python3
"""Sliding-window x-vector extraction for diarization on one MI355X: XVectorNet_ETDNN_12Layer.extract_windows against the
two routes the package had before it.

    python tools/bench_diarize.py [--recordings 64] [--frames 60000] [--rounds 5] [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_diarize.py --profile-only [a|c]
    python tools/bench_diarize.py --shares-from-trace DIR/.../<pid>_kernel_trace.csv

--recordings recordings of --frames frames, every frame inside one segment, cut by diarize.uniform_windows at window 144 /
shift 24 and at window 150 / shift 75.  Timed, each ending in a device synchronise (host planning and copies included):
  (a) extract_windows over the recordings' frames and the window table;
  (b) the only route before it: gather a copy of every window's rows, then extract_ragged on the copies;
  (c) extract_ragged over the recordings as whole utterances: the GEMM work of (a) without windows (measured, it is no
      floor of (a): the utterance pooling kernel dominates it at this length, design/k23_sliding_windows.md).
One warm-up of each, then --rounds rounds that alternate (a), (b), (c); the median and the minimum of the rounds are
reported, with the ratios of the medians.  (a) and (b) are compared bit for bit on the timed inputs first.  Kernel shares
come from a separate rocprofv3 run of --profile-only (two calls of (a) at 144 / 24, or of (c)): the third mode sums the
second call's kernels by name, lin11 apart from tdnn1..tdnn10."""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONFIGS = ((144, 24), (150, 75))


def window_table(recordings, frames, window, shift):
    from neuralplda_amd import diarize
    segs = [np.array([[0, frames]], np.int64)] * recordings
    win, dropped = diarize.uniform_windows(segs, window, shift)
    assert not dropped
    return win[:, 2:4] + (win[:, 0] * frames)[:, None]


def cutout_index(table):
    """Row index of the gather that builds route (b)'s input: every window's rows, one after the other."""
    n = table[:, 1] - table[:, 0]
    starts = np.concatenate([[0], np.cumsum(n)])[:-1]
    return np.repeat(table[:, 0] - starts, n) + np.arange(int(n.sum())), n


def wall(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / 1e3


def shares(trace_csv):
    tot, gemms = {}, 0
    for r in sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"])):
        name = r.get("Kernel_Name", "")
        for key in ("xvec_pool_windows_kernel", "xvec_pool_kernel", "xvec_gemm_kernel", "xvec_prep_kernel"):
            if key in name:
                name = key
        if name == "xvec_gemm_kernel":  # every extraction call launches tdnn1..tdnn10, then lin11
            name += " (lin11)" if gemms % 11 == 10 else " (tdnn1..tdnn10)"
            gemms += 1
        tot.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    # the first half of the calls is the warm-up: the trace holds two identical calls of (a)
    out = {k: float(sum(v[len(v) // 2:])) for k, v in tot.items()}
    s = sum(out.values())
    return {"kernel_s": out, "share": {k: v / s for k, v in out.items()}, "total_kernel_s": s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", nargs="?", const="a", choices=["a", "c"], default=None,
                    help="two calls of (a) at 144 / 24, or of (c) (for rocprofv3)")
    ap.add_argument("--shares-from-trace", default=None)
    a = ap.parse_args()
    if a.shares_from_trace:
        print(json.dumps(shares(a.shares_from_trace), indent=1))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_diarize: no HIP device (nothing here is measured without one)")
    from bench_xvec import PEAK_F32_MFMA, make_model
    from neuralplda_amd import xvector
    dev = torch.device("cuda:0")
    m = make_model(dev)
    R = a.recordings * a.frames
    frames = torch.from_numpy(np.random.default_rng(1).standard_normal((R, 30)).astype(np.float32)).to(dev)
    if a.profile_only:
        table = window_table(a.recordings, a.frames, *CONFIGS[0])
        for _ in range(2):
            if a.profile_only == "a":
                m.extract_windows(frames, table)
            else:
                m.extract_ragged(frames, [a.frames] * a.recordings)
            torch.cuda.synchronize(dev)
        return
    frame_flop, utt_flop = xvector.flops_per_frame()
    res = {"gpu": torch.cuda.get_device_name(dev), "recordings": a.recordings, "frames_per_recording": a.frames,
           "rounds": a.rounds, "configs": []}
    whole = [a.frames] * a.recordings
    for window, shift in CONFIGS:
        table = window_table(a.recordings, a.frames, window, shift)
        idx_np, n = cutout_index(table)
        idx = torch.from_numpy(idx_np).to(dev)
        routes = {"a_extract_windows": lambda: m.extract_windows(frames, table),
                  "b_cutouts_extract_ragged": lambda: m.extract_ragged(frames.index_select(0, idx), n),
                  "c_whole_recordings": lambda: m.extract_ragged(frames, whole)}
        xa, xb = routes["a_extract_windows"](), routes["b_cutouts_extract_ragged"]()
        same = bool(torch.equal(xa, xb)) and bool(torch.isfinite(xa).all())
        del xa, xb
        routes["c_whole_recordings"]()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(wall(fn, dev))
        med = {k: statistics.median(v) for k, v in times.items()}
        W = int(table.shape[0])
        flop_a = R * frame_flop + W * utt_flop
        res["configs"].append({
            "window": window, "shift": shift, "windows": W, "cutout_frames": int(n.sum()), "a_equals_b_bit_for_bit": same,
            "median_s": med, "min_s": {k: min(v) for k, v in times.items()}, "all_s": times,
            "b_over_a": med["b_cutouts_extract_ragged"] / med["a_extract_windows"],
            "a_over_c": med["a_extract_windows"] / med["c_whole_recordings"],
            "a_frames_per_s": R / med["a_extract_windows"], "a_windows_per_s": W / med["a_extract_windows"],
            "a_algorithmic_tflops": flop_a / med["a_extract_windows"] / 1e12,
            "a_frac_fp32_mfma_peak_whole_call": flop_a / med["a_extract_windows"] / PEAK_F32_MFMA})
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
