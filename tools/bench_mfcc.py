#!/usr/bin/env python3
"""Cost of the MFCC kernel (16-bit audio -> 30 cepstra per frame) next to the extraction it feeds.

    python tools/bench_mfcc.py [--utts 10000] [--seconds 4] [--reps 7] [--json profiles/r09a_bench_mfcc.json]

--utts utterances of --seconds of 16 kHz audio (noise, three sinusoids and a recording offset), the 30-bin configuration
(20 - 7600 Hz, 30 cepstra, snip_edges=false):

  (a) copy:  the int16 samples and the two offset tables to the device                                   device events
  (b) mfcc:  nplda_mfcc_frames_f32, ONE launch for every utterance                                       device events
  (c) xvec:  XVectorNet_ETDNN_12Layer.extract_ragged on the same frames, in the same run                 device events

Every figure is the median of --reps runs after one warm-up, with the minimum and maximum next to it.  The kernel's
fraction of the fp32 MFMA peak counts 2 N P + 2 (P / 2) B + 2 B C FLOP per frame against 157.3 TFLOP/s.  Nothing is gated:
the ratio (b) / (c) is what design/k14_mfcc.md records next to its expectation of 10 %."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_features import dev_timed  # noqa: E402
from tools.bench_xvec import make_model  # noqa: E402

PEAK_FP32_MFMA = 157.3e12


def synth_audio(utts, n, distinct=64, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    base = []
    for _ in range(min(distinct, utts)):
        x = rng.standard_normal(n) * 3000.0 + 2000.0
        for f, a in ((220.0, 4000.0), (1330.0, 2500.0), (3100.0, 1500.0)):
            x += a * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
        base.append(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
    samples = np.empty(utts * n, dtype=np.int16)
    for u in range(utts):
        samples[u * n:(u + 1) * n] = base[u % len(base)]
    return samples, np.arange(utts + 1, dtype=np.int64) * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=10000)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from neuralplda_amd import _lib, mfcc
    dev = torch.device("cuda:0")
    lib = _lib.load()
    o = mfcc.MfccOptions(sample_frequency=16000, num_mel_bins=30, num_ceps=30, low_freq=20, high_freq=7600, snip_edges=False)
    samples, offsets = synth_audio(a.utts, int(a.seconds * 16000))
    lengths = [int(t) for t in mfcc.num_frames(np.diff(offsets), o)]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    R, U = int(starts[-1]), a.utts
    N, P, B, C = o.frame_size, o.padded_size, o.num_mel_bins, o.num_ceps
    flop = 2 * N * P + 2 * (P // 2) * B + 2 * B * C
    res = {"gpu": torch.cuda.get_device_name(dev), "utts": U, "seconds_per_utt": a.seconds, "frames": R,
           "sample_bytes": int(samples.nbytes), "flop_per_frame": flop,
           "command": " ".join(["python", "tools/bench_mfcc.py"] + sys.argv[1:])}
    holder = {}

    def copy():
        holder["s"] = torch.from_numpy(samples).to(dev)
        holder["so"] = torch.from_numpy(offsets).to(dev)
        holder["fo"] = torch.from_numpy(starts).to(dev)
    res["a_h2d_copy"] = dev_timed(copy, dev, a.reps)
    res["a_h2d_copy"]["GB_per_s"] = samples.nbytes / res["a_h2d_copy"]["median_s"] / 1e9
    plan = mfcc.MfccPlan.get(o, dev)
    frames = torch.empty((R, C), dtype=torch.float32, device=dev)
    st = _lib.current_stream(dev)
    s, so, fo = holder["s"], holder["so"], holder["fo"]

    def k_mfcc():
        _lib.check(lib.nplda_mfcc_frames_f32(s.data_ptr(), so.data_ptr(), fo.data_ptr(), U, R, ctypes.addressof(plan.geometry),
                                             plan.window.data_ptr(), plan.dft.data_ptr(), plan.bank.data_ptr(),
                                             plan.dct.data_ptr(), frames.data_ptr(), st), "mfcc")
    res["b_mfcc_kernel"] = dev_timed(k_mfcc, dev, a.reps)
    t = res["b_mfcc_kernel"]["median_s"]
    res["b_mfcc_kernel"]["tflops"] = flop * R / t / 1e12
    res["b_mfcc_kernel"]["fraction_of_fp32_mfma_peak"] = flop * R / t / PEAK_FP32_MFMA
    res["b_mfcc_kernel"]["times_real_time"] = U * a.seconds / t
    via_api, _ = mfcc.compute_mfcc(s, offsets, o)
    res["api_equals_direct_call"] = bool(torch.equal(via_api, frames))
    m = make_model(dev)
    res["c_extract_ragged"] = dev_timed(lambda: m.extract_ragged(frames, lengths), dev, max(3, a.reps // 2))
    res["b_over_c"] = t / res["c_extract_ragged"]["median_s"]
    res["expected_b_over_c"] = 0.10
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    with torch.no_grad():
        sys.exit(main())
