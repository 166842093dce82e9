#!/usr/bin/env python3
"""Cost of the resampler (csrc/nplda_resample.hip) against the HBM bound of its bytes and against the same polyphase filter
composed of torch operations.

    python tools/bench_resample.py [--utts 2000] [--seconds 3] [--reps 7] [--inner 20] [--json OUT] [--no-chain] [--profile-only]

--utts utterances of --seconds of audio (noise, three sinusoids and a recording offset), int16 in, int16 out, three workloads:

  speeds    16 kHz audio, a speed factor of (0.9, 1.0, 1.1) per utterance in turn: 9:10, a copy, 11:10 in ONE call
  16k->8k   2:1, 25 taps
  44k->16k  441:160, 34 taps (the audio is --seconds long at 44.1 kHz)

For each: (a) one prepared nplda_resample_batch call, launch() timed with device events, --inner launches per timed window,
the median of --reps windows after a warm-up, with the bytes the algorithm needs (2 per input sample, 2 per output sample)
over that time and over the HBM bound at 4 TB/s; (b) the same filter as torch operations on the same GPU: one strided
torch.nn.functional.conv1d per ratio against the bank of `ou` filters laid on their common support (torchaudio's
formulation), float32 in (the conversion from int16 is not timed), float32 out, no gain, no rounding, the copies of the
speeds workload left out; the two are compared on the first utterances.  (c), unless --no-chain: the speeds call's share of
augment (every perturbed utterance reverberated) + compute_mfcc + the extractor's forward and backward on those frames.
Nothing is gated.  --profile-only launches each workload twice, for `rocprofv3 --kernel-trace --stats -- python
tools/bench_resample.py --profile-only`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_features import dev_timed, stats  # noqa: E402
from tools.bench_mfcc import synth_audio  # noqa: E402

HBM = 4.0e12


def timed(fn, dev, reps, inner):
    """Seconds per call of fn: `inner` calls per window of device events."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) / 1e3 / inner)
    return stats(out)


def torch_bank(rate_in, rate_out, dev):
    """(iu, ou, left padding, weight (ou, 1, K) float32): the bank on the common support of its phases."""
    from neuralplda_amd import resample as rs
    iu, ou, first, w = rs.filter_bank(rate_in, rate_out)
    taps = w.shape[1]
    K = int(first[-1] - first[0]) + taps
    W = np.zeros((ou, 1, K), np.float32)
    for p in range(ou):
        W[p, 0, int(first[p] - first[0]):int(first[p] - first[0]) + taps] = w[p]
    return iu, ou, int(-first[0]), torch.from_numpy(W).to(dev)


def torch_resample(X, bank, m):
    """X (U, n) float32 -> (U, m): y[u, b ou + p] = sum_j W[p, j] x[u, b iu + first[0] + j]."""
    iu, ou, left, W = bank
    U, n = X.shape
    blocks = -(-m // ou)
    right = max(0, (blocks - 1) * iu + W.shape[2] - left - n)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(X, (left, right))[:, None, :], W, stride=iu)
    return y[:, :, :blocks].transpose(1, 2).reshape(U, blocks * ou)[:, :m]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    from neuralplda_amd import augment as ag, mfcc, resample as rs
    dev = torch.device("cuda:0")
    U = a.utts
    speeds = np.array([(0.9, 1.0, 1.1)[u % 3] for u in range(U)])
    work = {"speeds": (16000, rs.speed_rates(speeds, 16000), 16000), "16k->8k": (16000, 16000, 8000),
            "44k->16k": (44100, 44100, 16000)}
    res = {"gpu": torch.cuda.get_device_name(dev), "utts": U, "seconds_per_utt": a.seconds, "inner": a.inner,
           "command": " ".join(["python", "tools/bench_resample.py"] + sys.argv[1:])}
    preps = {}
    for name, (sr, rin, rout) in work.items():
        n = int(a.seconds * sr)
        samples, offsets = synth_audio(U, n, seed=len(name))
        d_samples = torch.from_numpy(samples).to(dev)
        preps[name] = (rs.prepare(d_samples, offsets, rin, rout, device=dev), d_samples, offsets, n)
    if a.profile_only:
        for prep, _, _, _ in preps.values():
            for _ in range(2):
                prep.launch()
        torch.cuda.synchronize(dev)
        return 0

    for name, (sr, rin, rout) in work.items():
        prep, d_samples, offsets, n = preps[name]
        r = timed(prep.launch, dev, a.reps, a.inner)
        t = r["median_s"]
        n_in, n_out = int(offsets[-1]), int(prep.offsets[-1])
        r.update(samples_in=n_in, samples_out=n_out, bytes=2 * (n_in + n_out), bytes_per_s=2 * (n_in + n_out) / t,
                 hbm_bound_s=2 * (n_in + n_out) / HBM, fraction_of_hbm_bound=2 * (n_in + n_out) / HBM / t,
                 times_real_time=U * a.seconds / t, chunks=int(prep.call.total_chunks))
        res[name] = r
        # (b) the torch composition, one conv1d per ratio on the utterances of that ratio
        rin_u = np.broadcast_to(np.asarray(rin), (U,))
        X = d_samples.view(U, n).float()
        groups = []
        for ri in sorted(set(rin_u.tolist())):
            if ri == rout:
                continue
            idx = np.nonzero(rin_u == ri)[0]
            groups.append((idx, X[torch.from_numpy(idx).to(dev)].contiguous(), torch_bank(int(ri), int(rout), dev),
                           int(rs.output_lengths(n, int(ri), int(rout)))))
        holder = {}

        def compose():
            holder["y"] = [torch_resample(Xg, bank, m) for _, Xg, bank, m in groups]
        rt = timed(compose, dev, a.reps, max(1, a.inner // 4))
        rt["ours_over_torch"] = t / rt["median_s"]
        got = rs.resample(d_samples, offsets, rin, rout, out_dtype=torch.float32, device=dev)
        worst = 0.0
        for (idx, _, _, m), y in zip(groups, holder["y"]):
            u = int(idx[0])
            mine = got[0][int(got[1][u]):int(got[1][u + 1])]
            worst = max(worst, float((mine - y[0]).abs().max() / y[0].square().mean().sqrt()))
        rt["max_abs_difference_over_rms"] = worst
        res[name]["torch_conv1d"] = rt
        del holder, groups, X

    if not a.no_chain:
        from tools.bench_augment import synth_rirs
        from tools.bench_xvec_train import make, run_hip
        prep = preps["speeds"][0]
        out, ooff, _ = prep.launch()
        rirs = ag.RirTable(synth_rirs(8, 8000), 16000)
        reverb = ag.prepare(out, ooff, ag.Recipe(np.arange(U) % 8), rirs, device=dev)
        res["chain_augment"] = dev_timed(reverb.launch, dev, a.reps)
        s2, o2, _ = reverb.launch()
        o = mfcc.MfccOptions(sample_frequency=16000, num_mel_bins=30, num_ceps=30, low_freq=20, high_freq=7600, snip_edges=False)
        holder = {}

        def k_mfcc():
            holder["f"] = mfcc.compute_mfcc(s2, o2, o)
        res["chain_mfcc"] = dev_timed(k_mfcc, dev, a.reps)
        frames, lengths = holder["f"]
        with torch.enable_grad():
            m = make(dev)
            G = [torch.randn(U, 512, device=dev)]
            res["chain_extractor_fwd_bwd"] = dev_timed(lambda: run_hip(m, [(frames, lengths)], G, dev), dev, max(3, a.reps // 2))
        chain = sum(res[k]["median_s"] for k in ("chain_augment", "chain_mfcc", "chain_extractor_fwd_bwd"))
        res["frames"] = int(sum(lengths))
        res["speeds_share_of_augment_mfcc_fwd_bwd"] = res["speeds"]["median_s"] / chain
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    with torch.no_grad():
        sys.exit(main())
