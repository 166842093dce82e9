#!/usr/bin/env python3
"""Cost of the augmentation (csrc/nplda_augment.hip) next to the stages it feeds.

    python tools/bench_augment.py [--utts 2000] [--seconds 3] [--taps 8000] [--reps 7] [--json OUT] [--profile-only]

--utts utterances of --seconds of 16 kHz audio (noise, three sinusoids and a recording offset), 8 impulse responses of --taps
taps, 8 noise items of 5 s:

  (a) reverb:  one augment call, every utterance reverberated, int16 out (prepared once, launch() timed)    device events
  (b) fft:     the same convolution composed of torch.fft.rfft / irfft on the same GPU (float in, float out,
               one transform of the next power of two per utterance; no powers, no gain, no rounding)         device events
  (c) noise:   one augment call, no RIR, one repeated noise item per utterance, against the HBM bound of its
               bytes (12 per sample: the input three times, the noise twice, the output once) at 4 TB/s       device events
  (d) chain:   compute_mfcc on (a)'s output, and the extractor's forward + backward on those frames           device events

Every figure is the median of --reps runs after one warm-up, with the minimum and maximum next to it.  The transform
kernels' FLOP: 2 x 512 x 512 per block of 256 samples for the spectra, 2 x 256 x 512 for each of the two syntheses.  Nothing
is gated.  --profile-only runs (a) and (c) twice each, for `rocprofv3 --kernel-trace --stats -- python
tools/bench_augment.py --profile-only`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_features import dev_timed  # noqa: E402
from tools.bench_mfcc import synth_audio  # noqa: E402

PEAK_FP32_MFMA, HBM = 157.3e12, 4.0e12


def synth_rirs(count, taps, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(count):
        peak = 40 + 10 * r
        h = 0.3 * rng.standard_normal(taps) * np.exp(-np.maximum(np.arange(taps) - peak, 0) / (0.2 * taps))
        h[:peak] *= 0.1
        h = np.clip(h, -0.9, 0.9)
        h[peak] = 1.0
        out.append(h.astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--taps", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    from neuralplda_amd import augment as ag, mfcc
    dev = torch.device("cuda:0")
    n, U, L = int(a.seconds * 16000), a.utts, a.taps
    samples, offsets = synth_audio(U, n)
    d_samples = torch.from_numpy(samples).to(dev)
    hs = synth_rirs(8, L)
    rirs = ag.RirTable(hs, 16000)
    noises = ag.NoiseTable([synth_audio(1, 5 * 16000, seed=10 + i)[0] for i in range(8)], 16000)
    rir_of = np.arange(U) % 8
    reverb = ag.prepare(d_samples, offsets, ag.Recipe(rir_of), rirs, device=dev)
    noise = ag.prepare(d_samples, offsets, ag.Recipe(np.full(U, -1), [[(u % 8, 0, 10.0, True)] for u in range(U)]), None, noises,
                       device=dev)
    if a.profile_only:
        for _ in range(2):
            reverb.launch()
            noise.launch()
        torch.cuda.synchronize(dev)
        return 0
    blocks = U * (-(-(n + L - 1) // ag.BLOCK))
    res = {"gpu": torch.cuda.get_device_name(dev), "utts": U, "seconds_per_utt": a.seconds, "taps": L, "samples": U * n,
           "blocks": blocks, "workspace_bytes": reverb.workspace_bytes, "calls": len(reverb.calls),
           "command": " ".join(["python", "tools/bench_augment.py"] + sys.argv[1:])}
    res["a_reverb_call"] = dev_timed(reverb.launch, dev, a.reps)
    t = res["a_reverb_call"]["median_s"]
    res["a_reverb_call"]["times_real_time"] = U * a.seconds / t
    res["a_reverb_call"]["mfma_flop"] = blocks * (2 * 512 * 512 + 2 * 2 * 256 * 512)
    res["a_reverb_call"]["mfma_flop_over_call_time_fraction_of_peak"] = res["a_reverb_call"]["mfma_flop"] / t / PEAK_FP32_MFMA

    nfft = 1 << int(np.ceil(np.log2(n + L - 1)))
    peaks = torch.from_numpy(rirs.peaks[rir_of]).to(dev)
    X = d_samples.view(U, n).float()
    H = torch.fft.rfft(torch.from_numpy(np.stack(hs)).to(dev), nfft)[torch.from_numpy(rir_of).to(dev)]
    idx = peaks[:, None] + torch.arange(n, device=dev)[None, :]
    holder = {}

    def fft_conv():
        holder["y"] = torch.gather(torch.fft.irfft(torch.fft.rfft(X, nfft) * H, nfft), 1, idx)
    res["b_torch_fft"] = dev_timed(fft_conv, dev, a.reps)
    res["b_torch_fft"]["nfft"] = nfft
    res["a_over_b"] = t / res["b_torch_fft"]["median_s"]
    # the two compute the same thing: (a) without its gain, to float
    chk = ag.augment(d_samples[:8 * n], offsets[:9], ag.Recipe(rir_of[:8], normalize_output=False), rirs,
                     out_dtype=torch.float32, device=dev)[0].view(8, n)
    res["max_abs_difference_of_a_and_b_over_rms"] = float((chk - holder["y"][:8]).abs().max() / holder["y"][:8].square().mean().sqrt())
    del holder["y"], X, H, idx

    res["c_noise_call"] = dev_timed(noise.launch, dev, a.reps)
    tn = res["c_noise_call"]["median_s"]
    res["c_noise_call"]["bytes"] = 12 * U * n
    res["c_noise_call"]["hbm_bound_s"] = 12 * U * n / HBM
    res["c_noise_call"]["fraction_of_hbm_bound"] = 12 * U * n / HBM / tn

    o = mfcc.MfccOptions(sample_frequency=16000, num_mel_bins=30, num_ceps=30, low_freq=20, high_freq=7600, snip_edges=False)
    out, ooff, _ = reverb.launch()
    holder = {}

    def k_mfcc():
        holder["f"] = mfcc.compute_mfcc(out, ooff, o)
    res["d_mfcc"] = dev_timed(k_mfcc, dev, a.reps)
    frames, lengths = holder["f"]
    from tools.bench_xvec_train import make, run_hip
    with torch.enable_grad():
        m = make(dev)
        G = [torch.randn(U, 512, device=dev)]
        res["d_extractor_fwd_bwd"] = dev_timed(lambda: run_hip(m, [(frames, lengths)], G, dev), dev, max(3, a.reps // 2))
    chain = res["d_mfcc"]["median_s"] + res["d_extractor_fwd_bwd"]["median_s"]
    res["frames"] = int(sum(lengths))
    res["a_share_of_mfcc_plus_fwd_bwd"] = t / chain
    res["expected_share_by_flop"] = "0.02 - 0.03"
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    with torch.no_grad():
        sys.exit(main())
