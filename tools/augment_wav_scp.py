#!/usr/bin/env python3
"""Augment the 16-bit wave files of a Kaldi wav.scp on the HIP device: reverberation, noise, music and babble as the Kaldi
voxceleb recipe draws them (neuralplda_amd/augment.py, design/k28_augment.md).

    python tools/augment_wav_scp.py data/train/wav.scp --rir-list rirs.txt --noise-list noises.txt \\
        --kinds reverb,noise,music,babble --seed 0 --out-dir data/train_aug --suffix aug

rirs.txt: one wave file per line.  noises.txt: `<path> <noise|music|babble>` per line (a line without a label serves every
kind).  Writes <out-dir>/<key>-<suffix>.wav for every line of the scp and <out-dir>/wav.scp naming them; prints one JSON
line with the counts.  The draws come from numpy.random.Generator(PCG64(seed)) in scp order: a seed repeats a run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_list(path, labelled=False):
    paths, labels = [], []
    with open(path) as fh:
        for ln in fh:
            f = ln.split("#", 1)[0].split()
            if not f:
                continue
            paths.append(f[0])
            labels.append(f[1] if len(f) > 1 else None)
    if not labelled:
        return paths
    if any(s is None for s in labels):
        if any(s is not None for s in labels):
            raise SystemExit(f"{path}: label every noise item or none")
        labels = None
    return paths, labels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("wav_scp")
    ap.add_argument("--rir-list", default=None)
    ap.add_argument("--noise-list", default=None)
    ap.add_argument("--kinds", default="reverb,noise,music,babble")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--suffix", default="aug")
    ap.add_argument("--sample-frequency", type=int, default=16000)
    ap.add_argument("--utts-per-call", type=int, default=256)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    import torch
    from neuralplda_amd import augment as ag, kaldi_format as kf
    sr = a.sample_frequency
    kinds = tuple(k for k in a.kinds.split(",") if k)
    rirs = ag.RirTable(read_list(a.rir_list), sr) if a.rir_list else None
    noises = None
    if a.noise_list:
        paths, labels = read_list(a.noise_list, labelled=True)
        noises = ag.NoiseTable(paths, sr, labels=labels)
    aug = ag.Augmenter(rirs, noises, kinds=kinds, seed=a.seed)
    os.makedirs(a.out_dir, exist_ok=True)
    entries = kf.read_scp(a.wav_scp)
    dev = torch.device(a.device)
    written = clipped_total = 0
    with open(os.path.join(a.out_dir, "wav.scp"), "w") as scp:
        for lo in range(0, len(entries), a.utts_per_call):
            keys, offsets, samples = kf.load_wav_scp(a.wav_scp, entries=entries[lo:lo + a.utts_per_call], sample_frequency=sr)
            out, ooff, clipped = aug(samples, offsets, device=dev)
            host = out.cpu().numpy()
            clipped_total += int(clipped.sum())
            for u, key in enumerate(keys):
                path = os.path.join(a.out_dir, f"{key}-{a.suffix}.wav")
                kf.write_wav(path, host[ooff[u]:ooff[u + 1]], sr)
                scp.write(f"{key}-{a.suffix} {path}\n")
                written += 1
    print(json.dumps({"utterances": written, "clipped_samples": clipped_total, "kinds": list(kinds), "seed": a.seed,
                      "out_dir": a.out_dir}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
