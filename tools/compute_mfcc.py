#!/usr/bin/env python3
"""MFCCs of a Kaldi wav.scp on one MI355X: `compute-mfcc-feats --dither=0`, written as an uncompressed feature archive.

    python tools/compute_mfcc.py data/test/wav.scp --config conf/mfcc.conf --out-ark mfcc.ark --out-scp feats.scp

wav.scp names 16-bit PCM wave files (command pipes and `segments` are not read).  The archive holds one `FM` matrix per
utterance, (frames, num_ceps) float32, so that `copy-feats` / `compare-feats` of a Kaldi installation elsewhere can hold
it against compute-mfcc-feats' own output, and kaldi_format.load_feature_scp reads it back."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("wav_scp")
    ap.add_argument("--config", default=None, help="a Kaldi mfcc.conf (default: compute-mfcc-feats' defaults, dither 0)")
    ap.add_argument("--out-ark", required=True)
    ap.add_argument("--out-scp", default=None)
    ap.add_argument("--channel", type=int, default=0)
    ap.add_argument("--utts-per-call", type=int, default=256)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    from neuralplda_amd import kaldi_format, mfcc
    o = mfcc.MfccOptions.from_conf(a.config) if a.config else mfcc.MfccOptions()
    dev = torch.device(a.device)
    entries = kaldi_format.read_scp(a.wav_scp)
    keys, mats = [], []
    for lo in range(0, len(entries), a.utts_per_call):
        k, offsets, samples = kaldi_format.load_wav_scp(a.wav_scp, entries=entries[lo:lo + a.utts_per_call],
                                                        sample_frequency=o.sample_frequency, channel=a.channel)
        frames, lengths = mfcc.compute_mfcc(samples, offsets, o, dev)
        host = frames.cpu().numpy()
        at = np.concatenate([[0], np.cumsum(lengths)])
        keys += k
        mats += [host[at[i]:at[i + 1]] for i in range(len(k))]
    kaldi_format.write_feature_ark(a.out_ark, keys, mats, a.out_scp)
    print(f"wrote {len(keys)} matrices, {sum(len(m) for m in mats)} frames of {o.num_ceps} cepstra, to {a.out_ark}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
