#!/usr/bin/env python3
"""Resample or speed-perturb the 16-bit wave files of a Kaldi wav.scp on the HIP device (neuralplda_amd.resample).

    python tools/resample_wav_scp.py data/train/wav.scp out_dir --rate 16000
    python tools/resample_wav_scp.py data/train/wav.scp out_dir --speeds 0.9,1.0,1.1 --utt2spk data/train/utt2spk

--rate R writes every utterance at R samples per second under its own key.  --speeds writes one copy per factor f, f times as
fast at the file's own rate (resampled from round(f rate) to rate: 1 / f as long, shifted in pitch — sox's `speed`), named
as utils/perturb_data_dir_speed.sh names them: utterance `sp<f>-<utt>`, and with --utt2spk speaker `sp<f>-<spk>` in the
utt2spk and spk2utt written next to the new wav.scp (the copies count as new speakers; the factor 1.0 gets its prefix too,
as a run of that script with factor 1.0 gives it).  The wave files go to out_dir/<new key>.wav; wav.scp, utt2spk and spk2utt
are sorted by key.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def speed_prefix(factor):
    """'sp0.9-' for '0.9' (the factor as it was written on the command line)."""
    return f"sp{factor}-"


def plan_copies(keys, speeds=None, utt2spk=None):
    """[(new key, source key, factor string or None)] sorted by new key, and the new utt2spk dict (None without one)."""
    if speeds is None:
        copies = [(k, k, None) for k in keys]
        new_u2s = None if utt2spk is None else {k: utt2spk[k] for k in keys}
    else:
        copies = [(speed_prefix(f) + k, k, f) for f in speeds for k in keys]
        new_u2s = None if utt2spk is None else {speed_prefix(f) + k: speed_prefix(f) + utt2spk[k] for f in speeds for k in keys}
    if len({c[0] for c in copies}) != len(copies):
        raise ValueError("the new utterance keys are not distinct (a repeated key or speed factor)")
    return sorted(copies), new_u2s


def spk2utt_of(utt2spk):
    out = {}
    for utt in sorted(utt2spk):
        out.setdefault(utt2spk[utt], []).append(utt)
    return out


def read_utt2spk(path):
    out = {}
    with open(path) as fh:
        for line in fh:
            parts = line.split()
            if len(parts) != 2:
                raise ValueError(f"{path}: expected `utterance speaker` per line, got {line!r}")
            out[parts[0]] = parts[1]
    return out


def write_tables(out_dir, copies, new_u2s):
    with open(os.path.join(out_dir, "wav.scp"), "w") as fh:
        for new, _, _ in copies:
            fh.write(f"{new} {os.path.join(out_dir, new + '.wav')}\n")
    if new_u2s is not None:
        with open(os.path.join(out_dir, "utt2spk"), "w") as fh:
            for utt in sorted(new_u2s):
                fh.write(f"{utt} {new_u2s[utt]}\n")
        with open(os.path.join(out_dir, "spk2utt"), "w") as fh:
            for spk, utts in sorted(spk2utt_of(new_u2s).items()):
                fh.write(f"{spk} {' '.join(utts)}\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("wav_scp")
    ap.add_argument("out_dir")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--rate", type=int, help="the new sample rate")
    what.add_argument("--speeds", help="comma-separated speed factors, e.g. 0.9,1.0,1.1")
    ap.add_argument("--utt2spk", help="with --speeds: the utt2spk of the wav.scp")
    ap.add_argument("--utts-per-call", type=int, default=256)
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)

    import numpy as np
    from neuralplda_amd import kaldi_format as kf, resample as rs

    speeds = [s.strip() for s in args.speeds.split(",")] if args.speeds else None
    if speeds is not None and (not speeds or any(not float(s) > 0 for s in speeds)):
        ap.error("--speeds: positive factors")
    if args.utt2spk and speeds is None:
        ap.error("--utt2spk goes with --speeds")
    entries = kf.read_scp(args.wav_scp)
    rx = dict(entries)
    u2s = read_utt2spk(args.utt2spk) if args.utt2spk else None
    if u2s is not None and any(k not in u2s for k in rx):
        ap.error("--utt2spk: an utterance of the wav.scp has no speaker")
    copies, new_u2s = plan_copies([k for k, _ in entries], speeds, u2s)
    os.makedirs(args.out_dir, exist_ok=True)
    clipped_total = 0
    for lo in range(0, len(copies), max(1, args.utts_per_call)):
        piece = copies[lo:lo + max(1, args.utts_per_call)]
        _, offsets, samples, rates = kf.load_wav_scp(args.wav_scp, entries=[(src, rx[src]) for _, src, _ in piece],
                                                     return_rates=True)
        if speeds is None:
            rate_out = np.full(len(piece), args.rate, dtype=np.int64)
            rate_in = rates
        else:
            rate_out = rates
            rate_in = np.array([int(rs.speed_rates(float(f), int(r))) for (_, _, f), r in zip(piece, rates)], dtype=np.int64)
        out, ooff, clipped = rs.resample(samples, offsets, rate_in, rate_out, device=args.device)
        out = out.cpu().numpy()
        clipped_total += int(clipped.sum())
        for u, (new, _, _) in enumerate(piece):
            kf.write_wav(os.path.join(args.out_dir, new + ".wav"), out[ooff[u]:ooff[u + 1]], int(rate_out[u]))
    write_tables(args.out_dir, copies, new_u2s)
    print(f"{len(copies)} wave files in {args.out_dir} ({clipped_total} samples saturated)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
