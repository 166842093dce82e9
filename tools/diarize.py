#!/usr/bin/env python3
"""Diarize recordings into an RTTM file with sliding-window x-vectors, on one MI355X.

    python tools/diarize.py --feats-scp diar/feats.scp --xvector-model models/etdnn.pt --model models/NPLDA.pt \
        --threshold 0.0 --rttm diar/out.rttm
    python tools/diarize.py --wav-scp diar/wav.scp --segments diar/segments --xvector-model models/etdnn.pt \
        --model models/NPLDA.pt --min-clusters 8 --vb-plda models/plda --rttm diar/out.rttm

--wav-scp (16-bit PCM files; MFCCs are computed on the device) or --feats-scp (30-dimensional MFCC matrices of whole
recordings, not mean-normalised): one entry per recording.
--xvector-model: a pickled / torch.save'd XVectorNet_ETDNN_12Layer (or an Etdnn_Xvec_NeuralPlda, whose extractor is
taken); --model: a pickled NeuralPlda, the score the windows are clustered under.
--segments: a Kaldi `segments` file (`<segment> <recording> <start> <end>`) naming the speech of each recording; a
recording it does not list has no speech.  Without it the energy VAD of the package finds the speech (--min-speech,
--max-gap, in frames).
--window / --shift (frames): the rule of neuralplda_amd.diarize.uniform_windows.
--threshold, --calibration, --min-clusters, --linkage, --vb-plda, --vb-fa, --vb-fb, --vb-loop, --vb-max-iters: the
clustering and the VB-HMM resegmentation, as in tools/cluster_xvectors.py (each recording on its own).
--clusterer spectral [--neighbours 4,6,8,...] [--max-speakers N]: cluster.spectral_cluster in place of the agglomerative
step: no threshold, the speaker count of a recording (between --min-clusters and --max-speakers, default 16) comes from the
eigengap of its affinity graph; the VB-HMM options apply as before.
The scp is worked through --recordings-per-call recordings at a time, so that the features and the workspaces stay
bounded; speaker labels are counted on through the pieces.  Output: one RTTM line per speaker turn.
--ref-rttm: a reference RTTM; the overall diarization error rate of the output against it (collar 0.25 s, overlapped
speech included) is printed after the RTTM is written (tools/score_rttm.py scores with other settings and per recording)."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def load_extractor(path, dev):
    from neuralplda_amd import compat, xvector
    compat.install()
    try:
        obj = torch.load(path, map_location="cpu", weights_only=False)
    except Exception:
        with open(path, "rb") as fh:
            obj = pickle.load(fh)
    if isinstance(obj, xvector.Etdnn_Xvec_NeuralPlda):
        obj = obj.xvector_extractor
    if not isinstance(obj, xvector.XVectorNet_ETDNN_12Layer):
        raise SystemExit(f"{path}: expected a pickled XVectorNet_ETDNN_12Layer, got {type(obj).__name__}")
    return obj.to(dev).eval().requires_grad_(False)


def main(argv=None):
    from identify import load_model
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--wav-scp")
    src.add_argument("--feats-scp")
    ap.add_argument("--xvector-model", required=True)
    ap.add_argument("--model", required=True)
    ap.add_argument("--segments")
    ap.add_argument("--min-speech", type=int, default=50)
    ap.add_argument("--max-gap", type=int, default=30)
    ap.add_argument("--cmn-window", type=int, default=300)
    ap.add_argument("--window", type=int, default=144)
    ap.add_argument("--shift", type=int, default=24)
    ap.add_argument("--frame-shift", type=float, default=0.01, help="seconds per frame (of --segments and the RTTM)")
    ap.add_argument("--threshold", type=float, default=float("-inf"))
    ap.add_argument("--calibration", type=float, nargs=2, metavar=("A", "B"),
                    help="--threshold is in units of llr = A s + B (A > 0): it is mapped to (threshold - B) / A")
    ap.add_argument("--min-clusters", type=int, default=1)
    ap.add_argument("--linkage", default="average", choices=["average", "complete", "single"])
    ap.add_argument("--clusterer", default="ahc", choices=["ahc", "spectral"],
                    help="spectral: the neighbour count of the affinity graph is tuned per recording by the normalised maximum "
                         "eigengap and the speaker count read from it; --threshold, --calibration and --linkage are not used")
    ap.add_argument("--neighbours", help="--clusterer spectral: comma-separated candidate neighbour counts, strictly increasing")
    ap.add_argument("--max-speakers", type=int, default=16, help="--clusterer spectral: the most speakers per recording")
    ap.add_argument("--vb-plda", help="a Kaldi PLDA model: refine the clusters by VB-HMM resegmentation under its psi")
    ap.add_argument("--vb-fa", type=float, default=0.3)
    ap.add_argument("--vb-fb", type=float, default=17.0)
    ap.add_argument("--vb-loop", type=float, default=0.99)
    ap.add_argument("--vb-max-iters", type=int, default=40)
    ap.add_argument("--recordings-per-call", type=int, default=16)
    ap.add_argument("--rttm", required=True)
    ap.add_argument("--ref-rttm", help="a reference RTTM: print the overall DER of the output (tools/score_rttm.py has the rest)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("diarize: no HIP device (the extraction and the clustering have no CPU path)")
    if args.recordings_per_call < 1:
        raise SystemExit("diarize: --recordings-per-call must be positive")
    thr = args.threshold
    if args.calibration is not None:
        a, b = args.calibration
        if not a > 0:
            raise SystemExit("diarize: a calibration slope must be positive")
        thr = (thr - b) / a
    from neuralplda_amd import diarize, features, kaldi_format
    dev = torch.device(args.device)
    extractor, model = load_extractor(args.xvector_model, dev), load_model(args.model, dev)
    psi = kaldi_format.read_plda(args.vb_plda)["Psi_across_covar_diag"] if args.vb_plda else None
    vb = dict(Fa=args.vb_fa, Fb=args.vb_fb, loop_prob=args.vb_loop, max_iters=args.vb_max_iters)
    spectral = None
    if args.clusterer == "spectral":
        spectral = dict(neighbours=[int(v) for v in args.neighbours.split(",")] if args.neighbours else None,
                        min_clusters=args.min_clusters, max_clusters=args.max_speakers)
    given = None
    if args.segments:
        recs, segs = diarize.read_segments(args.segments, args.frame_shift)
        given = dict(zip(recs, segs))
    scp = args.wav_scp or args.feats_scp
    entries = kaldi_format.read_scp(scp)
    mfcc_opts = None
    if args.wav_scp:
        from neuralplda_amd import mfcc
        mfcc_opts = mfcc.MfccOptions(sample_frequency=16000, num_mel_bins=30, num_ceps=30, low_freq=20, high_freq=7600,
                                     snip_edges=False)
    reco_ids, turns, base, n_windows = [], [], 0, 0
    for lo in range(0, len(entries), args.recordings_per_call):
        piece = entries[lo:lo + args.recordings_per_call]
        if args.wav_scp:
            keys, offsets, samples = kaldi_format.load_wav_scp(scp, entries=piece, sample_frequency=mfcc_opts.sample_frequency)
            frames, lengths = mfcc.compute_mfcc(samples, offsets, mfcc_opts, dev)
        else:
            feats = kaldi_format.load_feature_scp(scp, entries=piece, cols=30)
            keys = list(feats[0])
            frames, lengths = features.decode_features(feats, dev)
        segments = None
        if given is not None:  # clipped to the recording: a segments file may run a frame past the features
            segments = [np.minimum(given.get(k, np.zeros((0, 2), np.int64)), T) for k, T in zip(keys, lengths)]
        res = diarize.diarize(model, extractor, frames, lengths, keys, segments=segments, min_speech=args.min_speech,
                              max_gap=args.max_gap, cmn_window=args.cmn_window, window=args.window, shift=args.shift,
                              threshold=thr, min_clusters=args.min_clusters, linkage=args.linkage, vb_psi=psi, vb=vb,
                              clusterer=args.clusterer, spectral=spectral)
        for r, s, n in res.dropped:
            print(f"diarize: {keys[r]}: a segment of {n} frames is too short for a window", file=sys.stderr)
        t = res.turns.copy()
        t[:, 0] += len(reco_ids)
        t[:, 3] += base
        turns.append(t)
        reco_ids += keys
        n_windows += res.windows.shape[0]
        base += int(res.labels.max()) + 1 if res.labels.size else 0
    turns = np.concatenate(turns) if turns else np.zeros((0, 4), np.int64)
    diarize.write_rttm(args.rttm, reco_ids, turns, args.frame_shift)
    print(f"{len(reco_ids)} recordings, {n_windows} windows -> {turns.shape[0]} turns of {base} speakers in {args.rttm}",
          file=sys.stderr)
    if args.ref_rttm:
        from neuralplda_amd import metrics
        print(metrics.der(args.ref_rttm, args.rttm, frame_shift=args.frame_shift).lines()[-1])


if __name__ == "__main__":
    main()
