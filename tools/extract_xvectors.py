#!/usr/bin/env python3
"""x-vectors of a Kaldi data directory's features: the `nnet3-xvector-compute` step of the recipe, on one MI355X.

    python tools/extract_xvectors.py data/test/feats.scp --vad-scp data/test/vad.scp --model model.pt \\
        --out-ark xvector.ark --out-scp xvector.scp
    python tools/extract_xvectors.py data/test/feats.scp --vad-conf conf/vad.conf --model etdnn_weights.pkl ...
    python tools/extract_xvectors.py --wav-scp data/test/wav.scp --mfcc-config conf/mfcc.conf --model model.pt ...

feats.scp may point at FM, DM, CM, CM2 or CM3 matrices (make_mfcc.sh writes CM).  The frames are decoded, normalised
(sliding mean, --cmn-window) and selected (--vad-scp: given decisions; --vad-conf: energy VAD with that file's options;
neither: energy VAD with the recipe's defaults; --no-vad: every frame) on the device, and the x-vectors are written as a
binary vector archive that kaldi_format.load_vector_scp and the score generators read.  Utterances with fewer than
--min-frames voiced frames are listed on stderr and left out.

--wav-scp (instead of feats.scp): 16-bit PCM wave files; their MFCCs are computed on the device first (compute-mfcc-feats
with --dither=0 and the options of --mfcc-config, which must give 30 cepstra; default 16 kHz, 30 bins, 20 - 7600 Hz).

--model: a pickled / torch.save'd XVectorNet_ETDNN_12Layer or Etdnn_Xvec_NeuralPlda, a state dict of either, or the
recipe's pickle of Kaldi weights ({'tdnn1.affine': {'params': ...}, ...}, what LoadFromKaldi reads)."""
import argparse
import os
import pickle
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_extractor(path, pooling, dev):
    from neuralplda_amd import xvector
    try:
        obj = torch.load(path, map_location="cpu", weights_only=False)
    except Exception:
        with open(path, "rb") as fh:
            obj = pickle.load(fh)
    if isinstance(obj, torch.nn.Module):
        m = getattr(obj, "xvector_extractor", obj)
        if not isinstance(m, xvector.XVectorNet_ETDNN_12Layer):
            raise SystemExit(f"{path}: a {type(obj).__name__} holds no E-TDNN extractor")
    elif isinstance(obj, dict):
        m = xvector.XVectorNet_ETDNN_12Layer(pooling_function=torch.var if pooling == "var" else torch.std)
        if "tdnn1.affine" in obj:
            m.LoadFromKaldi(path)
        else:
            pre = "xvector_extractor."
            sd = {k[len(pre):]: v for k, v in obj.items() if k.startswith(pre)} or obj
            own = m.state_dict()
            # a checkpoint's classifier layer (finlin) has the training set's number of classes; extraction does not read it
            m.load_state_dict({k: v for k, v in sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}, strict=False)
            missing = [k for k in own if k.startswith(("tdnn", "lin11")) and k not in sd]
            if missing:
                raise SystemExit(f"{path}: state dict lacks {missing[:3]} ...")
    else:
        raise SystemExit(f"{path}: expected a module, a state dict or a Kaldi weight pickle, got {type(obj).__name__}")
    return m.to(dev).eval().requires_grad_(False)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("feats_scp", nargs="?", default=None)
    ap.add_argument("--feats-scp", dest="feats_scp_opt", default=None, help="the same as the positional argument")
    ap.add_argument("--wav-scp", default=None, help="16-bit PCM wave files instead of features")
    ap.add_argument("--mfcc-config", default=None, help="a Kaldi mfcc.conf for --wav-scp")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--vad-scp", help="given 0/1 decisions per frame (compute-vad-energy's output)")
    g.add_argument("--vad-conf", help="energy VAD on the device with the --vad-* options of this file")
    g.add_argument("--no-vad", action="store_true", help="keep every frame")
    ap.add_argument("--model", required=True)
    ap.add_argument("--pooling", choices=("std", "var"), default="std", help="for state dicts and Kaldi weight pickles")
    ap.add_argument("--out-ark", required=True)
    ap.add_argument("--out-scp", default=None)
    ap.add_argument("--cmn-window", type=int, default=300)
    ap.add_argument("--min-frames", type=int, default=25)
    ap.add_argument("--utts-per-call", type=int, default=2048)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    feats_scp = a.feats_scp or a.feats_scp_opt
    if (feats_scp is None) == (a.wav_scp is None) or (a.feats_scp and a.feats_scp_opt):
        ap.error("give one of feats.scp (positional or --feats-scp) and --wav-scp")
    if a.wav_scp is None and a.mfcc_config:
        ap.error("--mfcc-config goes with --wav-scp")
    if a.wav_scp is not None and a.vad_scp:
        ap.error("--vad-scp goes with a feats.scp (its decisions belong to those frames)")
    from neuralplda_amd import features, kaldi_format
    dev = torch.device(a.device)
    m = load_extractor(a.model, a.pooling, dev)
    if a.no_vad:
        vad = None
    elif a.vad_scp:
        vad = a.vad_scp
    else:
        vad = features.VadOptions.from_conf(a.vad_conf) if a.vad_conf else features.VadOptions()
    if a.wav_scp is not None:
        from neuralplda_amd import mfcc
        keys, xv, dropped = m.extract_from_wav_scp(a.wav_scp, mfcc=mfcc.MfccOptions.from_conf(a.mfcc_config) if a.mfcc_config
                                                   else None, vad=vad, cmn_window=a.cmn_window, min_frames=a.min_frames,
                                                   utts_per_call=min(a.utts_per_call, 256), device=dev)
    else:
        keys, xv, dropped = m.extract_from_scp(feats_scp, vad=vad, cmn_window=a.cmn_window, min_frames=a.min_frames,
                                               utts_per_call=a.utts_per_call, device=dev)
    kaldi_format.write_vector_ark(a.out_ark, keys, xv.cpu().numpy(), a.out_scp)
    for k, n in dropped:
        print(f"dropped {k}: {n} voiced frames (fewer than {a.min_frames})", file=sys.stderr)
    print(f"wrote {len(keys)} x-vectors to {a.out_ark}; dropped {len(dropped)} utterances", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
