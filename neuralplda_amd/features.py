"""From a Kaldi feature archive to the E-TDNN extractor's input, on the HIP device (csrc/nplda_feat.hip).

The x-vector recipe feeds the network `apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 |
select-voiced-frames` over `feats.scp` and `vad.scp`; `vad.scp` comes from `compute-vad-energy` with the four options of
`vad.conf`.  Here the matrix bodies go to the device as they lie in the archive (`kaldi_format.load_feature_scp`: one byte
per value for a `CM` matrix) and three kernels decode them, take the VAD decisions (or use given ones), normalise and
select:

    feats = kaldi_format.load_feature_scp("data/train/feats.scp")
    prep = prepare_features(feats, vad=VadOptions.from_conf("conf/vad.conf"))
    xvec = extractor.extract_ragged(prep.frames, prep.lengths)

`XVectorNet_ETDNN_12Layer.extract_from_scp` does this in bounded pieces.  design/k13_feature_frontend.md.
"""
import collections
import os

import numpy as np
import torch

from . import _lib, kaldi_format

__all__ = ["VadOptions", "PreparedFeatures", "prepare_features", "prepare_frames", "decode_features", "energy_vad", "cmn_select", "FEAT_DIM"]

FEAT_DIM = 30  # include/nplda_hip.h NPLDA_FEAT_DIM


class VadOptions(collections.namedtuple("VadOptions", "energy_threshold energy_mean_scale proportion_threshold "
                                                      "frames_context")):
    """compute-vad-energy's options (--vad-energy-threshold, --vad-energy-mean-scale, --vad-proportion-threshold,
    --vad-frames-context); the defaults are the values of the recipe's vad.conf."""
    __slots__ = ()
    _FLAGS = {"vad-energy-threshold": ("energy_threshold", float), "vad-energy-mean-scale": ("energy_mean_scale", float),
              "vad-proportion-threshold": ("proportion_threshold", float), "vad-frames-context": ("frames_context", int)}

    def __new__(cls, energy_threshold=5.5, energy_mean_scale=0.5, proportion_threshold=0.12, frames_context=2):
        if int(frames_context) < 0 or not 0.0 < float(proportion_threshold) < 1.0 or float(energy_mean_scale) < 0.0:
            raise ValueError("VadOptions: frames_context >= 0, 0 < proportion_threshold < 1, energy_mean_scale >= 0")
        return super(VadOptions, cls).__new__(cls, float(energy_threshold), float(energy_mean_scale),
                                              float(proportion_threshold), int(frames_context))

    @classmethod
    def from_conf(cls, path):
        """A Kaldi option file: one `--name=value` per line, `#` comments.  Options other than the four are an error."""
        kw = {}
        with open(path, "r") as fh:
            for n, ln in enumerate(fh, 1):
                ln = ln.split("#", 1)[0].strip()
                if not ln:
                    continue
                name, sep, val = ln.partition("=")
                name = name.strip().lstrip("-")
                if not sep or name not in cls._FLAGS:
                    raise ValueError(f"{path}:{n}: not a VAD option: {ln!r}")
                field, conv = cls._FLAGS[name]
                kw[field] = conv(val.strip())
        return cls(**kw)


PreparedFeatures = collections.namedtuple("PreparedFeatures", "frames lengths keys dropped")
PreparedFeatures.__doc__ = """frames: (sum lengths, 30) float32 on the device, normalised, voiced frames only, utterance after
utterance; lengths: their frame counts (list of int); keys: their keys; dropped: [(key, voiced frames)] of the utterances
left out because they have fewer than min_frames voiced frames."""


def _vad_mask(vad, keys, rows, starts):
    """Host uint8 mask (total frames) from given decisions: {key: 0/1 vector} or the path of a vad.scp."""
    if isinstance(vad, (str, os.PathLike)):
        want = set(keys)
        vad = {k: v for k, v in kaldi_format.read_vector_scp(vad) if k in want}
    mask = np.zeros(int(starts[-1]), dtype=np.uint8)
    for i, k in enumerate(keys):
        if k not in vad:
            raise KeyError(f"{k}: no VAD decisions for this utterance")
        v = np.asarray(vad[k]).ravel()
        if v.shape[0] != rows[i]:
            raise ValueError(f"{k}: {v.shape[0]} VAD decisions for {rows[i]} frames")
        mask[starts[i]:starts[i + 1]] = v != 0
    return mask


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the feature front end runs on a HIP device, not on {dev}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _offsets(lengths, dev):
    starts = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)
    if len(lengths) and min(lengths) < 0:
        raise ValueError("negative utterance length")
    return starts, torch.from_numpy(starts).to(dev)


def decode_features(feats, device=None):
    """feats: what kaldi_format.load_feature_scp returned -> (frames (sum T_u, 30) float32 on the device, [T_u]).  The
    payload goes to the device as it is (one copy) and one launch decodes every matrix."""
    keys, desc, payload = feats
    U = len(keys)
    if len(desc) != U or desc.dtype != kaldi_format.FEAT_DESC:
        raise ValueError("feats: expected the (keys, desc, payload) of kaldi_format.load_feature_scp")
    dev = _device(device)
    if U == 0:
        return torch.empty((0, FEAT_DIM), dtype=torch.float32, device=dev), []
    bad = np.nonzero(desc["cols"] != FEAT_DIM)[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"{keys[i]}: matrix of {int(desc['cols'][i])} columns, the extractor takes {FEAT_DIM}")
    fmt = desc["format"]
    unknown = (fmt < 0) | (fmt > 4)
    if unknown.any():
        raise ValueError(f"{keys[int(np.argmax(unknown))]}: unknown matrix format code")
    esz = np.array([4, 8, 1, 2, 1], dtype=np.int64)[fmt]
    rows = desc["rows"].astype(np.int64)
    nbytes = int(payload.shape[0])
    off_bad = (rows < 0) | (desc["data_off"] < 0) | (desc["data_off"] % esz != 0) | \
        (desc["data_off"] + rows * FEAT_DIM * esz > nbytes) | \
        ((fmt == 2) & ((desc["hdr_off"] < 0) | (desc["hdr_off"] % 2 != 0) | (desc["hdr_off"] + 8 * FEAT_DIM > nbytes)))
    if off_bad.any():
        raise ValueError(f"{keys[int(np.argmax(off_bad))]}: descriptor does not address a body inside the payload")
    lengths = [int(r) for r in rows]
    starts, d_off = _offsets(lengths, dev)
    R = int(starts[-1])
    lib = _lib.load()
    with _lib.on_device(dev):
        d_payload = torch.from_numpy(np.ascontiguousarray(payload)).to(dev) if nbytes else \
            torch.empty(8, dtype=torch.uint8, device=dev)
        d_desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(dev)
        frames = torch.empty((R, FEAT_DIM), dtype=torch.float32, device=dev)
        _lib.check(lib.nplda_feat_decode_f32(d_payload.data_ptr(), nbytes, d_desc.data_ptr(), d_off.data_ptr(), U, R,
                                             frames.data_ptr(), _lib.current_stream(dev)), "nplda_feat_decode_f32")
    return frames, lengths


def _check_frames(frames, lengths):
    if frames.dim() != 2 or frames.shape[1] != FEAT_DIM or frames.dtype != torch.float32 or not frames.is_cuda \
            or not frames.is_contiguous():
        raise ValueError(f"frames: expected a contiguous float32 (frames, {FEAT_DIM}) tensor on the HIP device")
    if sum(lengths) != frames.shape[0]:
        raise ValueError(f"lengths sum to {sum(lengths)}, frames has {frames.shape[0]} rows")


def energy_vad(frames, lengths, options=VadOptions()):
    """compute-vad-energy on c0 of every utterance -> uint8 (frames,) decisions on the device."""
    lengths = [int(T) for T in lengths]
    _check_frames(frames, lengths)
    dev = frames.device
    mask = torch.empty(frames.shape[0], dtype=torch.uint8, device=dev)
    if frames.shape[0] == 0:
        return mask
    lib = _lib.load()
    with _lib.on_device(dev):
        _, d_off = _offsets(lengths, dev)
        _lib.check(lib.nplda_feat_vad_energy_f32(frames.data_ptr(), d_off.data_ptr(), len(lengths), frames.shape[0],
                                                 options.energy_threshold, options.energy_mean_scale,
                                                 options.proportion_threshold, options.frames_context, mask.data_ptr(),
                                                 _lib.current_stream(dev)), "nplda_feat_vad_energy_f32")
    return mask


def cmn_select(frames, lengths, mask=None, cmn_window=300, min_frames=25):
    """Sliding-window mean subtraction, then the frames with mask != 0 (None: all) of the utterances that keep at least
    min_frames -> (rows (sum kept, 30) float32, counts: numpy int32 kept frames of EVERY utterance).  Reading the counts
    is the one host synchronisation."""
    lengths = [int(T) for T in lengths]
    _check_frames(frames, lengths)
    if int(cmn_window) < 0 or int(min_frames) < 0:
        raise ValueError("cmn_window and min_frames must not be negative")
    dev = frames.device
    U, R = len(lengths), frames.shape[0]
    if U == 0:
        return frames, np.zeros(0, dtype=np.int32)
    if mask is not None and (mask.dtype != torch.uint8 or mask.shape != (R,) or mask.device != dev or not mask.is_contiguous()):
        raise ValueError("mask: expected a contiguous uint8 (frames,) tensor on the frames' device")
    lib = _lib.load()
    with _lib.on_device(dev):
        _, d_off = _offsets(lengths, dev)
        out = torch.empty((R, FEAT_DIM), dtype=torch.float32, device=dev)
        counts = torch.empty(U, dtype=torch.int32, device=dev)
        ws_n = lib.nplda_feat_workspace_bytes(R, U)
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        _lib.check(lib.nplda_feat_cmn_select_f32(frames.data_ptr(), d_off.data_ptr(), U, R, _lib.ptr(mask) if R else None,
                                                 int(cmn_window), int(min_frames), out.data_ptr(), counts.data_ptr(),
                                                 ws.data_ptr(), ws_n, _lib.current_stream(dev)), "nplda_feat_cmn_select_f32")
        cnt = counts.cpu().numpy()
    return out[:int(cnt[cnt >= int(min_frames)].sum())], cnt


def prepare_frames(keys, frames, lengths, vad=VadOptions(), cmn_window=300, min_frames=25):
    """The part of prepare_features after the decode, for frames that are on the device already (mfcc.compute_mfcc):
    keys, frames (sum T_u, 30) and [T_u] -> PreparedFeatures.  vad, cmn_window, min_frames: as prepare_features."""
    keys = list(keys)
    if not keys:
        return PreparedFeatures(frames, [], [], [])
    if vad is None:
        mask = None
    elif isinstance(vad, VadOptions):
        mask = energy_vad(frames, lengths, vad)
    else:
        starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        mask = torch.from_numpy(_vad_mask(vad, keys, lengths, starts)).to(frames.device)
    out, cnt = cmn_select(frames, lengths, mask, cmn_window, min_frames)
    keep = cnt >= int(min_frames)
    return PreparedFeatures(out, [int(c) for c in cnt[keep]], [k for k, f in zip(keys, keep) if f],
                            [(k, int(c)) for k, c, f in zip(keys, cnt, keep) if not f])


def prepare_features(feats, vad=VadOptions(), cmn_window=300, min_frames=25, device=None):
    """feats: what kaldi_format.load_feature_scp returned.  vad: VadOptions (energy VAD on c0, on the device), a {key: 0/1
    vector} dict or the path of a vad.scp (given decisions), or None (every frame is kept).  cmn_window: frames of the
    centred sliding mean (0: none).  Utterances with fewer than min_frames voiced frames are left out and returned in
    `dropped` with their counts.  One host synchronisation (the voiced counts).  -> PreparedFeatures."""
    frames, lengths = decode_features(feats, device)
    return prepare_frames(feats[0], frames, lengths, vad, cmn_window, min_frames)
