#!/usr/bin/env python3
"""Cost of the feature front end (Kaldi feature archive -> the extractor's input) next to the extraction it feeds.

    python tools/bench_features.py [--utts 10000] [--frames 400] [--reps 7] [--json OUT]

A synthetic CM-compressed archive of --utts utterances of --frames frames (c0 in speech / silence runs, about three
quarters voiced) is written to a temporary directory, then timed:

  (a) host:   kaldi_format.load_feature_scp (memory-map, headers, descriptor table, ONE payload buffer)   wall clock
  (b) copy:   the payload, descriptors and offsets to the device                                          device events
  (c) front:  the three kernels — decode, energy VAD, sliding CMN + select (with its count and scan)       device events
  (d) xvec:   XVectorNet_ETDNN_12Layer.extract_ragged on the rows (c) produced                            device events
  (e) numpy:  the same front end as per-utterance NumPy (decode, VAD, window means, select) on 16 threads  wall clock

Every device figure is the median of --reps runs after one warm-up, with the minimum and maximum next to it.  The one
figure with a bound is (c) / (d) <= 0.05 in the same run (exit status 1 otherwise); the rest is recorded."""
import argparse
import concurrent.futures
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import feat_ref  # noqa: E402
from tools.bench_xvec import make_model  # noqa: E402


def synth_archive(tmp, utts, frames, distinct=200, seed=0):
    """`utts` CM entries built from `distinct` encoded matrices (encoding is per-column Python: not what is measured)."""
    rng = np.random.default_rng(seed)
    objs = []
    for _ in range(min(distinct, utts)):
        x = rng.standard_normal((frames, 30)) * np.linspace(3.0, 0.3, 30)
        c0 = np.empty(frames)
        t, speech = 0, bool(rng.integers(2))
        while t < frames:
            n = int(rng.integers(20, 120)) if speech else int(rng.integers(5, 40))
            c0[t:t + n] = rng.normal(13.0 if speech else 2.0, 1.0, min(n, frames - t))
            t, speech = t + n, not speech
        x[:, 0] = c0
        objs.append(b"\0B" + feat_ref.encode(x, "CM"))
    ark, scp = os.path.join(tmp, "feats.ark"), os.path.join(tmp, "feats.scp")
    pos = 0
    with open(ark, "wb") as fa, open(scp, "w") as fs:
        for u in range(utts):
            kb = f"utt{u:06d} ".encode()
            fs.write(f"utt{u:06d} {ark}:{pos + len(kb)}\n")
            fa.write(kb + objs[u % len(objs)])
            pos += len(kb) + len(objs[u % len(objs)])
    return scp


def stats(v):
    v = sorted(v)
    return {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "runs": len(v)}


def dev_timed(fn, dev, reps):
    fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) / 1e3)
    return stats(out)


def numpy_front_end(feats, threads, W=300, min_frames=25):
    """Per-utterance NumPy on a thread pool: what a user of the extractor had to write before this front end."""
    from neuralplda_amd import kaldi_format as kf
    keys, desc, payload = feats

    def one(i):
        d = desc[i]
        T, D = int(d["rows"]), int(d["cols"])
        body = payload[int(d["hdr_off"]):int(d["data_off"]) + T * D].tobytes()
        x = kf._decode_compressed("CM", d["min_value"], d["range"], T, D, body)
        keep = feat_ref.vad_energy(x[:, 0])
        if keep.sum() < min_frames:
            return None
        t = np.arange(T)
        s = t - W // 2
        e = s + W
        sh = np.minimum(s, 0)
        s, e = s - sh, e - sh
        sh = np.maximum(e - T, 0)
        s, e = np.maximum(s - sh, 0), e - sh
        P = np.concatenate([np.zeros((1, D)), np.cumsum(x, axis=0)])
        return (x - (P[e] - P[s]) / (e - s)[:, None])[keep].astype(np.float32)

    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        rows = [r for r in ex.map(one, range(len(keys))) if r is not None]
    out = np.concatenate(rows)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from neuralplda_amd import _lib, features, kaldi_format as kf
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"gpu": torch.cuda.get_device_name(dev), "utts": a.utts, "frames_per_utt": a.frames,
           "command": " ".join(["python", "tools/bench_features.py"] + sys.argv[1:])}
    with tempfile.TemporaryDirectory() as tmp:
        scp = synth_archive(tmp, a.utts, a.frames)
        kf.load_feature_scp(scp)  # page cache warm: (a) measures the reader, not the disk
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            feats = kf.load_feature_scp(scp, cols=30)
            host.append(time.perf_counter() - t0)
    res["a_host_read"] = stats(host)
    keys, desc, payload = feats
    res["payload_bytes"] = int(payload.shape[0])
    U = len(keys)
    lengths = [int(r) for r in desc["rows"]]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    R = int(starts[-1])
    res["frames"] = R
    desc8 = np.ascontiguousarray(desc).view(np.uint8)
    holder = {}

    def copy():
        holder["p"] = torch.from_numpy(payload).to(dev)
        holder["d"] = torch.from_numpy(desc8).to(dev)
        holder["o"] = torch.from_numpy(starts).to(dev)
    res["b_h2d_copy"] = dev_timed(copy, dev, a.reps)
    res["b_h2d_copy"]["GB_per_s"] = payload.shape[0] / res["b_h2d_copy"]["median_s"] / 1e9
    p, d, o = holder["p"], holder["d"], holder["o"]
    frames = torch.empty((R, 30), dtype=torch.float32, device=dev)
    mask = torch.empty(R, dtype=torch.uint8, device=dev)
    out = torch.empty((R, 30), dtype=torch.float32, device=dev)
    counts = torch.empty(U, dtype=torch.int32, device=dev)
    ws_n = lib.nplda_feat_workspace_bytes(R, U)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    st = _lib.current_stream(dev)
    vo = features.VadOptions()

    def k_decode():
        _lib.check(lib.nplda_feat_decode_f32(p.data_ptr(), payload.shape[0], d.data_ptr(), o.data_ptr(), U, R,
                                             frames.data_ptr(), st), "decode")

    def k_vad():
        _lib.check(lib.nplda_feat_vad_energy_f32(frames.data_ptr(), o.data_ptr(), U, R, vo.energy_threshold,
                                                 vo.energy_mean_scale, vo.proportion_threshold, vo.frames_context,
                                                 mask.data_ptr(), st), "vad")

    def k_cmn():
        _lib.check(lib.nplda_feat_cmn_select_f32(frames.data_ptr(), o.data_ptr(), U, R, mask.data_ptr(), 300, 25,
                                                 out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_n, st), "cmn_select")

    def front():
        k_decode()
        k_vad()
        k_cmn()
    res["c_front_end"] = dev_timed(front, dev, a.reps)
    res["c_decode"] = dev_timed(k_decode, dev, a.reps)
    res["c_vad"] = dev_timed(k_vad, dev, a.reps)
    res["c_cmn_select"] = dev_timed(k_cmn, dev, a.reps)
    cnt = counts.cpu().numpy()
    kept = cnt[cnt >= 25]
    rows = out[:int(kept.sum())]
    res["voiced_frames"] = int(kept.sum())
    res["kept_utts"] = int(kept.shape[0])
    m = make_model(dev)
    klen = [int(c) for c in kept]
    res["d_extract_ragged"] = dev_timed(lambda: m.extract_ragged(rows, klen), dev, max(3, a.reps // 2))
    t_np, ref = numpy_front_end(feats, a.threads)
    res["e_numpy_front_end"] = {"s": t_np, "threads": a.threads}
    got = rows.cpu().numpy()
    res["max_abs_diff_vs_numpy"] = float(np.abs(got - ref).max()) if got.shape == ref.shape else None
    c, dd = res["c_front_end"]["median_s"], res["d_extract_ragged"]["median_s"]
    res["c_over_d"] = c / dd
    res["gate_c_at_most_5_percent_of_d"] = bool(c <= 0.05 * dd)
    res["a_plus_b_over_d"] = (res["a_host_read"]["median_s"] + res["b_h2d_copy"]["median_s"]) / dd
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["gate_c_at_most_5_percent_of_d"] and res["max_abs_diff_vs_numpy"] is not None else 1


if __name__ == "__main__":
    with torch.no_grad():
        sys.exit(main())
