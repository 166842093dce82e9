#!/usr/bin/env python
"""DER scoring of a threshold sweep (ops.der, csrc/nplda_der.hip) against the host routes, on one GPU.

The shape: --recordings (256) recordings of --frames (60 000) frames, 8 reference speakers with about 10 % of the speech
overlapped, windows of 144 frames every 24 over the speech, and --cuts (32) hypotheses per recording (window labels: the true
speaker with a share of the windows relabelled, 2 .. 33 clusters), so recordings x cuts problems in ONE call:
  items   the labelled-items form (what diarize.sweep_thresholds sends: one label per window and problem);
  turns   the same hypotheses as turn tables (what metrics.der sends).
A few distinct recordings are generated (--distinct) and repeated; every problem is scored in full.
Device events around the whole call (output and workspace allocation included), one warm-up call per form, then --rounds
rounds that alternate the two forms; medians and minima.  The counts of the first problems are checked against the twin.
Host baselines on the same machine, ONE core: the vectorised numpy twin of tests/der_ref.py per problem, and
diarize.turns(windows, labels) per problem (the host half of a sweep that scores through turn tables); both are timed on
--twin-problems problems and scaled to the call (marked "extrapolated").
--trace: one warm-up and ONE call of each form and nothing else, for a kernel trace in a process of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_der.py --trace).  One JSON line per variant and a summary line."""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # before numpy loads its BLAS: the baselines are one host core

import argparse  # noqa: E402
import json  # noqa: E402
import statistics  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_reference(rng, T, S=8, overlap=0.10):
    """Turns of 1 .. 6 s with pauses; about `overlap` of the turns start inside the one before."""
    rows, t = [], int(rng.integers(0, 200))
    while t < T - 100:
        n = int(rng.integers(100, 600))
        rows.append((t, min(t + n, T), int(rng.integers(0, S))))
        t += n + (-int(rng.integers(50, 100 + n // 2)) if rng.random() < 2.2 * overlap else int(rng.integers(0, 150)))
        t = max(t, 0)
    return np.array(rows, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=256)
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--cuts", type=int, default=32)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--collar", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--twin-problems", type=int, default=4)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_der: no HIP device (a time is measured on the GPU or not at all)")
    from neuralplda_amd import diarize, ops
    from tests import der_ref as dr
    dev = torch.device("cuda:0")
    Rn, T, K, nsrc = args.recordings, args.frames, args.cuts, min(args.distinct, args.recordings)
    rng = np.random.default_rng(24)
    big = ops.DER_MAX_FRAMES

    src, t_turns = [], []
    for s in range(nsrc):
        ref = make_reference(rng, T)
        A = dr.activity(ref, 8, T)
        speech = diarize._runs(A.any(axis=0))
        windows, _ = diarize.uniform_windows([speech], 144, 24)
        W = windows.shape[0]
        centre = (windows[:, 2] + windows[:, 3]) // 2
        truth = A[:, centre].argmax(axis=0)
        item = np.full(T, -1, np.int32)
        for _, _, b0, fl in diarize.frame_labels(windows, np.arange(W)):
            item[b0:b0 + fl.size] = fl
        labels, turns = [], []
        for k in range(K):
            lab = np.where(rng.random(W) < 0.02 + 0.01 * k, rng.integers(0, 2 + k, W), truth).astype(np.int64)
            t0 = time.perf_counter()
            tt = diarize.turns(windows, lab)
            t_turns.append(time.perf_counter() - t0)
            labels.append(lab.astype(np.int32))
            turns.append(tt[:, 1:].astype(np.int32))
        src.append(dict(ref=ref, item=item, labels=labels, turns=turns, W=W, overlap=float((A.sum(axis=0) > 1).sum() / max(A.any(axis=0).sum(), 1))))

    P = Rn * K
    prob = ops.der_problems(np.repeat(np.arange(Rn), K), dev)
    fo = ops.RaggedOffsets(np.arange(Rn + 1, dtype=np.int64) * T, dev, max_rows=big)
    refs = [src[r % nsrc]["ref"] for r in range(Rn)]
    ro = ops.RaggedOffsets(np.concatenate([[0], np.cumsum([t.shape[0] for t in refs])]), dev, max_rows=big)
    rt = torch.from_numpy(np.concatenate(refs).astype(np.int32)).to(dev)
    fi = torch.from_numpy(np.concatenate([src[r % nsrc]["item"] for r in range(Rn)])).to(dev)
    labs = [src[r % nsrc]["labels"][k] for r in range(Rn) for k in range(K)]
    io = ops.RaggedOffsets(np.concatenate([[0], np.cumsum([v.size for v in labs])]), dev, max_rows=big)
    il = torch.from_numpy(np.concatenate(labs)).to(dev)
    tabs = [src[r % nsrc]["turns"][k] for r in range(Rn) for k in range(K)]
    ho = ops.RaggedOffsets(np.concatenate([[0], np.cumsum([t.shape[0] for t in tabs])]), dev, max_rows=big)
    ht = torch.from_numpy(np.concatenate(tabs)).to(dev)
    common = dict(collar=args.collar, n_ref_speakers=8, n_hyp_speakers=64)
    forms = {"items": lambda: ops.der(fo, ro, rt, prob, frame_item=fi, item_offsets=io, item_labels=il, **common),
             "turns": lambda: ops.der(fo, ro, rt, prob, hyp_offsets=ho, hyp_turns=ht, **common)}
    shape = {"recordings": Rn, "frames": T, "cuts": K, "problems": P, "ref_turns": int(ro.rows), "windows": int(io.rows),
             "hyp_turns": int(ho.rows), "overlapped_share_of_speech": round(src[0]["overlap"], 3), "collar": args.collar}

    out = {name: [t.cpu().numpy() for t in fn()[:2]] for name, fn in forms.items()}     # (the warm-up calls)
    assert np.array_equal(out["items"][0], out["turns"][0]) and np.array_equal(out["items"][1], out["turns"][1])
    if args.trace:
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, **shape}), flush=True)
        return

    t_twin = []
    for p in range(min(args.twin_problems, P)):
        r, k = divmod(p, K)
        t0 = time.perf_counter()
        want = dr.der_counts_items(src[r % nsrc]["ref"], src[r % nsrc]["item"], src[r % nsrc]["labels"][k], T, 8, 64,
                                   collar=args.collar)
        t_twin.append(time.perf_counter() - t0)
        assert out["items"][0][p].tolist() == [want[n] for n in ops.DER_COUNTS], p

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    ts = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            ts[name].append(timed(fn))
    summary = {}
    for name in forms:
        med = statistics.median(ts[name])
        print(json.dumps({"variant": name, **shape, "rounds": args.rounds, "median_s": med, "min_s": min(ts[name]),
                          "max_s": max(ts[name]), "us_per_problem": med * 1e6 / P, "frames_per_s": P * T / med}), flush=True)
        summary[f"{name}_ms"] = round(med * 1e3, 3)
    for name, per in (("numpy_twin_one_core", statistics.median(t_twin)), ("host_turns_one_core", statistics.median(t_turns))):
        print(json.dumps({"variant": name, "problems_timed": len(t_twin) if "twin" in name else len(t_turns),
                          "median_s_per_problem": per, "call_s": per * P, "extrapolated": True}), flush=True)
        summary[f"{name}_s"] = round(per * P, 2)
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
