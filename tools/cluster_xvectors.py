#!/usr/bin/env python3
"""Cluster unlabelled x-vectors under a NeuralPlda model's own score into pseudo-speakers, on one MI355X.

    python tools/cluster_xvectors.py --model models/NPLDA.pt --xvectors dev/xvector.scp --threshold 0.0 --out-dir dev/clusters
    python tools/cluster_xvectors.py --model models/NPLDA.pt --xvectors diar/xvector.scp --reco2utt diar/reco2utt \
        --min-clusters 2 --out-dir diar/clusters

--model: a pickled / torch.save'd NeuralPlda (a pickle written by the reference loads through neuralplda_amd.compat).
--xvectors: Kaldi `xvector.scp` files or binary vector archives (`.ark`); several may be given.
--reco2utt: `reco utt1 utt2 ...` per line; every recording is clustered on its own (the clustering step of diarization over
sliding-window x-vectors).  Utterances it does not list are left out; without it the whole set is one problem of at most
16 384 rows.
Merging takes the pair of clusters with the largest linkage value and stops before the first value below --threshold, or at
--min-clusters clusters per recording.  --threshold is in raw score units unless --calibration A B is given: the a and b
of a score_calibration.fit_linear calibration (llr = a s + b, a > 0).  Average linkage commutes with a positive affine
map, so a threshold t on calibrated scores is the threshold (t - b) / a on raw ones; nothing else is rescaled.
--vb-plda FILE: refine the clustering by VB-HMM resegmentation (VBx) under the Kaldi PLDA model in FILE, whose between-class
variances must belong to the space of the model's embeddings; the utterances of a recording are taken in the order of
--reco2utt (of the table without it), AND THAT ORDER IS THE TIME ORDER.  Cluster with a high --threshold or a --min-clusters
above the expected number of speakers (at most 64 clusters per recording): the clusters are the speaker slots the
refinement starts from.  --vb-fa, --vb-fb, --vb-loop, --vb-max-iters: its scaling factors, self-loop probability and
iteration limit.
--method spectral: spectral clustering with the neighbour count of the affinity graph tuned per recording by the normalised
maximum eigengap instead (cluster.spectral_cluster; at most 2 048 rows per recording): no threshold; --neighbours 4,6,8,...
gives the candidate counts, --max-speakers the most clusters per recording (default 16), --min-clusters the fewest;
--threshold, --calibration and --linkage are not used.
Output: `utt2spk` (sorted by utterance) and `spk2utt` in --out-dir, what every spk2utt consumer of the package reads."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    from identify import load_model, load_table
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--xvectors", required=True, nargs="+")
    ap.add_argument("--reco2utt")
    ap.add_argument("--threshold", type=float, default=float("-inf"))
    ap.add_argument("--calibration", type=float, nargs=2, metavar=("A", "B"),
                    help="--threshold is in units of llr = A s + B (A > 0): it is mapped to (threshold - B) / A")
    ap.add_argument("--min-clusters", type=int, default=1)
    ap.add_argument("--linkage", default="average", choices=["average", "complete", "single"])
    ap.add_argument("--method", default="ahc", choices=["ahc", "spectral"])
    ap.add_argument("--neighbours", help="--method spectral: comma-separated candidate neighbour counts, strictly increasing")
    ap.add_argument("--max-speakers", type=int, default=16, help="--method spectral: the most clusters per recording")
    ap.add_argument("--vb-plda", help="a Kaldi PLDA model: refine the clusters by VB-HMM resegmentation under its psi")
    ap.add_argument("--vb-fa", type=float, default=0.3)
    ap.add_argument("--vb-fb", type=float, default=17.0)
    ap.add_argument("--vb-loop", type=float, default=0.99)
    ap.add_argument("--vb-max-iters", type=int, default=40)
    ap.add_argument("--prefix", default="c")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cluster_xvectors: no HIP device (the clustering has no CPU path)")
    thr = args.threshold
    if args.calibration is not None:
        a, b = args.calibration
        if not a > 0:
            raise SystemExit("cluster_xvectors: a calibration slope must be positive")
        thr = (thr - b) / a
    from neuralplda_amd import backend, cluster
    dev = torch.device(args.device)
    model = load_model(args.model, dev)
    table = load_table(args.xvectors)
    if len(table) == 0:
        raise SystemExit("cluster_xvectors: no x-vectors")
    if args.reco2utt:
        rows, offs, recos, missing = backend.class_layout(table, args.reco2utt)
        if missing:
            print(f"cluster_xvectors: {len(missing)} utterances of {args.reco2utt} are not in the table", file=sys.stderr)
        groups = [p for p in range(len(recos)) for _ in range(int(offs[p + 1] - offs[p]))]
        ids = [table.ids[r] for r in rows]
        x = table.on(dev)[torch.from_numpy(rows).to(dev)]
    else:
        groups, ids, x = None, list(table.ids), table.on(dev)
    if args.method == "spectral":
        nb = [int(v) for v in args.neighbours.split(",")] if args.neighbours else None
        res = cluster.spectral_cluster(model, x, groups=groups, neighbours=nb, min_clusters=args.min_clusters,
                                       max_clusters=args.max_speakers)
    else:
        res = cluster.cluster(model, x, groups=groups, threshold=thr, min_clusters=args.min_clusters, linkage=args.linkage)
    if args.vb_plda:
        from neuralplda_amd import kaldi_format
        psi = kaldi_format.read_plda(args.vb_plda)["Psi_across_covar_diag"]
        res = cluster.vb_refine(model, x, res, psi, groups=groups, Fa=args.vb_fa, Fb=args.vb_fb, loop_prob=args.vb_loop,
                                max_iters=args.vb_max_iters)
    s2u = res.spk2utt(ids, prefix=args.prefix)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "spk2utt"), "w") as fh:
        fh.write("".join(f"{name} {' '.join(utts)}\n" for name, utts in s2u))
    with open(os.path.join(args.out_dir, "utt2spk"), "w") as fh:
        fh.write("".join(f"{u} {name}\n" for u, name in sorted((u, name) for name, utts in s2u for u in utts)))
    print(f"{len(ids)} x-vectors in {len(res.n_clusters)} problems -> {int(res.n_clusters.sum())} clusters in {args.out_dir}",
          file=sys.stderr)


if __name__ == "__main__":
    main()
