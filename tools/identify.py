#!/usr/bin/env python3
"""1:N identification: the k best-scoring gallery entries for every probe x-vector, on one MI355X.

    python tools/identify.py --model models/NPLDA.pt --gallery enroll/xvector.scp --probes test/xvector.scp --k 10 --out top10.tsv

--model: a pickled / torch.save'd NeuralPlda (a pickle written by the reference loads through neuralplda_amd.compat).
--gallery / --probes: Kaldi `xvector.scp` files or binary vector archives (`.ark`); several may be given for either.
The gallery is embedded once (search.Gallery), the probes are searched in blocks of --block; the probes x gallery score matrix
is never written.  Output: a TSV of probe_id, rank (1 = best), gallery_id, score; a probe facing a gallery of fewer than k
entries gets as many lines as there are entries."""
import argparse
import os
import pickle
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_model(path, dev):
    from neuralplda_amd import compat, models
    compat.install()
    try:
        obj = torch.load(path, map_location="cpu", weights_only=False)
    except Exception:
        with open(path, "rb") as fh:
            obj = pickle.load(fh)
    if not isinstance(obj, models.NeuralPlda):
        raise SystemExit(f"{path}: expected a pickled NeuralPlda, got {type(obj).__name__}")
    return obj.to(dev).eval().requires_grad_(False)


def load_table(paths):
    from neuralplda_amd.sv_trials_loaders import XvectorTable
    arks = [p for p in paths if p.endswith(".ark")]
    scps = [p for p in paths if not p.endswith(".ark")]
    if arks and scps:
        raise SystemExit("give archives or scp files for one side, not both")
    return XvectorTable.from_ark(*arks) if arks else XvectorTable.from_scp(*scps)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--gallery", required=True, nargs="+")
    ap.add_argument("--probes", required=True, nargs="+")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", required=True)
    ap.add_argument("--block", type=int, default=16384, help="probes per search call")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("identify: no HIP device (the search has no CPU path)")
    from neuralplda_amd import search
    dev = torch.device(args.device)
    model = load_model(args.model, dev)
    gallery, probes = load_table(args.gallery), load_table(args.probes)
    if len(gallery) == 0 or len(probes) == 0:
        raise SystemExit("identify: an empty gallery or probe list")
    gal = search.Gallery.build(model, gallery.on(dev), ids=gallery.ids)
    xp = probes.on(dev)
    with open(args.out, "w") as out:
        for lo in range(0, len(probes), args.block):
            vals, idx = gal.search(xp[lo:lo + args.block], k=args.k)
            vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
            for r in range(idx.shape[0]):
                pid = probes.ids[lo + r]
                for rank, (j, s) in enumerate(zip(idx[r], vals[r]), 1):
                    if j >= 0:
                        out.write(f"{pid}\t{rank}\t{gallery.ids[j]}\t{s:.6f}\n")
    print(f"{len(probes)} probes x {len(gallery)} gallery entries -> {args.out}", file=sys.stderr)


if __name__ == "__main__":
    main()
