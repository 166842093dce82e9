#!/usr/bin/env python3
"""Evaluate a score file with bootstrap confidence intervals (neuralplda_amd.metrics.bootstrap, design/k20_bootstrap.md).

    python tools/eval_scores.py SCORES KEY [--label-col 3] [--skip-header 1] [--side1-map FILE] [--side2-map FILE]
                                [--n-boot 1000] [--seed 0] [--betas 99,199] [--alpha 0.05] [--llr]
                                [--compare OTHER_SCORES]

SCORES holds one trial per row with the score in its last column; KEY has the same rows with the two trial ids in
columns 0 and 1 and the label in column --label-col ('target' / 'tgt', 'nontarget' / 'imp'; other labels are ignored).
--skip-header rows are skipped at the top of SCORES, KEY and OTHER_SCORES.  The groups that are resampled are the ids of
columns 0 and 1, or their images under the two-column map files (id -> speaker).  Prints, per metric, the point
estimate and its percentile interval as `A <metric> <point> <lo> <hi>`: EER and the minimum cost per beta, with --llr
(the scores are log-likelihood ratios) also the cost at the Bayes threshold and Cllr.  With --compare the same for the
other system (B) and for the paired differences (A-B, same resamplings), whose last field tells whether the interval
excludes 0.  Needs a HIP device.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _column(path, col, skip, numeric):
    from neuralplda_amd import textio
    with open(path, "rb") as fh:
        for _ in range(skip):
            fh.readline()
        text = fh.read()
    n, _ = textio.scan(text)
    return textio.column_f64(text, col, n) if numeric else textio.column_tokens(text, col, n)


def _groups(key, col, skip, map_path):
    ids = _column(key, col, skip, False)
    if map_path is None:
        return ids
    table = dict(zip(_column(map_path, 0, 0, False), _column(map_path, 1, 0, False)))
    missing = [i for i in ids if i not in table]
    if missing:
        raise SystemExit(f"{map_path}: no entry for {missing[0]!r} ({len(missing)} trials in all)")
    return [table[i] for i in ids]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scores")
    ap.add_argument("key")
    ap.add_argument("--label-col", type=int, default=3)
    ap.add_argument("--skip-header", type=int, default=1)
    ap.add_argument("--side1-map", default=None, help="two columns: id of key column 0 -> group (speaker)")
    ap.add_argument("--side2-map", default=None, help="two columns: id of key column 1 -> group (speaker)")
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--betas", default="99,199", help="cost ratios (NpldaConf's beta)")
    ap.add_argument("--alpha", type=float, default=0.05, help="1 - coverage of the intervals")
    ap.add_argument("--llr", action="store_true", help="the scores are log-likelihood ratios: add act_cost and Cllr")
    ap.add_argument("--compare", default=None, help="scores of another system on the same trials")
    a = ap.parse_args(argv)
    import numpy as np
    from neuralplda_amd import metrics, score_calibration as sc
    betas = [float(b) for b in a.betas.split(",")]
    target = sc.labels_to_target(np.array(_column(a.key, a.label_col, a.skip_header, False)))
    g1 = np.array(_groups(a.key, 0, a.skip_header, a.side1_map))
    g2 = np.array(_groups(a.key, 1, a.skip_header, a.side2_map))
    kw = dict(n_boot=a.n_boot, seed=a.seed, betas=betas, llr=a.llr)
    print(f"{target.numel()} trials, {np.unique(g1).size} x {np.unique(g2).size} groups, {a.n_boot} replicates, "
          f"{100 * (1 - a.alpha):g} % percentile intervals")
    systems = [("A", a.scores)] + ([("B", a.compare)] if a.compare else [])
    scores = {}
    for name, path in systems:
        s = _column(path, -1, a.skip_header, True).astype(np.float32)
        if s.size != target.numel():
            raise SystemExit(f"{path}: {s.size} scores but {target.numel()} key rows")
        scores[name] = s
        res = metrics.bootstrap(s, target, g1, g2, **kw)
        for metric, (p, lo, hi) in metrics.bootstrap_ci(res, alpha=a.alpha).items():
            print(f"{name} {metric} {p:.6f} {lo:.6f} {hi:.6f}")
    if a.compare:
        _, ci = metrics.bootstrap_diff(scores["A"], scores["B"], target, g1, g2, alpha=a.alpha, **kw)
        for metric, (p, lo, hi, excl) in ci.items():
            print(f"A-B {metric} {p:+.6f} {lo:+.6f} {hi:+.6f} {'excludes 0' if excl else 'includes 0'}")


if __name__ == "__main__":
    main()
