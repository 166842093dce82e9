#!/usr/bin/env python3
"""Calibrate a score file: the command-line form of neuralplda_amd.score_calibration.calibrate_scorefile.

    python tools/calibrate_scores.py DEV_SCORES DEV_KEY SCORES [--method gaussian|linear|pav] [--out PATH]
                                     [--label-col 3] [--dev-skip-header 1] [--skip-header 1]
                                     [--p-target 0.5] [--l2 0] [--key EVAL_KEY] [--betas 99,199]

Trains on the last column of DEV_SCORES with the labels of column --label-col of DEV_KEY ('target' / 'tgt',
'nontarget' / 'imp'; other labels are ignored) and writes SCORES with its last column calibrated ('{:f}') to
<SCORES>_calibrated<ext>.  With --key (a key file for SCORES, same layout as DEV_KEY) it also prints Cllr, the cost at
the Bayes threshold (act_cost), the minimum cost (minc_exact) and min Cllr (the Cllr of the best monotone map, which
calibration cannot change) before and after.  Needs a HIP device.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dev_scores")
    ap.add_argument("dev_key")
    ap.add_argument("scores")
    ap.add_argument("--method", choices=("gaussian", "linear", "pav"), default="gaussian")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label-col", type=int, default=3)
    ap.add_argument("--dev-skip-header", type=int, default=1)
    ap.add_argument("--skip-header", type=int, default=1)
    ap.add_argument("--p-target", type=float, default=0.5, help="linear: the prior the fit is weighted for")
    ap.add_argument("--l2", type=float, default=0.0, help="linear: ridge on the scale(s)")
    ap.add_argument("--key", default=None, help="key file of SCORES: print Cllr / act_cost / minc_exact before and after")
    ap.add_argument("--betas", default="99,199", help="cost ratios of act_cost / minc_exact (NpldaConf's beta)")
    a = ap.parse_args(argv)
    import numpy as np
    from neuralplda_amd import metrics, score_calibration as sc
    kw = dict(p_target=a.p_target, l2=a.l2) if a.method == "linear" else {}
    out, model = sc.calibrate_scorefile(a.dev_scores, a.dev_key, a.scores, method=a.method, label_col=a.label_col,
                                        dev_skip_header=a.dev_skip_header, skip_header=a.skip_header, out=a.out, **kw)
    print(f"model: {model!r}")
    print(f"wrote {out}")
    if a.key:
        import torch
        betas = [float(b) for b in a.betas.split(",")]
        target = sc.labels_to_target(np.array(_column(a.key, a.label_col, a.skip_header, False)))
        for name, path in (("before", a.scores), ("after", out)):
            s = torch.from_numpy(_column(path, -1, a.skip_header, True))
            if s.numel() != target.numel():
                raise SystemExit(f"{path}: {s.numel()} scores but {target.numel()} key rows")
            act, _ = metrics.act_cost(s, target, betas)
            mc, _ = metrics.minc_exact(s.float(), target, betas)
            print(f"{name:>6}: Cllr = {metrics.cllr(s, target):.6f}  act_cost = {act:.6f}  minc_exact = {float(mc):.6f}  "
                  f"min_Cllr = {metrics.min_cllr(s, target):.6f}")


if __name__ == "__main__":
    main()
