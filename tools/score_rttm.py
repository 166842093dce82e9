#!/usr/bin/env python3
"""Score a hypothesis RTTM against a reference RTTM: the diarization error rate on one MI355X.

    python tools/score_rttm.py --ref diar/ref.rttm --hyp diar/out.rttm
    python tools/score_rttm.py --ref diar/ref.rttm --hyp diar/out.rttm --uem diar/all.uem --collar 0 --skip-overlap

What NIST md-eval computes, on a grid of --frame-shift seconds (neuralplda_amd.metrics.der, design/k24_der.md): missed
speech, false alarm and speaker confusion over the scored time under the one-to-one speaker mapping that maximises the
matched time.  --collar: seconds on either side of every reference boundary that are not scored (0.25 by default);
--skip-overlap: frames with more than one reference speaker are not scored; --uem: `<recording> <channel> <start> <end>`
regions to evaluate (a recording it does not list is evaluated whole).  Recordings are matched by name; one that only one file
has is scored against nothing.  Output: one line per recording and an OVERALL line whose rate pools the counts."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", required=True)
    ap.add_argument("--hyp", required=True)
    ap.add_argument("--uem")
    ap.add_argument("--collar", type=float, default=0.25)
    ap.add_argument("--skip-overlap", action="store_true")
    ap.add_argument("--frame-shift", type=float, default=0.01)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("score_rttm: no HIP device (the scorer has no CPU path)")
    if not args.frame_shift > 0 or args.collar < 0:
        raise SystemExit("score_rttm: --frame-shift must be positive and --collar must not be negative")
    from neuralplda_amd import metrics
    res = metrics.der(args.ref, args.hyp, uem=args.uem, collar=args.collar, skip_overlap=args.skip_overlap,
                      frame_shift=args.frame_shift)
    print("\n".join(res.lines()))
    return res


if __name__ == "__main__":
    main()
