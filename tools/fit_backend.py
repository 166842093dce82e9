#!/usr/bin/env python3
"""mean.vec, transform.mat and plda from x-vector archives and a spk2utt — Kaldi's ivector-mean, ivector-compute-lda and
ivector-compute-plda in one GPU pass (neuralplda_amd/backend.py).

    python tools/fit_backend.py --xvector-scp exp/xvectors_train/xvector.scp --spk2utt data/train/spk2utt \\
        --lda-dim 150 --out-dir exp/backend [--plda-dim 150] [--length-norm unit|sqrt_dim] \\
        [--center-scp exp/xvectors_indomain/xvector.scp] [--device cuda:0]

--xvector-scp / --xvector-ark may be repeated.  The files in --out-dir are read by NeuralPlda.LoadPldaParamsFromKaldi,
DPlda.LoadParamsFromKaldi, GaussianBackend.LoadPldaParamsFromKaldi and by Kaldi's own tools."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _table(scps, arks, XvectorTable):
    from neuralplda_amd import kaldi_format
    parts = [kaldi_format.load_vector_scp(p) for p in scps] + [kaldi_format.load_vector_ark(p) for p in arks]
    return XvectorTable._from_parts(parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--xvector-scp", action="append", default=[])
    ap.add_argument("--xvector-ark", action="append", default=[])
    ap.add_argument("--spk2utt", required=True)
    ap.add_argument("--lda-dim", type=int, required=True)
    ap.add_argument("--plda-dim", type=int, default=None)
    ap.add_argument("--length-norm", choices=("unit", "sqrt_dim"), default="unit")
    ap.add_argument("--center-scp", action="append", default=[], help="in-domain x-vectors whose mean becomes mean.vec")
    ap.add_argument("--num-em-iters", type=int, default=10)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not a.xvector_scp and not a.xvector_ark:
        ap.error("give --xvector-scp or --xvector-ark")
    from neuralplda_amd import backend
    from neuralplda_amd.sv_trials_loaders import XvectorTable
    table = _table(a.xvector_scp, a.xvector_ark, XvectorTable)
    center = _table(a.center_scp, [], XvectorTable) if a.center_scp else None
    be = backend.fit_backend(table, a.spk2utt, a.lda_dim, plda_dim=a.plda_dim, length_norm=a.length_norm, center=center,
                             num_em_iters=a.num_em_iters, device=a.device)
    be.save(a.out_dir)
    print(f"{a.out_dir}: mean.vec ({be.mean_vec.shape[0]}), transform.mat {be.transform_mat.shape}, plda {be.plda_transform.shape}"
          f" from {len(table)} x-vectors; psi {be.psi[0]:.4g} .. {be.psi[-1]:.4g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
