#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (needs /root/reference); the outputs are plain arrays / small
text files (never pickles of reference classes, never reference source).  The reference has no
tests or fixtures of its own, so these vectors are what pins oracle/nplda_oracle.py.

    python tests/golden/make_golden.py

Reference symbols executed: utils/models.py NeuralPlda.{__init__, forward, extract_plda_embeddings,
softcdet, crossentropy, loss, cdet, minc, LoadPldaParamsFromKaldi}, GaussianBackend.forward,
utils/sv_trials_loaders.py {combine_trials_and_get_loader, get_trials_loaders_dict,
load_xvec_trials_from_numbatch, load_xvec_trials_from_idbatch}, utils/scorefile_generator.py
generate_{sre,voices}_scores, utils/adaptive_score_normalization.py (exec'd with its two
hard-coded input paths substituted), torch.optim.Adam as driven by xvector_NeuralPlda_pytorch.py:139.
"""
import io
import copy
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.modules.setdefault("kaldi_io", types.ModuleType("kaldi_io"))  # imported but unused by what we call

from utils import models as refm  # noqa: E402
from utils import sv_trials_loaders as refl  # noqa: E402
from utils import scorefile_generator as refs  # noqa: E402

from neuralplda_amd import kaldi_format as kf  # noqa: E402  (our own Kaldi readers)

torch.set_num_threads(4)


class NC:
    """Minimal stand-in for NpldaConf (fields read at utils/models.py:351-363)."""

    def __init__(self, D0=512, D1=170, D2=170, beta=(99.0, 199.0), alpha=15.0, loss="SoftCdet"):
        self.xvector_dim, self.layer1_LDA_dim, self.layer2_PLDA_spkfactor_dim = D0, D1, D2
        self.beta, self.alpha, self.device, self.loss = list(beta), alpha, "cpu", loss


# --- make Kaldi's text output for the reference's parser (Kaldi binaries are absent here) --------

def _kaldi_text_matrix(m):
    rows = ["  " + " ".join(repr(float(v)) for v in r) for r in m]
    return (" [\n" + " \n".join(rows) + " ]\n").encode()


def _kaldi_text_vector(v):
    return (" [ " + " ".join(repr(float(x)) for x in v) + " ]\n").encode()


def fake_check_output(cmd, *a, **k):
    """What `copy-matrix/copy-vector/ivector-copy-plda --binary=false <file> -` would print, produced
    by our own readers at full precision (Kaldi itself would round to 7 significant digits)."""
    prog, path = cmd[0], cmd[2]
    if prog == "copy-matrix":
        return _kaldi_text_matrix(kf.read_matrix(path))
    if prog == "copy-vector":
        return _kaldi_text_vector(kf.read_vector(path))
    if prog == "ivector-copy-plda":
        p = kf.read_plda(path)
        return (b"<Plda> " + _kaldi_text_vector(p["plda_mean"]) + _kaldi_text_matrix(p["diagonalizing_transform"])
                + _kaldi_text_vector(p["Psi_across_covar_diag"]) + b"</Plda> \n")
    raise RuntimeError(cmd)


def kaldi_init_model(nc):
    m = refm.NeuralPlda(nc)
    real = subprocess.check_output
    subprocess.check_output = fake_check_output
    try:
        m.LoadPldaParamsFromKaldi(f"{REF}/Kaldi_Models/mean.vec", f"{REF}/Kaldi_Models/transform.mat",
                                  f"{REF}/Kaldi_Models/plda")
    finally:
        subprocess.check_output = real
    return m


def params_of(m):
    sd = m.state_dict()
    return dict(W1=sd["centering_and_LDA.weight"].numpy().copy(), b1=sd["centering_and_LDA.bias"].numpy().copy(),
                W2=sd["centering_and_wccn_plda.weight"].numpy().copy(),
                b2=sd["centering_and_wccn_plda.bias"].numpy().copy(), P_sqrt=sd["P_sqrt"].numpy().copy(),
                Q=sd["Q"].numpy().copy())


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")


def g5b():
    """G5b: NeuralPlda.minc on labels outside {0, 1}.  The reference picks the classes with t > 0.5 / t < 0.5 but divides by
    target.sum() and (1 - target).sum() over all labels; quantised scores make ties.  Own RNG stream: no other fixture moves."""
    rg = np.random.default_rng(55)
    N = 256
    tb = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)[rg.integers(0, 5, N)]
    sb = (np.round((rg.standard_normal(N) * 0.5 + 0.5 * (tb > 0.5)) * 16) / 16).astype(np.float32)
    betas = (1.0, 9.9)
    m = refm.NeuralPlda(NC(D0=64, D1=24, D2=20, beta=betas))
    with torch.no_grad():
        minc, th = m.minc(torch.from_numpy(sb), torch.from_numpy(tb))
    save("g5b_metrics_labels.npz", s=sb, t=tb, beta=np.asarray(betas), minc=np.asarray(minc),
         minc_th=np.asarray([th[b].item() for b in betas]))


def main():
    mean_vec = kf.read_vector(f"{REF}/Kaldi_Models/mean.vec")

    # ---- G1: Kaldi-initialised parameters (D1 = D2 = 170) ---------------------------------------
    nc = NC()
    torch.manual_seed(1)
    mk = kaldi_init_model(nc)
    pk = params_of(mk)
    plda = kf.read_plda(f"{REF}/Kaldi_Models/plda")
    save("g1_kaldi_params.npz", **pk, psi=plda["Psi_across_covar_diag"], plda_mean=plda["plda_mean"],
         state_dict_keys=np.asarray(list(mk.state_dict().keys())))

    # ---- G2: forward with intermediates ----------------------------------------------------------
    rng = np.random.default_rng(1234)
    B = 64
    x1 = (mean_vec + rng.standard_normal((B, 512))).astype(np.float32)
    x2 = (mean_vec + rng.standard_normal((B, 512))).astype(np.float32)
    with torch.no_grad():
        t1, t2 = torch.from_numpy(x1), torch.from_numpy(x2)
        u1 = mk.centering_and_LDA(t1)
        y1 = torch.nn.functional.normalize(u1)
        z1 = mk.extract_plda_embeddings(t1)
        z2 = mk.extract_plda_embeddings(t2)
        s = mk.forward(t1, t2)
        s_from_z = mk.forward_from_plda_embeddings(z1, z2)
        md = kaldi_init_model(nc).double()
        s64 = md.forward(t1.double(), t2.double())
        s1 = mk.forward(t1[:1], t2[:1])
    save("g2_forward_kaldi170.npz", x1=x1, x2=x2, u1=u1.numpy(), y1=y1.numpy(), z1=z1.numpy(), z2=z2.numpy(),
         s=s.numpy(), s_from_z=s_from_z.numpy(), s64=s64.numpy(), s_b1=s1.numpy())

    # D = 150 random-init model (nn.Linear default init, torch.rand P_sqrt/Q)
    nc150 = NC(D1=150, D2=150)
    torch.manual_seed(150)
    m150 = refm.NeuralPlda(nc150)
    p150 = params_of(m150)
    Bs = 48
    xa = rng.standard_normal((Bs, 512)).astype(np.float32)
    xb = rng.standard_normal((Bs, 512)).astype(np.float32)
    xa[7] = 0.0  # with b1 zeroed below this row hits the eps branch of F.normalize
    with torch.no_grad():
        s150 = m150.forward(torch.from_numpy(xa), torch.from_numpy(xb))
        m150.centering_and_LDA.bias.zero_()
        s150_zero_bias = m150.forward(torch.from_numpy(xa), torch.from_numpy(xb))
    save("g2_forward_rand150.npz", **p150, x1=xa, x2=xb, s=s150.numpy(), s_zero_b1=s150_zero_bias.numpy())

    # ---- G3: loss + gradients on a small model (full grads) and on the 170-d model (s, L, g) ----
    ncs = NC(D0=64, D1=24, D2=20)
    torch.manual_seed(3)
    ms = refm.NeuralPlda(ncs)
    with torch.no_grad():
        ms.threshold[99.0].fill_(-0.5)
        ms.threshold[199.0].fill_(-0.3)
        ms.threshold_Xent.fill_(0.25)
    ps = params_of(ms)
    Bg = 512
    xg1 = rng.standard_normal((Bg, 64)).astype(np.float32)
    xg2 = rng.standard_normal((Bg, 64)).astype(np.float32)
    tg = (rng.random(Bg) < 0.1).astype(np.float32)
    out = {}
    for lossname in ("SoftCdet", "crossentropy"):
        ms.lossfn = lossname
        ms.zero_grad()
        sc = ms(torch.from_numpy(xg1), torch.from_numpy(xg2))
        sc.retain_grad()
        L = ms.loss(sc, torch.from_numpy(tg))
        L.backward()
        out[lossname + "_L"] = L.detach().numpy()
        out[lossname + "_g"] = sc.grad.numpy().copy()
        for k, prm in ms.named_parameters():
            out[f"{lossname}_grad_{k}"] = (prm.grad.numpy().copy() if prm.grad is not None
                                           else np.zeros(prm.shape, np.float32))
        out[lossname + "_s"] = sc.detach().numpy()
    # fp64 re-evaluation of the SoftCdet gradient (tighter yardstick)
    msd = refm.NeuralPlda(ncs).double()
    msd.load_state_dict({k: v.double() for k, v in ms.state_dict().items()})
    msd.threshold = {99.0: msd.Th99, 199.0: msd.Th199}
    msd.alpha = torch.tensor(15.0, dtype=torch.float64)
    msd.lossfn = "SoftCdet"
    scd = msd(torch.from_numpy(xg1).double(), torch.from_numpy(xg2).double())
    scd.retain_grad()
    Ld = msd.softcdet(scd, torch.from_numpy(tg).double())
    Ld.backward()
    for k, prm in msd.named_parameters():
        if prm.grad is not None:
            out[f"SoftCdet64_grad_{k}"] = prm.grad.numpy().copy()
    out["SoftCdet64_L"] = Ld.detach().numpy()
    out["SoftCdet64_g"] = scd.grad.numpy().copy()
    save("g3_loss_grad_small.npz", **ps, x1=xg1, x2=xg2, t=tg, theta=np.asarray([-0.5, -0.3]), theta_xent=0.25,
         beta=np.asarray([99.0, 199.0]), alpha=15.0, **out)

    with torch.no_grad():
        mk.threshold[99.0].fill_(-0.9)
        mk.threshold[199.0].fill_(-0.8)
    tk = (rng.random(B) < 0.25).astype(np.float32)
    mk.lossfn = "SoftCdet"
    mk.zero_grad()
    sk = mk(torch.from_numpy(x1), torch.from_numpy(x2))
    sk.retain_grad()
    Lk = mk.loss(sk, torch.from_numpy(tk))
    Lk.backward()
    save("g3_loss_kaldi170.npz", t=tk, theta=np.asarray([-0.9, -0.8]), beta=np.asarray([99.0, 199.0]), alpha=15.0,
         L=Lk.detach().numpy(), g=sk.grad.numpy(), grad_Q=mk.Q.grad.numpy(), grad_P_sqrt=mk.P_sqrt.grad.numpy(),
         grad_b2=mk.centering_and_wccn_plda.bias.grad.numpy(), grad_b1=mk.centering_and_LDA.bias.grad.numpy(),
         grad_W2_row0=mk.centering_and_wccn_plda.weight.grad.numpy()[0],
         grad_W1_row0=mk.centering_and_LDA.weight.grad.numpy()[0],
         grad_W1_fro=np.linalg.norm(mk.centering_and_LDA.weight.grad.numpy()),
         grad_W2_fro=np.linalg.norm(mk.centering_and_wccn_plda.weight.grad.numpy()),
         grad_Th99=mk.Th99.grad.numpy(), grad_Th199=mk.Th199.grad.numpy())

    # ---- G4: 3 Adam steps as the training script takes them (xvector_NeuralPlda_pytorch.py:35-43,139)
    torch.manual_seed(4)
    ma = refm.NeuralPlda(ncs)
    with torch.no_grad():
        ma.threshold[99.0].fill_(-0.5)
        ma.threshold[199.0].fill_(-0.3)
    ma.lossfn = "SoftCdet"
    p0 = {k: v.numpy().copy() for k, v in ma.state_dict().items()}
    opt = torch.optim.Adam(ma.parameters(), lr=1e-4, weight_decay=1e-5)
    losses = []
    for step in range(3):
        opt.zero_grad()
        lo, hi = step * 128, (step + 1) * 128
        o = ma(torch.from_numpy(xg1[lo:hi]), torch.from_numpy(xg2[lo:hi]))
        L = ma.loss(o, torch.from_numpy(tg[lo:hi]))
        losses.append(L.item())
        L.backward()
        opt.step()
    p3 = {k: v.numpy().copy() for k, v in ma.state_dict().items()}
    save("g4_adam_small.npz", losses=np.asarray(losses), keys=np.asarray(list(p0.keys())),
         **{"p0_" + k: v for k, v in p0.items()}, **{"p3_" + k: v for k, v in p3.items()})

    # ---- G5: metrics ------------------------------------------------------------------------------
    N = 2000
    tm = (rng.random(N) < 0.08).astype(np.float32)
    sm = (rng.standard_normal(N) * 0.4 - 1.0 + 0.9 * tm).astype(np.float32)
    nc5 = NC(D0=64, D1=24, D2=20)
    m5 = refm.NeuralPlda(nc5)
    with torch.no_grad():
        m5.threshold[99.0].fill_(-0.2)
        m5.threshold[199.0].fill_(-0.1)
    S, T = torch.from_numpy(sm), torch.from_numpy(tm)
    with torch.no_grad():
        c5 = m5.cdet(S, T).numpy()
        sc5 = m5.softcdet(S, T).numpy()
        xe5 = m5.crossentropy(S, T).numpy()
        minc5, th5 = m5.minc(S, T)
        minc5b, _ = m5.minc(S, T, update_thresholds=True)
        th_after = np.asarray([m5.Th99.item(), m5.Th199.item()])
        # perfectly separable case: quirk floor
        ssep = np.where(tm > 0.5, 1.0 + 0.001 * np.arange(N), -1.0 - 0.001 * np.arange(N)).astype(np.float32)
        mincsep, thsep = m5.minc(torch.from_numpy(ssep), T)
    save("g5_metrics.npz", s=sm, t=tm, theta=np.asarray([-0.2, -0.1]), beta=np.asarray([99.0, 199.0]), alpha=15.0,
         cdet=c5, softcdet=sc5, xent=xe5, minc=np.asarray(minc5), minc_th=np.asarray([th5[99.0].item(), th5[199.0].item()]),
         th_after_update=th_after, s_sep=ssep, minc_sep=np.asarray(mincsep),
         minc_sep_th=np.asarray([thsep[99.0].item(), thsep[199.0].item()]))

    g5b()

    # ---- G6: AS-norm script ------------------------------------------------------------------------
    enr = [f"enr{i}" for i in range(5)]
    tst = [f"tst{i}" for i in range(7)]
    coh = [f"coh{i:04d}" for i in range(600)]
    with tempfile.TemporaryDirectory() as td:
        rawf, cohf = os.path.join(td, "raw.tsv"), os.path.join(td, "cohort.tsv")
        raw_rows, raw_scores = [], []
        for e in enr:
            for t_ in tst:
                v = float(rng.standard_normal())
                raw_rows.append((e, t_ + ".sph", "a"))
                raw_scores.append(v)
        with open(rawf, "w") as f:
            f.write("modelid\tsegmentid\tside\tLLR\n")
            for (e, t_, sd), v in zip(raw_rows, raw_scores):
                f.write(f"{e}\t{t_}\t{sd}\t{float(v)!r}\n")
        ids = enr + tst
        C = rng.standard_normal((len(ids), len(coh))) * (1 + 0.1 * np.arange(len(ids)))[:, None] - 0.5
        with open(cohf, "w") as f:
            f.write("id\tcohort\tLLR\n")
            for i, a in enumerate(ids):
                for j, c in enumerate(coh):
                    f.write(f"{a}\t{c}\t{float(C[i, j])!r}\n")
        src = open(f"{REF}/utils/adaptive_score_normalization.py").read()
        src = re.sub(r"^raw_score_filename = .*$", f"raw_score_filename = {rawf!r}", src, flags=re.M)
        src = re.sub(r"^cohort_score_filename = .*$", f"cohort_score_filename = {cohf!r}", src, flags=re.M)
        exec(compile(src, "adaptive_score_normalization.py", "exec"), {"__name__": "asnorm_ref"})
        outs = {}
        for suf in ("znorm", "tnorm", "snorm", "asnorm1"):
            txt = open(rawf + f"_{suf}.tsv").read()
            outs[suf + "_text"] = np.asarray(txt)
            tab = np.genfromtxt(io.StringIO(txt), dtype=str, skip_header=1)
            outs[suf] = tab[:, -1].astype(np.float64)
    save("g6_asnorm.npz", cohort=C, ids=np.asarray(ids), raw=np.asarray(raw_scores),
         enroll=np.asarray([r[0] for r in raw_rows]), test=np.asarray([r[1] for r in raw_rows]),
         side=np.asarray([r[2] for r in raw_rows]), topn=500, **outs)

    # ---- G7: GaussianBackend.forward ----------------------------------------------------------------
    ncg = NC(D0=32, D1=16, D2=16)
    torch.manual_seed(7)
    gb = refm.GaussianBackend(ncg)
    A = torch.randn(32, 32)
    gb.paired_cov_inv_target = A @ A.T / 32 + torch.eye(32)
    A = torch.randn(32, 32)
    gb.paired_cov_inv_nontarget = A @ A.T / 32 + 0.5 * torch.eye(32)
    gb.paired_mean_target = 0.1 * torch.randn(32)
    gb.paired_mean_nontarget = 0.1 * torch.randn(32)
    xg_a = rng.standard_normal((40, 32)).astype(np.float32)
    xg_b = rng.standard_normal((40, 32)).astype(np.float32)
    with torch.no_grad():
        sg = gb.forward(torch.from_numpy(xg_a), torch.from_numpy(xg_b))
        xp = gb.forward_getpaired(torch.from_numpy(xg_a), torch.from_numpy(xg_b))
    save("g7_gb.npz", W1=gb.centering_and_LDA.weight.detach().numpy(), b1=gb.centering_and_LDA.bias.detach().numpy(),
         mu_t=gb.paired_mean_target.numpy(), Lam_t=gb.paired_cov_inv_target.numpy(),
         mu_n=gb.paired_mean_nontarget.numpy(), Lam_n=gb.paired_cov_inv_nontarget.numpy(),
         x1=xg_a, x2=xg_b, s=sg.numpy(), paired=xp.numpy())
    # GaussianBackend at the shipped LDA size (170) — scores only, params derived from g1 + seeded stats
    ncg2 = NC(D0=512, D1=170, D2=170)
    gb2 = refm.GaussianBackend(ncg2)
    with torch.no_grad():
        gb2.centering_and_LDA.weight.copy_(torch.from_numpy(pk["W1"]))
        gb2.centering_and_LDA.bias.copy_(torch.from_numpy(pk["b1"]))
    rg = np.random.default_rng(77)
    A = rg.standard_normal((340, 340)).astype(np.float32)
    Lt = (A @ A.T / 340 + np.eye(340, dtype=np.float32)).astype(np.float32)
    A = rg.standard_normal((340, 340)).astype(np.float32)
    Ln = (A @ A.T / 340 + 0.5 * np.eye(340, dtype=np.float32)).astype(np.float32)
    mt = (0.05 * rg.standard_normal(340)).astype(np.float32)
    mn = (0.05 * rg.standard_normal(340)).astype(np.float32)
    gb2.paired_cov_inv_target, gb2.paired_cov_inv_nontarget = torch.from_numpy(Lt), torch.from_numpy(Ln)
    gb2.paired_mean_target, gb2.paired_mean_nontarget = torch.from_numpy(mt), torch.from_numpy(mn)
    with torch.no_grad():
        sg2 = gb2.forward(torch.from_numpy(x1), torch.from_numpy(x2))
    save("g7_gb_kaldi170.npz", seed=77, s=sg2.numpy())

    # ---- G10: DPlda.forward (utils/models.py:463-495), forward only -------------------------------------------
    ncd = NC(D0=64, D1=24, D2=24)
    torch.manual_seed(10)
    dp = refm.DPlda(ncd)
    rng10 = np.random.default_rng(10)  # own stream: the fixtures generated after this block must not move
    xd1 = rng10.standard_normal((50, 64)).astype(np.float32)
    xd2 = rng10.standard_normal((50, 64)).astype(np.float32)
    with torch.no_grad():
        sd_ = dp.forward(torch.from_numpy(xd1), torch.from_numpy(xd2))
        yd = dp.extract_plda_embeddings(torch.from_numpy(xd1))
        sfe = dp.forward_from_plda_embeddings(yd, dp.extract_plda_embeddings(torch.from_numpy(xd2)))
    save("g10_dplda_small.npz", W1=dp.centering_and_LDA.weight.detach().numpy(), b1=dp.centering_and_LDA.bias.detach().numpy(),
         wlr=dp.logistic_regres.weight.detach().numpy(), blr=dp.logistic_regres.bias.detach().numpy(), x1=xd1, x2=xd2,
         s=sd_.numpy(), y1=yd.numpy(), s_from_emb=sfe.numpy(),
         state_dict_keys=np.asarray(list(dp.state_dict().keys())))
    ncd2 = NC(D0=512, D1=170, D2=170)
    dp2 = refm.DPlda(ncd2)
    rgd = np.random.default_rng(1010)
    wlr2 = (rgd.standard_normal((1, 2 * 170 * 170 + 170)) * 0.05).astype(np.float32)
    with torch.no_grad():
        dp2.centering_and_LDA.weight.copy_(torch.from_numpy(pk["W1"]))
        dp2.centering_and_LDA.bias.copy_(torch.from_numpy(pk["b1"]))
        dp2.logistic_regres.weight.copy_(torch.from_numpy(wlr2))
        dp2.logistic_regres.bias.fill_(0.125)
        sd2 = dp2.forward(torch.from_numpy(x1), torch.from_numpy(x2))
    save("g10_dplda_kaldi170.npz", seed=1010, s=sd2.numpy())
    # gradient of the linear unit (the recipe trains logistic_regres + thresholds with the LDA frozen,
    # xvector_DPlda_pytorch.py:140-147): reference autograd, fp32 and an fp64 re-evaluation
    td = (rng10.random(50) < 0.3).astype(np.float32)
    outg = {}
    for tag, mdl, cast in (("f32", dp, lambda a: torch.from_numpy(a)), ("f64", copy.deepcopy(dp).double(), lambda a: torch.from_numpy(a).double())):
        with torch.no_grad():
            mdl.threshold[99.0].fill_(0.2)
            mdl.threshold[199.0].fill_(0.35)
        for lossname in ("SoftCdet", "crossentropy"):
            mdl.lossfn = lossname
            mdl.zero_grad()
            sg_ = mdl(cast(xd1), cast(xd2))
            Lg_ = mdl.loss(sg_, cast(td))
            Lg_.backward()
            outg[f"{lossname}_{tag}_L"] = Lg_.detach().numpy()
            outg[f"{lossname}_{tag}_dwlr"] = mdl.logistic_regres.weight.grad.numpy().copy()
            outg[f"{lossname}_{tag}_dblr"] = mdl.logistic_regres.bias.grad.numpy().copy()
            if lossname == "SoftCdet":
                outg[f"{lossname}_{tag}_dTh99"] = mdl.threshold[99.0].grad.numpy().copy()
                outg[f"{lossname}_{tag}_dTh199"] = mdl.threshold[199.0].grad.numpy().copy()
    save("g10_dplda_grad.npz", t=td, theta=np.asarray([0.2, 0.35]), **outg)

    # ---- G8: loaders and score-file writers ----------------------------------------------------------
    nutt = 150
    utt_ids = [f"spk{u // 5:03d}-utt{u:04d}" for u in range(nutt)]
    xv = rng.standard_normal((nutt, 512)).astype(np.float32)
    mega = {u: xv[i] for i, u in enumerate(utt_ids)}
    num_to_id = {i: u for i, u in enumerate(utt_ids)}
    id_to_num = {u: i for i, u in enumerate(utt_ids)}
    ntr = 1000
    a = rng.integers(0, nutt, ntr)
    b = rng.integers(0, nutt, ntr)
    lab = (a // 5 == b // 5).astype(int)
    trial_lines = [f"{utt_ids[i]}\t{utt_ids[j]}\t{l}" for i, j, l in zip(a, b, lab)]
    trial_lines[10] = f"UNKNOWN\t{utt_ids[3]}\t0"  # silently dropped by the reference (:379-383)
    val_lines = [f"{utt_ids[i]}\t{utt_ids[j]}.wav\t{l}" for i, j, l in zip(a[:200], b[:200], lab[:200])]
    with tempfile.TemporaryDirectory() as td:
        trf, vaf = os.path.join(td, "train_trials.tsv"), os.path.join(td, "val_trials.tsv")
        open(trf, "w").write("\n".join(trial_lines) + "\n")
        open(vaf, "w").write("\n".join(val_lines) + "\n")
        np.random.seed(1)
        torch.manual_seed(1)
        loader = refl.combine_trials_and_get_loader([trf], id_to_num, subsample_factors=[0.5], batch_size=32)
        kept = np.asarray(loader.dataset.datasets[0].indices)
        d1, d2, tt = next(iter(loader))
        np.random.seed(2)
        torch.manual_seed(2)
        vd = refl.get_trials_loaders_dict([vaf], id_to_num, subsample_factors=[1.01], batch_size=50)
        vkey = list(vd.keys())
        v1, v2, vt = next(iter(vd[vkey[0]]))
        X1, X2 = refl.load_xvec_trials_from_numbatch(mega, num_to_id, d1, d2, torch.device("cpu"))
        idtr = np.asarray([[f"/some/dir/{utt_ids[i]}.wav", f"{utt_ids[j]}.sph"] for i, j in zip(a[:16], b[:16])])
        I1, I2 = refl.load_xvec_trials_from_idbatch(mega, idtr, torch.device("cpu"))
        # score files (model forced to CPU by the reference)
        mk.eval()
        vo_trials = os.path.join(td, "voices_trials.lst")
        open(vo_trials, "w").write("\n".join(f"{utt_ids[i]} {utt_ids[j]}.wav {'tgt' if l else 'imp'}"
                                             for i, j, l in zip(a[:37], b[:37], lab[:37])) + "\n")
        vo_out = os.path.join(td, "voices_scores.txt")
        refs.generate_voices_scores(vo_out, vo_trials, mega, mk, torch.device("cpu"), batch_size=16)
        sre_trials = os.path.join(td, "sre_trials.tsv")
        open(sre_trials, "w").write("modelid\tsegmentid\tside\n" + "\n".join(
            f"{utt_ids[i]}\t{utt_ids[j]}.sph\ta" for i, j in zip(a[:37], b[:37])) + "\n")
        sre_out = os.path.join(td, "sre_scores.tsv")
        refs.generate_sre_scores(sre_out, sre_trials, mega, mk, torch.device("cpu"), batch_size=16)
        save("g8_loaders.npz", xvec=xv, utt_ids=np.asarray(utt_ids), train_trials_text=np.asarray(open(trf).read()),
             val_trials_text=np.asarray(open(vaf).read()), kept=kept, batch_d1=d1.numpy(), batch_d2=d2.numpy(),
             batch_t=tt.numpy(), val_key=np.asarray(vkey), val_d1=v1.numpy(), val_d2=v2.numpy(), val_t=vt.numpy(),
             n_train_dataset=len(loader.dataset), n_val_dataset=len(vd[vkey[0]].dataset),
             X1=X1.numpy(), X2=X2.numpy(), idtrials=idtr, I1=I1.numpy(), I2=I2.numpy(),
             voices_trials_text=np.asarray(open(vo_trials).read()), voices_scores_text=np.asarray(open(vo_out).read()),
             sre_trials_text=np.asarray(open(sre_trials).read()), sre_scores_text=np.asarray(open(sre_out).read()))

    # ---- G9: end-to-end speaker-structured synthetic set under Kaldi init -----------
    # x is regenerated from the seed by tests/synth.py (committed); the fixture keeps a fingerprint of
    # it (first rows + column sums) so RNG drift is detected instead of silently changing the inputs.
    from tests import synth
    S_spk, U = 400, 5
    x9, spk = synth.speaker_structured_xvectors(pk["W1"], pk["b1"], pk["W2"].astype(np.float64),
                                                plda["plda_mean"], plda["Psi_across_covar_diag"], S_spk, U, 2.0, 7)
    ia, ib, t9 = synth.trial_list(spk, 20000, 200, U, 7)
    with torch.no_grad():
        s9 = mk.forward(torch.from_numpy(x9[ia]), torch.from_numpy(x9[ib])).numpy()
        minc9, th9 = mk.minc(torch.from_numpy(s9), torch.from_numpy(t9))
    save("g9_e2e_kaldi170.npz", seed=7, S=S_spk, U=U, c=2.0, x_head=x9[:4], x_colsum=x9.sum(axis=0, dtype=np.float64),
         i1=ia, i2=ib, t=t9, s=s9, minc_ref=np.asarray(minc9),
         minc_ref_th=np.asarray([th9[99.0].item(), th9[199.0].item()]))


if __name__ == "__main__":
    if sys.argv[1:] == ["g5b"]:  # one fixture alone
        g5b()
    else:
        main()
