"""GPU parity of the detection-cost sweep (nplda_detcost_sweep_f32): NeuralPlda.minc with the reference's quirks bit for
bit (golden G5 = the reference's own outputs), the exact minimum detection cost and the EER against the oracle; and the
rule "which trial counts, and as what" of csrc/nplda_trials.h in the four families that share it."""
import os

import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_minc_reference_semantics_golden(hip_lib):
    from neuralplda_amd import metrics
    g = np.load(os.path.join(G, "g5_metrics.npz"))
    for dev in ("cpu", "cuda"):  # CPU tensors are moved to the device; results come back on the caller's device
        S, T = torch.from_numpy(g["s"]).to(dev), torch.from_numpy(g["t"]).to(dev)
        mc, th = metrics.minc(S, T, [99.0, 199.0])
        assert mc.device.type == dev and mc.dim() == 0
        assert abs(mc.item() - float(g["minc"])) <= 1e-7
        assert th[99.0].item() == np.float32(g["minc_th"][0]) and th[199.0].item() == np.float32(g["minc_th"][1])
        mcs, _ = metrics.minc(torch.from_numpy(g["s_sep"]).to(dev), T, [99.0, 199.0])
        assert abs(mcs.item() - float(g["minc_sep"])) <= 1e-7 and mcs.item() > 0
        assert metrics.minc(torch.from_numpy(g["s_sep"]).to(dev), T, [99.0, 199.0], reference_semantics=False)[0].item() == 0.0
        assert abs(metrics.eer(S, T) - orc.eer(g["s"], g["t"])) < 1e-6
        assert abs(metrics.minc_exact(S, T, [99.0])[0].item() - orc.minc_exact(g["s"], g["t"], [99.0])[0]) < 1e-6


@pytest.mark.parametrize("n,ptgt,quant", [(2, 0.5, None), (17, 0.3, None), (1000, 0.1, 0.05), (4097, 0.02, None),
                                          (300000, 0.01, 0.001), (1 << 20, 0.05, None)])
def test_sweep_vs_oracle(hip_lib, n, ptgt, quant):
    from neuralplda_amd import metrics
    rg = np.random.default_rng(n)
    t = (rg.random(n) < ptgt).astype(np.float32)
    t[0], t[1] = 1.0, 0.0
    s = (rg.standard_normal(n) + 2.0 * t).astype(np.float32)
    if quant:  # heavy ties
        s = (np.round(s / quant) * quant).astype(np.float32)
    betas = [99.0, 199.0, 9.9]
    S, T = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    mc, th = metrics.minc(S, T, betas)
    ref_mc, ref_th = orc.minc_reference(s, t, betas)
    assert abs(mc.item() - float(ref_mc)) <= 1e-6 * max(1.0, abs(float(ref_mc)))
    for b in betas:  # with ties in the cost the oracle (numpy argmin) and the kernel both take the first occurrence
        assert th[b].item() == np.float32(ref_th[b])
    mce, the = metrics.minc(S, T, betas, reference_semantics=False)
    ref_e, ref_the = orc.minc_exact(s, t, betas)
    assert abs(mce.item() - float(ref_e)) <= 1e-6
    for b in betas:
        assert the[b].item() == np.float32(ref_the[b])
    assert abs(metrics.eer(S, T) - orc.eer(s, t)) <= 1e-6
    # determinism
    mc2, th2 = metrics.minc(S, T, betas)
    assert mc2.item() == mc.item() and all(th2[b].item() == th[b].item() for b in betas)


@pytest.mark.parametrize("n", [257, 1025])  # one and four label blocks, plus one trial
def test_one_trial_rule_in_all_four_families(hip_lib, n):
    """csrc/nplda_trials.h on one input (tests/detcost_cases.py: every_exclusion): target iff t > 0.5, non-target iff
    t < 0.5, a label of 0.5 or NaN in neither class; the sorted families (detcost, pav, bootstrap) also drop a trial whose
    score is NaN, the calibration costs do not.  The class counts are NumPy's; the minimum cost is an O(N^2) count over
    the kept trials in exact integers, which the kernel's single fp64 evaluation meets to half a float32 ulp."""
    from fractions import Fraction

    from neuralplda_amd import ops
    from tests import detcost_cases as cases
    from tests import detcost_ref as ref
    s, t = cases.every_exclusion(n, n)
    assert {cases.NAN_NEG, cases.NAN_POS} <= set(s.view(np.uint32).tolist()) and np.isinf(s).any() and np.isnan(t).any()
    assert all((t == v).any() for v in (0.0, 0.25, 0.5, 0.75, 1.0)) and np.unique(s[~np.isnan(s)]).size < n // 2
    ok = ~np.isnan(s)
    tgt, non = (t > 0.5) & ok, (t < 0.5) & ok
    nt, nn = int(tgt.sum()), int(non.sum())
    assert 4 * nt >= n and 4 * nn >= n and ((t > 0.5) & ~ok).any() and ((t < 0.5) & ~ok).any()
    S, T = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    summary = ops.pav_fit(S, T)[5].cpu().numpy()
    g1 = torch.arange(n, dtype=torch.int32, device="cuda") % 7
    totals = ops.bootstrap_metrics(S, T, g1, 7, n_boot=1)[1].cpu().numpy()
    counts = ops.calib_costs(S, T)[0].cpu().numpy()
    beta = 1.0  # an interior threshold wins: at 9 or more, accepting nothing does
    minc = ops.detcost_sweep(S, T, [beta], exact=True)[0].cpu().numpy()
    print("pav", summary[:2], "bootstrap", totals[0], "calib", counts, "numpy", nt, nn, "minc", minc)
    assert summary[0] == nt and summary[1] == nn
    assert totals[0].tolist() == [nt, nn]
    assert counts.tolist() == [int((t > 0.5).sum()), int((t < 0.5).sum())]
    th = np.concatenate([np.unique(s[ok]), [np.inf]])  # every distinct score, then "accept nothing"
    miss = (tgt[None, :] & (s[None, :] < th[:, None])).sum(axis=1)
    fa = (non[None, :] & (s[None, :] >= th[:, None])).sum(axis=1)
    miss[-1], fa[-1] = nt, 0  # the last candidate accepts nothing, a score of +inf included
    want = min(Fraction(int(m), nt) + int(beta) * Fraction(int(f), nn) for m, f in zip(miss, fa))
    assert ref.within_rounding(minc[0], want), (minc[0], float(want))


def test_sweep_edge_cases(hip_lib):
    from neuralplda_amd import _lib, metrics, ops
    s = torch.tensor([0.5, 0.5, 0.5, 0.5], device="cuda")
    t = torch.tensor([1.0, 0.0, 1.0, 0.0], device="cuda")
    mc, th = metrics.minc(s, t, [99.0])
    ref_mc, ref_th = orc.minc_reference(s.cpu().numpy(), t.cpu().numpy(), [99.0])
    assert abs(mc.item() - float(ref_mc)) < 1e-6 and th[99.0].item() == 0.5
    # all non-targets: the reference raises (torch.min of an empty tensor); here the result is NaN
    mc, _ = metrics.minc(s, torch.zeros(4, device="cuda"), [99.0])
    assert np.isnan(mc.item())
    with pytest.raises(_lib.NpldaHipError):
        ops.detcost_sweep(s, t, [1.0] * 9)
    with pytest.raises(ValueError):
        ops.detcost_sweep(s, t[:3], [1.0])
