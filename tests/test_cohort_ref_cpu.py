"""The reference side of tests/test_cohort_fp32_units_gpu.py, checked without a GPU (tests/cohort_ref.py): the order-statistic
probe recovers single scores, ref64 is the exactly rounded score, every fused case's gate separates the six-pass split
product from each of its six dropped-pass forms by 1.5 x on either side, and the probed columns reach every lane position and
both edge tiles."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import nplda_oracle as orc
from tests import cohort_ref as cr


def test_probe_recovers_the_order_statistics():
    c = cr.inputs("normal", "real", 150, 40, 4099)
    ref64, _ = cr.refs(c)
    got = cr.probe(lambda n, select: orc.cohort_stats(ref64, n, select)[:, 2])
    want = cr.order_stats(ref64)
    s = np.sort(ref64, axis=1)
    assert np.array_equal(want[:, :cr.NPROBE], s[:, :cr.NPROBE]) and np.array_equal(want[:, cr.NPROBE:], s[:, ::-1][:, :cr.NPROBE])
    err = np.abs(got - want).max() / np.abs(ref64).max()
    print(f"probe on the oracle's statistics: max error {err:.2e} of the largest score")
    assert err <= 1e-12


@pytest.mark.parametrize("family,qkind,D", [("normal", "real", 170), ("stress", "zero", 150)])
def test_ref64_against_exact_sums(family, qkind, D):
    """ref64 on a sample of entries against the score summed exactly (rational arithmetic on the float32 inputs)."""
    c = cr.inputs(family, qkind, D, 40, 4099)
    ref64, _ = cr.refs(c)
    rng = np.random.default_rng(D)
    P = [Fraction(float(v)) for v in (c["P_sqrt"] * c["P_sqrt"])]   # the image holds fp32(P_sqrt^2)
    worst = 0.0
    for r, m in zip(rng.integers(0, c["R"], 48), rng.integers(0, c["M"], 48)):
        terms = [2 * P[d] * Fraction(float(c["zr"][r, d])) * Fraction(float(c["zc"][m, d])) for d in range(D)]
        exact = Fraction(float(c["qr"][r])) + Fraction(float(c["qc"][m])) + sum(terms)
        mag = abs(float(c["qr"][r])) + abs(float(c["qc"][m])) + math.fsum(abs(float(t)) for t in terms)
        worst = max(worst, abs(float(Fraction(float(ref64[r, m])) - exact)) / mag)
    print(f"ref64 against exact sums: worst error {worst:.2e} of the summed magnitudes")
    assert worst <= (D + 4) * 2.0 ** -53


@pytest.mark.parametrize("family,qkind,D,M", cr.FUSED_INPUTS)
def test_gate_separates_the_split_product_from_its_dropped_pass_forms(family, qkind, D, M):
    s = cr.summary(family, qkind, D, cr.R_FUSED, M)
    for k in ("all", "probe"):
        v = s[k]
        print(f"{family} q={qkind} D={D} M={M} {k}: r_ok {v['r_ok']:.3f} r_mut {v['r_mut']:.3f} g {v['g']:.3f} dropped "
              + " ".join(f"{p} {x:.3g}" for p, x in v["dropped"].items()))
        assert v["r_ok"] <= v["g"] / 1.5 and v["r_mut"] >= 1.5 * v["g"], (k, v)


@pytest.mark.parametrize("family,qkind,D,M", cr.FUSED_INPUTS)
def test_probe_coverage(family, qkind, D, M):
    s = cr.summary(family, qkind, D, cr.R_FUSED, M)
    print(f"{family} q={qkind} D={D} M={M}: probed columns per position mod 64 min {s['lane_hits'].min()}, first tile "
          f"{s['first_tile_hits']}, last tile {s['last_tile_hits']}")
    assert s["lane_hits"].min() >= 16
    assert s["last_tile_hits"] >= 16
    assert s["first_tile_hits"] >= 64
