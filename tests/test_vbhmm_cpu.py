"""The VB-HMM resegmentation without a GPU: the numpy twins of tests/vbhmm_ref.py against each other and against longdouble, the
twin's ELBO trace, the recovery of over-clustered separable speakers, the argument checks of the C entry points (status codes
come before any launch), the declared names and the resource budget of csrc/nplda_vbhmm.hip."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import vbhmm_ref as vr
from tests.test_topk_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(17, 2), (65, 3), (300, 7), (1000, 12)]
SEED = 200      # see test_elbo_trace_of_the_twin_does_not_decrease


def test_longdouble_is_wider_than_float64():
    assert np.finfo(np.longdouble).nmant >= 63


# ---- the twins ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def twins(T, S, sep, Fa, Fb, iters):
    x, psi, lab, _ = vr.make_problem(SEED + 31 * T + S, T, S, 128, sep)
    g0 = vr.gamma_from_labels(lab, S)
    kw = dict(Fa=Fa, Fb=Fb, max_iters=iters, eps=-np.inf)
    return (vr.vbhmm(x, psi, g0, dtype=np.longdouble, **kw), vr.vbhmm(x, psi, g0, **kw), vr.vbhmm_scaled(x, psi, g0, **kw))


@pytest.mark.parametrize("T,S", SHAPES)
@pytest.mark.parametrize("iters", [1, 40])
def test_second_formulation_within_the_gates(T, S, iters):
    """Per-step normalisation, the O(S) step and sums in another order against the log-domain twin, in units of that twin's own
    float64 error.  Measured, the worst of all cases (rms / max): gamma 0.04 / 0.02, pi 0.65 / 0.65 and the ELBO 0.89, all
    three at T = 17; the unit on gamma after one iteration is 3e-13 (T = 17) .. 1.3e-9 (T = 1000)."""
    for sep in (0.1, 0.25):
        for Fa, Fb in ((0.3, 17.0), (1.0, 1.0)):
            ld, r64, sc = twins(T, S, sep, Fa, Fb, iters)
            assert ld.n_iters == r64.n_iters == sc.n_iters == iters
            vr.check_result(sc, ld, r64, f"T = {T}, S = {S}, sep = {sep}, Fa = {Fa}, {iters} iterations")
            assert np.array_equal(sc.labels, ld.labels) or vr.top_two_margin(ld.gamma) < 1e-6


@pytest.mark.parametrize("T,S", SHAPES)
def test_float32_emissions_are_far_outside_the_gates(T, S):
    """The yardstick sees what it is for: with the emission product in float32 gamma and the ELBO land more than ten times
    above the gates (measured: gamma 52 .. 1e4 rms units, the ELBO above 1e4)."""
    x, psi, lab, _ = vr.make_problem(SEED + 31 * T + S, T, S, 128, 0.25)
    g0 = vr.gamma_from_labels(lab, S)
    ld, r64, _ = twins(T, S, 0.25, 0.3, 17.0, 1)
    real = vr._models

    def models32(x_, rho, psi_, gamma, Fa, Fb, G, dt):
        ll, kl = real(x_, rho, psi_, gamma, Fa, Fb, G, dt)
        r = dt(Fa) / dt(Fb)
        invL = 1 / (1 + r * gamma.sum(axis=0)[:, None] * psi_[None, :])
        alpha = r * invL * (gamma.T @ rho)
        dot32 = (rho.astype(np.float32) @ alpha.T.astype(np.float32)).astype(dt)
        return ll + dt(Fa) * (dot32 - rho @ alpha.T), kl

    vr._models = models32
    try:
        bad = vr.vbhmm(x, psi, g0, max_iters=1, eps=-np.inf)
    finally:
        vr._models = real
    if S > 1 and T > 17:
        assert vr.units(bad.gamma, ld.gamma, r64.gamma)[0] > 10.0 * vr.RMS_MAX
    assert vr.units(bad.elbo[:1], ld.elbo[:1], r64.elbo[:1])[1] > 10.0 * vr.MAX_MAX


@pytest.mark.parametrize("T,S", SHAPES)
def test_elbo_trace_of_the_twin_does_not_decrease(T, S):
    """No decrease larger than the twin's own float64-vs-longdouble ELBO error, on these inputs.  Once a run has converged
    the float64 trace moves by a few ulps up and down while the longdouble trace still rises (its largest decrease over all
    of these runs is 1e-14): a drop is then the difference of two rounding errors, each at most the error it is compared
    with.  Of the seed bases 0, 100 .. 600, four (200, 400, 500, 600) keep every drop below that error (the largest at 0.56,
    0.67, 0.42, 0.94 of it) and three do not (a drop of up to 1.6 times the error, at T = 17 and T = 65); SEED is the first
    of the four."""
    for sep in (0.1, 0.25):
        for Fa, Fb in ((0.3, 17.0), (1.0, 1.0)):
            ld, r64, _ = twins(T, S, sep, Fa, Fb, 40)
            err = float(np.abs(r64.elbo - ld.elbo).max())
            drop = float(-np.diff(np.asarray(r64.elbo, np.float64)).min())
            assert drop <= err, (sep, Fa, drop, err)


def test_over_clustered_separable_speakers_are_recovered():
    T, K, S = 300, 4, 7
    x, psi, lab, truth = vr.make_problem(12, T, S, 128, 8.0, K=K)
    assert np.unique(lab).size == S
    r = vr.vbhmm(x, psi, vr.gamma_from_labels(lab, S))
    assert r.n_speakers == K and np.unique(r.labels).tolist() == list(range(K))
    assert len({(int(a), int(b)) for a, b in zip(r.labels, truth)}) == K          # one to one with the true speakers
    assert 2 <= r.n_iters < 40 and np.isnan(r.elbo[r.n_iters:]).all()
    sc = vr.vbhmm_scaled(x, psi, vr.gamma_from_labels(lab, S))
    assert np.array_equal(sc.labels, r.labels) and sc.n_iters == r.n_iters


def test_helpers():
    g = vr.gamma_from_labels(np.array([0, 2, -1, 3]), 3, 5.0)
    hi = np.exp(5.0) / (np.exp(5.0) + 2)
    assert np.allclose(g[0], [hi, (1 - hi) / 2, (1 - hi) / 2]) and np.argmax(g[1]) == 2
    assert np.array_equal(g[2], np.full(3, 1 / 3)) and np.array_equal(g[3], np.full(3, 1 / 3))
    lab, n = vr.hard_labels(np.array([[0.1, 0.1, 0.8], [0.4, 0.4, 0.2], [0.0, 0.2, 0.8]]))
    assert lab.tolist() == [1, 0, 1] and n == 2                                   # ties: the lowest s; dense ranks
    assert vr.units(np.array([1.0 + 2.0 ** -52]), np.array([1.0], np.longdouble), np.array([1.0])) == (2.0, 2.0)
    eps, n = vr.pick_epsilon(np.cumsum([0.0, 100.0, 10.0, 1.0, 0.9, 1e-9]))
    assert abs(eps - np.sqrt(10.0)) < 1e-9 and n == 4


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

NAMES = ["nplda_vbhmm_max_speakers", "nplda_vbhmm_max_iters", "nplda_vbhmm_block", "nplda_vbhmm_workspace_bytes", "nplda_vbhmm_f64"]


def test_declared_names_are_present(hip_lib):
    from neuralplda_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(hip_lib, n) and re.search(r"\b%s\(" % n, hdr), n
    assert hip_lib.nplda_abi_version() == 4
    assert hip_lib.nplda_vbhmm_max_speakers() == 64 and hip_lib.nplda_vbhmm_max_iters() == 256
    assert hip_lib.nplda_vbhmm_block() % 64 == 0 and 128 <= hip_lib.nplda_vbhmm_block() <= 1024


def _offs(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_abi_sizes_and_argument_checks(hip_lib):
    EINVAL, EUNSUP, ENOSPC = -22, -95, -28
    L = hip_lib
    dummy = ctypes.create_string_buffer(4096)
    p16 = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40
    rows, slots = _offs(0, 0, 5, 6, 6, 16), _offs(0, 2, 5, 6, 6, 70)
    maxn, maxd = L.nplda_ahc_max_n(), L.nplda_max_dim()
    need = L.nplda_vbhmm_workspace_bytes(rows, slots, 5, 150)
    assert need >= 8 * 3 * (5 * 3 + 1 * 1 + 10 * 64) and need % 256 == 0
    assert L.nplda_vbhmm_workspace_bytes(_offs(0), _offs(0), 0, 150) > 0
    assert L.nplda_vbhmm_workspace_bytes(_offs(0, 0), _offs(0, 0), 1, 150) % 256 == 0 < L.nplda_vbhmm_workspace_bytes(_offs(0, 0), _offs(0, 0), 1, 150)
    assert L.nplda_vbhmm_workspace_bytes(_offs(0, maxn), _offs(0, 64), 1, maxd) >= 8 * 3 * maxn * 64
    for r, s, P, D in ((_offs(0, 5, 4), _offs(0, 1, 2), 2, 150), (_offs(1, 5), _offs(0, 1), 1, 150), (_offs(0, 5), _offs(1, 2), 1, 150),
                       (_offs(0, 5), _offs(0, 0), 1, 150), (_offs(0, 5), _offs(3, 2), 1, 150), (_offs(0, maxn + 1), _offs(0, 2), 1, 150),
                       (_offs(0, 5), _offs(0, 65), 1, 150), (rows, slots, -1, 150), (rows, slots, 5, 0), (rows, slots, 5, maxd + 1),
                       (None, slots, 5, 150), (rows, None, 5, 150)):
        assert L.nplda_vbhmm_workspace_bytes(r, s, P, D) == 0

    def vb(z=p16, ldz=160, oh=rows, od=p16, sh=slots, sd=p16, P=5, D2=150, psi=p16, lab=p16, gi=None, pi0=None, Fa=0.3, Fb=17.0,
           loop=0.99, eps=1e-4, smooth=5.0, iters=40, gamma=p16, pi=p16, elbo=p16, ni=p16, labels=p16, ns=p16, ws=p16, wsb=big):
        return L.nplda_vbhmm_f64(z, ldz, oh, od, sh, sd, P, D2, psi, lab, gi, pi0, Fa, Fb, loop, eps, smooth, iters, gamma, pi, elbo,
                                 ni, labels, ns, ws, wsb, None)

    none = dict(z=None, oh=None, od=None, sh=None, sd=None, psi=None, lab=None, gamma=None, pi=None, elbo=None, ni=None, labels=None,
                ns=None, ws=None)
    assert vb(P=0) == 0 and vb(P=0, **none) == 0
    for k in none:
        if k != "lab":
            assert vb(**{k: None}) == EINVAL, k
    assert vb(lab=None) == EINVAL and vb(gi=p16) == EINVAL and vb(lab=None, gi=None) == EINVAL     # both or neither initialiser
    nan, inf = float("nan"), float("inf")
    for kw in (dict(eps=nan), dict(Fa=0.0), dict(Fa=-1.0), dict(Fa=nan), dict(Fb=0.0), dict(Fb=nan), dict(loop=1.0), dict(loop=-0.01),
               dict(loop=nan), dict(smooth=-1.0), dict(smooth=nan), dict(iters=0), dict(iters=-2), dict(P=-1), dict(D2=0),
               dict(oh=_offs(0, 5, 4), sh=_offs(0, 1, 2), P=2), dict(oh=_offs(2, 5), sh=_offs(0, 1), P=1),
               dict(oh=_offs(0, 5), sh=_offs(0, 0), P=1), dict(oh=_offs(0, 5), sh=_offs(3, 2), P=1), dict(ldz=149), dict(ldz=162)):
        assert vb(**kw) == EINVAL, kw
    for kw in (dict(z=p16 + 4), dict(ws=p16 + 8), dict(psi=p16 + 4), dict(gamma=p16 + 4), dict(pi=p16 + 4), dict(elbo=p16 + 4),
               dict(pi0=p16 + 4), dict(lab=None, gi=p16 + 4), dict(lab=p16 + 2), dict(ni=p16 + 2), dict(labels=p16 + 2),
               dict(ns=p16 + 2), dict(od=p16 + 4), dict(sd=p16 + 4)):
        assert vb(**kw) == EINVAL, kw
    assert vb(eps=-inf, wsb=0) == ENOSPC and vb(eps=inf, wsb=need - 1) == ENOSPC
    for kw in (dict(oh=_offs(0, 5), sh=_offs(0, 65), P=1), dict(iters=257), dict(oh=_offs(0, maxn + 1), sh=_offs(0, 2), P=1),
               dict(D2=maxd + 1, ldz=maxd + 16), dict(P=1 << 22)):
        assert vb(**kw) == EUNSUP, kw
    assert vb(lab=None, gi=p16, wsb=0) == ENOSPC and vb(pi0=p16, wsb=0) == ENOSPC     # every check but the last passed


# ---- kernel resources --------------------------------------------------------------------------------------------------------------

def test_resource_budget_of_the_vbhmm_kernel():
    """design/k22_vbhmm.md: one kernel, no scratch; a workgroup of 512 threads is eight waves, two per SIMD, so a thread may
    hold up to 256 registers and one workgroup is resident per CU; LDS holds a tile of 32 rows (24 KB of float32 features,
    16 KB of float64 posteriors), psi, sqrt(psi), five per-speaker vectors and the reduction slots: 46 KB of 160."""
    res = _resources("nplda_vbhmm.hip")
    assert len(res) == 1 and "vbhmm_kernel" in next(iter(res)), sorted(res)
    for name, v in res.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256 and v["LDS"] <= 48 * 1024, (name, v)
