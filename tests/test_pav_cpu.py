"""PAV / ROC convex hull without a GPU: the yardstick of the GPU tests (tests/pav_ref.py) against two unrelated
formulations, the declared ABI, the workspace size, every status code of the nplda_pav_* entry points (returned before
anything is enqueued: no valid call is made), and the host replay of the hull's merge tree (tests/c/pav_core_host.cpp,
which shares csrc/nplda_pav_core.h with the kernels) under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from neuralplda_amd import _lib

from tests import pav_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENOSPC = -22, -95, -28
NAMES = ["nplda_pav_chunk", "nplda_pav_workspace_bytes", "nplda_pav_fit_f32", "nplda_pav_fit_f64", "nplda_pav_fit_stages_f32", "nplda_pav_apply_f32",
         "nplda_pav_apply_f64"]


# ---- the reference ------------------------------------------------------------------------------------------------------
def _minmax(n, t):
    """p_k = max_{a <= k} min_{b >= k} mean(a .. b), by brute force in exact rationals."""
    from fractions import Fraction
    M = len(n)
    cn = np.concatenate(([0], np.cumsum(n))).tolist()
    ct = np.concatenate(([0], np.cumsum(t))).tolist()
    mean = lambda a, b: Fraction(ct[b + 1] - ct[a], cn[b + 1] - cn[a])  # noqa: E731
    return [max(min(mean(a, b) for b in range(k, M)) for a in range(k + 1)) for k in range(M)]


@pytest.mark.parametrize("seed", range(40))
def test_reference_against_the_min_max_formula(seed):
    rg = np.random.default_rng(seed)
    N = int(rg.integers(2, 25))
    s = rg.choice(np.array([-2.0, -0.5, -0.0, 0.0, 1.0, 3.5]), size=N)  # six values, of which two are equal: heavy ties
    y = (rg.random(N) < 0.4).astype(np.float64)
    p, n, t = pr.fitted_values(s, y)
    want = _minmax(n.tolist(), t.tolist())
    from fractions import Fraction
    v = pr.hull(n, t)
    cn = np.concatenate(([0], np.cumsum(n))).tolist()
    ct = np.concatenate(([0], np.cumsum(t))).tolist()
    got = [None] * len(n)
    for b in range(len(v) - 1):
        for k in range(v[b], v[b + 1]):
            got[k] = Fraction(ct[v[b + 1]] - ct[v[b]], cn[v[b + 1]] - cn[v[b]])
    assert got == want
    slopes = [got[v[b]] for b in range(len(v) - 1)]
    assert all(a < b for a, b in zip(slopes, slopes[1:]))  # strict hull: p_b strictly increasing
    assert np.array_equal(p, np.array([float(x) for x in want]))


@pytest.mark.parametrize("seed,N,levels", [(0, 50, 6), (1, 300, 16), (2, 2000, 0), (3, 2000, 3), (4, 5, 2)])
def test_reference_against_scipy_isotonic_regression(seed, N, levels):
    import scipy.optimize
    rg = np.random.default_rng(seed)
    y = (rg.random(N) < 0.3).astype(np.float64)
    s = rg.standard_normal(N) + 1.5 * y
    if levels:
        s = np.round(s * levels / 4.0)
    p, n, t = pr.fitted_values(s, y)
    r = scipy.optimize.isotonic_regression(t / n, weights=n.astype(np.float64))
    assert np.abs(p - r.x).max() <= 1e-12  # values, not blocks: equal-mean pooling conventions do not matter


def test_reference_metrics_on_cases_done_by_hand():
    # perfectly separated: two blocks, p = 0 and 1: min Cllr 0, EER 0
    f = pr.fit([0.0, 1.0, 2.0, 3.0], [0, 0, 1, 1], laplace=False)
    assert f["nb"] == 2 and f["n"].tolist() == [2, 2] and f["t"].tolist() == [0, 2]
    assert f["min_cllr"] == 0.0 and f["rocch_eer"] == 0.0 and f["llr"].tolist() == [-np.inf, np.inf]
    # perfectly inverted: one block at the prior: min Cllr 1 bit, EER 1/2
    f = pr.fit([0.0, 1.0, 2.0, 3.0], [1, 1, 0, 0], laplace=False)
    assert f["nb"] == 1 and abs(f["min_cllr"] - 1.0) <= 1e-15 and abs(f["rocch_eer"] - 0.5) <= 1e-15 and f["llr"][0] == 0.0
    # Laplace: dummy bins alone at both ends when the data start with a non-target and end with a target
    f = pr.fit([0.0, 1.0, 2.0, 3.0], [0, 0, 1, 1], laplace=True)
    assert f["n"].tolist() == [4, 4] and f["t"].tolist() == [1, 3] and f["lo"].tolist() == [0.0, 2.0]
    f = pr.fit([0.0, 1.0, 2.0, 3.0], [1, 1, 0, 0], laplace=True)
    assert f["nb"] == 1 and f["lo"][0] == 0.0 and f["hi"][0] == 3.0
    f = pr.fit([0.0, 0.0, 1.0, 5.0, 5.0], [1, 1, 0, 0, 0], laplace=True)  # 2/2 | 1/2 dummy... the dummy bin (1/2) pools
    assert f["t"].sum() == 4 and f["n"].sum() == 9
    # excluded trials and NaN scores do not count
    f = pr.fit([0.0, np.nan, 1.0, 2.0, 7.0], [0, 1, 0.5, 1, np.nan], laplace=False)
    assert (f["N_t"], f["N_n"], f["M"]) == (1, 1, 2)
    # the map: inside, gaps, ends, NaN
    lo, hi, llr = np.array([0.0, 2.0]), np.array([1.0, 3.0]), np.array([-1.0, 1.0])
    got = pr.apply(lo, hi, llr, [-5.0, 0.0, 0.5, 1.0, 1.5, 1.75, 2.0, 3.0, 9.0, np.nan, -np.inf, np.inf])
    assert np.array_equal(got[:9], [-1.0, -1.0, -1.0, -1.0, 0.0, 0.5, 1.0, 1.0, 1.0]) and np.isnan(got[9])
    assert got[10] == -1.0 and got[11] == 1.0
    lo, hi, llr = np.array([-np.inf, 0.0, np.inf]), np.array([-np.inf, 1.0, np.inf]), np.array([-2.0, 0.0, 2.0])
    assert pr.apply(lo, hi, llr, [-np.inf, -7.0, 0.5, 7.0, np.inf]).tolist() == [-2.0, -2.0, 0.0, 2.0, 2.0]


# ---- the library --------------------------------------------------------------------------------------------------------
def test_declared_names(hip_lib):
    assert hip_lib.nplda_abi_version() == 4
    with open(os.path.join(ROOT, "include", "nplda_hip.h")) as fh:
        hdr = fh.read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None, name
    from neuralplda_amd import metrics, ops, score_calibration
    for mod, fns in ((ops, ("pav_fit", "pav_apply", "pav_chunk")), (metrics, ("min_cllr", "rocch_eer", "rocch")),
                     (score_calibration, ("fit_pav", "PavCalibration"))):
        for fn in fns:
            assert callable(getattr(mod, fn)), fn
    assert hip_lib.nplda_pav_chunk() >= 2
    with pytest.raises(ValueError):
        score_calibration.calibrate_scorefile("a", "b", "c", method="isotonic")


def test_workspace_bytes(hip_lib):
    f = hip_lib.nplda_pav_workspace_bytes
    C = hip_lib.nplda_pav_chunk()
    ns = [2, 3, C - 1, C, C + 1, 2 * C + 1, 4099, 1 << 20, 10_000_000, 2 ** 31 - 1]
    ns = sorted(n for n in ns if n >= 2)
    for is64 in (0, 1):
        sizes = [f(n, is64) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
        for n in (1, 0, -5, 2 ** 31, 2 ** 40):
            assert f(n, is64) == 0, n
    assert f(1000, 1) >= f(1000, 0)


def _host():
    buf = np.zeros(4096, dtype=np.float64)
    return buf, buf.ctypes.data


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_status_codes_of_fit(hip_lib, p):
    buf, a = _host()
    N = 100
    ws = hip_lib.nplda_pav_workspace_bytes(N, int(p == "f64"))
    fit = getattr(hip_lib, "nplda_pav_fit_" + p)

    def call(s=a, t=a, N=N, lap=1, lo=a, hi=a, n=a, tt=a, llr=a, cap=16, summ=a, w=a, wb=ws):
        return fit(s, t, N, lap, lo, hi, n, tt, llr, cap, summ, w, wb, None)

    for name in ("s", "t", "lo", "hi", "n", "tt", "llr", "summ", "w"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("lo", "hi", "n", "tt", "llr", "summ"):
        assert call(**{name: a + 4}) == EINVAL, name  # not aligned to 8 bytes
    assert call(w=a + 8) == EINVAL and call(s=a + 2) == EINVAL and call(t=a + 2) == EINVAL
    assert call(N=1) == EINVAL and call(N=0) == EINVAL and call(N=-3) == EINVAL and call(cap=0) == EINVAL
    assert call(N=2 ** 31) == EUNSUPPORTED
    assert call(wb=ws - 1) == ENOSPC and call(wb=0) == ENOSPC


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_status_codes_of_apply(hip_lib, p):
    buf, a = _host()
    app = getattr(hip_lib, "nplda_pav_apply_" + p)

    def call(s=a, N=100, lo=a, hi=a, llr=a, nb=3, out=a, f64=1):
        return app(s, N, lo, hi, llr, nb, out, f64, None)

    for name in ("s", "lo", "hi", "llr", "out"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("lo", "hi", "llr", "out"):
        assert call(**{name: a + 4}) == EINVAL, name
    assert call(s=a + 2) == EINVAL and call(out=a + 2, f64=0) == EINVAL
    assert call(N=-1) == EINVAL and call(nb=0) == EINVAL and call(nb=-2) == EINVAL
    assert call(N=2 ** 31) == EUNSUPPORTED and call(nb=2 ** 31) == EUNSUPPORTED
    assert call(N=0) == 0  # nothing to do, nothing launched


# ---- the merge tree on the host -----------------------------------------------------------------------------------------
def test_merge_tree_replay_on_the_host_under_sanitizers(tmp_path):
    """tests/c/pav_core_host.cpp: flags, chunk scans and every merge level with C = 2, 3, 4, 8 and N = 1 .. 200 over all
    families, vertex lists against the O(n) stack.  Built with -fsanitize=address,undefined when the runtime is there."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cxx), "no host C++ compiler (not even the hipcc that builds the library)"
    src = os.path.join(ROOT, "tests", "c", "pav_core_host.cpp")
    exe = str(tmp_path / "pav_core_host")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:  # no sanitizer runtime on this machine
        r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert re.search(r"\b\d+ cases, 0 failures", run.stdout), run.stdout[-500:]
