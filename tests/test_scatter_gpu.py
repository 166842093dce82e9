"""ops.class_scatter (csrc/nplda_scatter.hip) against the float64 oracle of tests/backend_ref.py, in units of the error the
same oracle makes when it accumulates the row statistics in float32 (tests/fp32_units.py; defaults RMS_MAX / MAX_MAX).
Shapes are the smallest that reach every path of the kernels: their row-group sizes are read from the source."""
import os
import re

import numpy as np
import pytest
import torch

from neuralplda_amd import _lib, ops
from tests import backend_ref as ref
from tests import fp32_units as fu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "neuralplda_amd", "csrc", "nplda_scatter.hip")).read()
GROUP = int(re.search(r"constexpr int kGroupRows = (\d+);", _SRC).group(1))   # rows a scatter block sums in fp32
SUMROWS = int(re.search(r"constexpr int kSumRows = (\d+);", _SRC).group(1))   # positions per class-sum block
DEV = "cuda:0"


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(case, **kw):
    sm, sc, cs = ops.class_scatter(_t(case["table"]), _t(case["offs"]), rows=_t(case["rows"]), pivot=_t(case["pivot"]),
                                   n=case["n"], **kw)
    return sm.cpu().numpy(), sc.cpu().numpy(), cs.cpu().numpy()


def _oracles(case):
    x = case["table"][:, :case["n"]]
    if "ref" not in case:
        case["ref"] = (ref.class_stats(x, case["offs"], case["rows"], case["pivot"], np.float64),
                       ref.class_stats(x, case["offs"], case["rows"], case["pivot"], np.float32))
    return case["ref"]


def _check(got, case, what):
    r64, r32 = _oracles(case)
    out = {}
    for name, g, a, b in zip(("sum", "scatter", "class_sum"), got, r64, r32):
        assert g.shape == a.shape, (what, name, g.shape, a.shape)
        if g.size:
            out[name] = fu.assert_fp32_level(g, a, b, f"{what}: {name}")["all"]
    print(f"{what}: (rms, max) fp32 units {out}")
    return out


def _sizes_to_offs(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.fixture(scope="module")
def big():
    """n = 512, three row groups with a ragged last one, gathered rows with repeats out of a larger table whose padding columns
    and unnamed rows are NaN; classes of 1 .. one longer than a row group that straddles a group boundary, one empty."""
    rng = np.random.default_rng(11)
    n, ld, R = 512, 520, 3000
    N = 2 * GROUP + 452
    long_class = GROUP + 76
    sizes = [1, 2, 3, 5, 0, 17, 300, long_class]
    assert sum(sizes[:7]) < GROUP < sum(sizes)           # the long class crosses the first group boundary
    rest = N - sum(sizes)
    sizes += [rest - rest // 2, rest // 2]
    table = np.full((R, ld), np.nan, dtype=np.float32)
    rows = rng.integers(0, R // 2, N).astype(np.int64) * 2   # even rows only, with repeats; odd rows stay NaN
    assert len(np.unique(rows)) < N
    named = np.unique(rows)
    table[named, :n] = rng.standard_normal((len(named), n)).astype(np.float32)
    return {"table": table, "rows": rows, "offs": _sizes_to_offs(sizes), "pivot": None, "n": n}


@pytest.fixture(scope="module")
def far():
    """n = 152 (no multiple of the tile), rows in table order, data with mean 50 and unit spread, a pivot near the mean."""
    rng = np.random.default_rng(12)
    n, N = 152, GROUP + 276
    sizes = rng.integers(1, 40, 400)
    sizes = sizes[np.cumsum(sizes) <= N].tolist()
    sizes.append(N - sum(sizes))
    table = (50.0 + rng.standard_normal((N, n))).astype(np.float32)
    pivot = (50.0 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return {"table": table, "rows": None, "offs": _sizes_to_offs(sizes), "pivot": pivot, "n": n}


def test_gathered_rows_ragged_groups_all_class_sizes(big):
    got = _run(big)
    assert all(np.isfinite(g).all() for g in got)     # NaN padding columns and NaN unnamed rows are never read
    assert np.array_equal(got[2][4], np.zeros(512))   # the empty class
    _check(got, big, "n=512 gathered")   # MI355X: sum 0.16 / 0.12, scatter 0.39 / 0.31, class_sum 0.40 / 0.22 (rms / max)


def test_block_walks_several_row_groups(big, monkeypatch):
    """NPLDA_SCATTER_MAX_CHUNKS = 2: the first block of every tile sums two row groups into its fp64 slab, the second one."""
    f = _lib.load().nplda_class_scatter_workspace_bytes
    N, slab = int(big["offs"][-1]), 512 * 512 * 8
    three = f(N, 1, 512)
    default = _run(big)
    monkeypatch.setenv("NPLDA_SCATTER_MAX_CHUNKS", "2")
    assert three - f(N, 1, 512) == slab      # three slabs (one per row group) by default, two now
    got = _run(big)
    _check(got, big, "n=512 two groups per block")
    monkeypatch.setenv("NPLDA_SCATTER_MAX_CHUNKS", "1")
    one = _run(big)
    _check(one, big, "n=512 one chunk")
    # the same fp32 group sums added in fp64 in the same order, whoever adds them: the bits of the default plan
    for a, b, c in zip(default, got, one):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    monkeypatch.setenv("NPLDA_SCATTER_MAX_CHUNKS", "100000")   # the variable can only lower the cap
    assert f(N, 1, 512) == three


def test_identical_calls_are_bitwise_equal_and_scatter_is_symmetric(big, far):
    for case in (big, far):
        a, b = _run(case), _run(case)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert np.array_equal(a[1], a[1].T)


def test_pivot_near_the_mean_of_far_data(far):
    _check(_run(far), far, "n=152 mean 50, pivoted")   # MI355X: scatter 0.62 / 0.56; sum, class_sum 0 (exact in fp32 here)


def test_accumulate_over_two_calls(far):
    h = int(far["offs"][len(far["offs"]) // 2])          # split at a class boundary
    k = len(far["offs"]) // 2
    first = dict(far, table=far["table"][:h], offs=far["offs"][:k + 1])
    second = dict(far, table=far["table"][h:], offs=far["offs"][k:] - h)
    first.pop("ref", None), second.pop("ref", None)
    sm, sc, cs1 = ops.class_scatter(_t(first["table"]), _t(first["offs"]), pivot=_t(far["pivot"]))
    sm2, sc2, cs2 = ops.class_scatter(_t(second["table"]), _t(second["offs"]), pivot=_t(far["pivot"]), out=(sm, sc))
    assert sm2.data_ptr() == sm.data_ptr() and sc2.data_ptr() == sc.data_ptr()
    got = (sm.cpu().numpy(), sc.cpu().numpy(), torch.cat([cs1, cs2]).cpu().numpy())
    _check(got, far, "n=152 accumulated over two calls")   # MI355X: scatter 0.51 / 0.50; sum, class_sum 0


@pytest.mark.parametrize("n,N", [(4, 2 * GROUP + 452), (4, 1), (512, 1), (152, SUMROWS + 1)])
def test_one_class_small_and_single_rows(n, N):
    """S = 1, rows = NULL, pivot = NULL on zero-mean data: n = 4 (one float4 column, 256 row lanes), N = 1, and a class one row
    longer than a class-sum block."""
    rng = np.random.default_rng(100 * n + N)
    case = {"table": rng.standard_normal((N, n)).astype(np.float32), "rows": None, "offs": np.array([0, N], dtype=np.int64),
            "pivot": None, "n": n}
    # MI355X, scatter rms / max: n=4 N=2500 0.08 / 0.06 (sum 0.03 / 0.03); n=4 N=1 0.31 / 0.48; n=512 N=1 0.43 / 0.55;
    # n=152 N=513 1.00 / 1.00 (sum 0.35 / 0.25)
    _check(_run(case), case, f"n={n} N={N} one class")


def test_no_rows():
    offs = torch.zeros(4, dtype=torch.int64, device=DEV)
    table = torch.zeros((8, 8), dtype=torch.float32, device=DEV)
    sm, sc, cs = ops.class_scatter(table, offs)
    assert cs.shape == (3, 8) and not sm.any() and not sc.any() and not cs.any()
    sm.fill_(2.0), sc.fill_(3.0)
    ops.class_scatter(table, offs, out=(sm, sc))
    assert bool((sm == 2.0).all()) and bool((sc == 3.0).all())     # untouched under accumulate


def test_unsupported_arguments_return_their_status_and_write_nothing():
    lib = _lib.load()
    n, N = 8, 16
    table = torch.zeros((N + 1, 16), dtype=torch.float32, device=DEV)
    offs = torch.tensor([0, N], dtype=torch.int64, device=DEV)
    outs = [torch.full((k,), 7.0, dtype=torch.float64, device=DEV) for k in (520, 520 * 520, 520)]
    ws = torch.zeros(1 << 20, dtype=torch.float64, device=DEV)

    def call(n=n, ldt=16, tptr=table.data_ptr(), pivot=None):
        return lib.nplda_class_scatter_f32(tptr, N, ldt, None, N, offs.data_ptr(), 1, n, pivot, outs[0].data_ptr(),
                                           outs[1].data_ptr(), outs[2].data_ptr(), 0, ws.data_ptr(), ws.numel() * 8,
                                           _lib.current_stream())

    assert call(n=6) == _lib.NPLDA_EUNSUPPORTED
    assert call(n=516) == _lib.NPLDA_EUNSUPPORTED
    assert call(tptr=table.data_ptr() + 4) == -22          # misaligned table
    assert call(pivot=table.data_ptr() + 8) == -22         # misaligned pivot
    assert call(ldt=18) == -22                             # ldt % 4 != 0
    assert call(ldt=4) == -22                              # ldt < n
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not outs[0][:n].any() and bool((outs[0][n:] == 7.0).all())
    with pytest.raises(ValueError):
        ops.class_scatter(table[:, :6], offs)
    with pytest.raises(ValueError):   # an index outside the table is caught before the kernel clamps it
        ops.class_scatter(table, offs, rows=torch.full((N,), N + 1, dtype=torch.int64, device=DEV))
