"""The training-mode forward and the generic template instances in units of an fp32 computation (tests/fp32_units.py).

nplda_forward_train_f32 and nplda_embed_train_f32 — nplda_fwd_small_kernel<NB, MODE_TRAIN / MODE_EMBED> up to 16 384 units,
nplda_fwd_v2_kernel above — with every saved activation (s, y, z, rn; both halves) measured on its own against the fp64
oracle, the float32 oracle as the unit, over all rows and per tile region; the pad columns exactly zero; nothing written past
the batch.  Shapes (tests/fwd_chain_ref.py: SHAPES) are the smallest that reach each instance (NB = 2, 4, 8, 10, 11, 12), D1 !=
D2, the run-time K loop with a ragged last k16-step or fewer steps than its prefetch ring, and the K-split instances.  The
scoring side (score_pairs, embed) of the same shapes follows at the end.

Bounds: fp32_units.RMS_MAX / MAX_MAX = 3 / 5 for every case.  A case could take more only where the chain-order reference's
own ratio, measured on the CPU by tests/test_fwd_chain_ref_cpu.py, exceeded 2 / 3.3 (fwd_bound there); none does: with one
rounding per MFMA it stays <= 1.50 / 1.65 (s) and <= 1.02 / 1.10 (y, z), and even with one rounding per product <= 1.82 / 2.52
(s) and <= 1.55 / 1.89 (y, z).

Batches of 1 .. 17 pairs are launched many times on different rows and the rows pooled, and the oracle runs ONCE on the pooled
rows: a ratio over a handful of values is a draw, and numpy's float32 matmul takes another BLAS path for <= 6 - 8 rows, whose
error — the unit — is 2.3 - 3.1 x smaller (tests/test_fwd_chain_ref_cpu.py::test_unit_shrinks_for_tiny_oracle_batches).  The
kernel's rows do not depend on the batch they arrive in; the unit must not either.

Measured on MI355X: see the figures next to each case table.
"""
import types

import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc
from tests import fp32_units as fu
from tests import fwd_chain_ref as fcr
from tests.test_forward_gpu import rand_params, to_dev
from tests.test_fwd_chain_ref_cpu import fwd_bound

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0   # finite, and ~1e4 x any value the forward produces
PAD_ROWS = 40        # sentinel rows behind every output (more than a 16-row tile; v2 clamps rows the same way)
UNITS_MAX = 256 * 64  # csrc/nplda_fwd_dispatch.h: launch_fwd_old sends up to this many units to the small-batch kernel
MID, SMALL = "nplda_fwd_mid_kernel", "nplda_fwd_small_kernel"
V3, V5, V6 = "nplda_fwd_v3_kernel", "nplda_fwd_v5_kernel", "nplda_fwd_v6_kernel"


def _model(shape):
    from neuralplda_amd import ops
    p = rand_params(np.random.default_rng(sum(shape)), *shape)
    return p, ops.pack_params(*to_dev(p))


def _randn(n, D0, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, D0, device="cuda", generator=gen)


def _full(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def forward_train_sentinel(x1, x2, packed, B, reps):
    """nplda_forward_train_f32 on rows [r B, (r + 1) B) of x1 / x2 for r < reps, each launch into its own slab of buffers
    pre-filled with a sentinel (ops.forward_train hands the kernel torch.empty: an unwritten element could hold anything).
    Returns s (reps, B), y, z (reps, 2 B, ldz), rn (reps, 2 B) after checking that no launch wrote behind its 2 B rows."""
    from neuralplda_amd import _lib
    lib = _lib.load()
    ldz = packed.ldz
    s, rn = _full(reps, B + PAD_ROWS), _full(reps, 2 * B + PAD_ROWS)
    y, z = _full(reps, 2 * B + PAD_ROWS, ldz), _full(reps, 2 * B + PAD_ROWS, ldz)
    with _lib.on_device(x1.device):
        for r in range(reps):
            a, b = x1[r * B:(r + 1) * B], x2[r * B:(r + 1) * B]
            code = lib.nplda_forward_train_f32(_lib.ptr(a), _lib.ptr(b), B, x1.stride(0), _lib.ptr(packed.buf), packed.D0,
                                               packed.D1, packed.D2, _lib.ptr(s[r]), _lib.ptr(y[r]), _lib.ptr(z[r]),
                                               _lib.ptr(rn[r]), ldz, _lib.current_stream())
            _lib.check(code, "nplda_forward_train_f32")
    for name, t, n in (("s", s, B), ("y", y, 2 * B), ("z", z, 2 * B), ("rn", rn, 2 * B)):
        assert bool((t[:, n:] == SENTINEL).all()), f"{name}: rows past the batch were written"
        assert bool((t[:, :n] != SENTINEL).all()), f"{name}: elements of the batch were not written"
    return s[:, :B], y[:, :2 * B], z[:, :2 * B], rn[:, :2 * B]


def embed_train_sentinel(x, packed):
    from neuralplda_amd import _lib
    lib = _lib.load()
    N, ldz = x.shape[0], packed.ldz
    z, y, rn = _full(N + PAD_ROWS, ldz), _full(N + PAD_ROWS, ldz), _full(N + PAD_ROWS)
    with _lib.on_device(x.device):
        code = lib.nplda_embed_train_f32(_lib.ptr(x), N, x.stride(0), _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2,
                                         _lib.ptr(z), _lib.ptr(y), _lib.ptr(rn), ldz, _lib.current_stream())
    _lib.check(code, "nplda_embed_train_f32")
    for name, t in (("z", z), ("y", y), ("rn", rn)):
        assert bool((t[N:] == SENTINEL).all()), f"{name}: rows past the batch were written"
        assert bool((t[:N] != SENTINEL).all()), f"{name}: elements of the batch were not written"
    return z[:N], y[:N], rn[:N]


def _check(results, got, r64, r32, what, reg, shape, kernel, output):
    """Measure, print, remember; the assertions come after every figure of the case is out (_assert_all)."""
    rms_max, max_max = fwd_bound(shape, kernel, output)
    r = fu.measure(got, r64, r32, reg)
    print(f"{what}: " + "  ".join(f"{k} {v[0]:.2f} / {v[1]:.2f}" for k, v in r.items()))
    results.append((what, r, rms_max, max_max))


def _assert_all(results):
    bad = {w: {k: v for k, v in r.items() if not (v[0] <= a and v[1] <= b)} for w, r, a, b in results}
    bad = {w: v for w, v in bad.items() if v}
    assert not bad, f"above the bound in fp32 units (rms, max): {bad}"


def _pooled_regions(B, reps):
    """Row sets of `reps` pooled launches of B pairs (row r B + i is pair i of launch r): the full tiles, the ragged tile."""
    i = np.tile(np.arange(B), reps)
    pos = {}
    if B > 16 and B % 16:
        pos["full tiles"] = np.flatnonzero(i < B // 16 * 16)
        pos["ragged last tile"] = np.flatnonzero(i >= B // 16 * 16)
    return types.SimpleNamespace(pos=pos)


def _train_case(shape, B, kernel):
    D0, D1, D2 = shape
    p, packed = _model(shape)
    pooled = B <= 17
    reps = -(-512 // B) if pooled else 1
    x1, x2 = _randn(reps * B, D0, 3 * B + D0), _randn(reps * B, D0, 3 * B + D0 + 1)
    s, y, z, rn = forward_train_sentinel(x1, x2, packed, B, reps)
    assert bool((y[:, :, D1:] == 0).all()) and bool((z[:, :, D2:] == 0).all()), "pad columns are not exactly zero"
    if pooled:
        reg, idx = _pooled_regions(B, reps), np.arange(reps * B)
    else:
        reg = fu.Regions(B, 16 if kernel == fcr.SMALL else 128, seed=B)
        idx = reg.idx
    sel = torch.from_numpy(idx).cuda()
    a, b = x1[sel].cpu().numpy(), x2[sel].cpu().numpy()
    r64, r32 = fcr.oracle_outputs(a, b, p, np.float64), fcr.oracle_outputs(a, b, p, np.float32)
    n = len(idx)
    halves = lambda t, D: (t[:, :B].reshape(reps * B, -1)[sel][:, :D].cpu().numpy(),  # noqa: E731
                           t[:, B:].reshape(reps * B, -1)[sel][:, :D].cpu().numpy())
    got = dict(s=(s.reshape(-1)[sel].cpu().numpy(),), y=halves(y, D1), z=halves(z, D2),
               rn=tuple(h[:, 0] for h in halves(rn.unsqueeze(-1), 1)))
    results = []
    for out in fcr.OUTPUTS:
        for h, g in enumerate(got[out]):
            lo = h * n
            what = f"forward_train {kernel} {shape} B={B} {out}{h + 1 if out != 's' else ''}"
            _check(results, g, r64[out][lo:lo + n], r32[out][lo:lo + n], what, reg, shape, kernel, out)
    _assert_all(results)


# forward_train, small-batch kernel (B <= 16 384): a single pair, the TINY_B sizes of tests/test_fp32_units_grad_gpu.py, a
# ragged 16-pair tile, many tiles with a ragged last.
# Measured on MI355X, worst rms / max over shapes, batch sizes, halves and regions: s 1.61 / 2.41, y 1.42 / 2.08,
# z 1.53 / 2.54, rn 1.24 / 2.00 (the chain reference with one rounding per product: s 1.82 / 2.52, y 1.41 / 1.89, z 1.55 / 1.85, rn
# 1.14 / 1.43).  Shape by shape the kernel sits on that reference: y / z 1.40 / 1.50 at (500, 150, 160), 1.00 / 1.25 at
# (400, 180, 192) and, for the K-split instances, 0.74 / 1.18 at (512, 150, 150) — at B = 3 and B = 8 as at B = 1003.
@pytest.mark.parametrize("B", [1, 3, 8, 17, 1003])
@pytest.mark.parametrize("shape", fcr.SHAPES)
def test_forward_train_small_kernel(hip_lib, shape, B):
    _train_case(shape, B, fcr.SMALL)


# forward_train, v2 kernel: just above the boundary, the last 128-pair block ragged (16 384 + 77 = 128 x 128 + 77).
# Measured on MI355X, worst rms / max: s 1.84 / 2.53, y 1.42 / 2.15, z 1.55 / 1.90, rn 1.24 / 1.80 (y / z at (512, 150, 150): 1.40 /
# 1.51, the 128-step chain the small-batch kernel's K-split avoids).
V2_SHAPES = [(512, 150, 150), (512, 170, 170), (512, 170, 150), (512, 192, 192), (500, 150, 160), (400, 180, 192)]


@pytest.mark.parametrize("shape", V2_SHAPES)
def test_forward_train_v2_kernel(hip_lib, shape):
    _train_case(shape, UNITS_MAX + 77, fcr.V2)


# embed_train: U = (N + 1) / 2 units of 32 rows.  N = 37: one ragged second tile; 32 767: U = 16 384, the small-batch kernel's
# last size, N odd (the last tile's second half one row short); 32 769: U = 16 385, v2 (256 rows per block), N odd.
# Measured on MI355X, worst rms / max: small-batch kernel z 1.55 / 2.04, y 1.44 / 2.21, rn 1.21 / 1.72; v2 z 1.55 / 2.01,
# y 1.41 / 2.31, rn 1.22 / 1.89.
@pytest.mark.parametrize("N,kernel", [(37, fcr.SMALL), (2 * UNITS_MAX - 1, fcr.SMALL), (2 * UNITS_MAX + 1, fcr.V2)])
@pytest.mark.parametrize("shape", fcr.SHAPES)
def test_embed_train(hip_lib, shape, N, kernel):
    D0, D1, D2 = shape
    assert ((N + 1) // 2 <= UNITS_MAX) == (kernel == fcr.SMALL)
    p, packed = _model(shape)
    x = _randn(N, D0, N + D0)
    z, y, rn = embed_train_sentinel(x, packed)
    assert bool((y[:, D1:] == 0).all()) and bool((z[:, D2:] == 0).all()), "pad columns are not exactly zero"
    reg = fu.Regions(N, 32 if kernel == fcr.SMALL else 256, seed=N)
    sel = torch.from_numpy(reg.idx).cuda()
    xr = x[sel].cpu().numpy()
    r64, r32 = fcr.oracle_outputs(xr, xr[:0], p, np.float64), fcr.oracle_outputs(xr, xr[:0], p, np.float32)
    got = dict(z=z[sel][:, :D2], y=y[sel][:, :D1], rn=rn[sel])
    results = []
    for out in ("z", "y", "rn"):
        _check(results, got[out].cpu().numpy(), r64[out], r32[out], f"embed_train {kernel} {shape} N={N} {out}", reg, shape,
               kernel, out)
    _assert_all(results)


# ---- the scoring side of the same shapes ---------------------------------------------------------------------------------
# The kernel each shape takes on a 256-CU device (nplda_score_pairs_kernel_name; csrc/nplda_fwd_dispatch.h): at B = 1000 the
# small-batch kernel, the balanced-tile kernel for 512-d x-vectors at NB = 10 / 11; at B = 20 037 the streaming kernel — v3 up
# to NB = 10, v6 at D1 = D2 = 150, v5 at NB = 12 — and again the balanced-tile kernel where it applies.
def _pair_kernels(shape):
    D0, D1, D2 = shape
    NB = fcr.kernel_nb(D1, D2)
    if D0 == 512 and NB in (10, 11):
        return MID, MID
    return SMALL, V6 if (D1, D2) == (150, 150) else (V3 if NB <= 10 else V5)


# Measured on MI355X, worst rms / max: small 1.48 / 1.75, mid 1.34 / 1.65, v3 1.78 / 2.35, v5 1.90 / 2.10, v6 1.53 / 2.06.
@pytest.mark.parametrize("B", [1000, 20037])
@pytest.mark.parametrize("shape", fcr.SHAPES)
def test_score_pairs(hip_lib, shape, B):
    from neuralplda_amd import _lib, ops
    D0, D1, D2 = shape
    want = _pair_kernels(shape)[B > 1000]
    name = _lib.load().nplda_score_pairs_kernel_name(B, D0, D1, D2).decode()
    assert name.startswith(want), (shape, B, name)
    p, packed = _model(shape)
    x1, x2 = _randn(B, D0, B + D0), _randn(B, D0, B + D0 + 1)
    s = ops.score_pairs(x1, x2, packed)
    reg = fu.Regions(B, 128 if want in (V3, V5, V6) else 16, seed=B)
    sel = torch.from_numpy(reg.idx).cuda()
    a, b = x1[sel].cpu().numpy(), x2[sel].cpu().numpy()
    results = []
    _check(results, s[sel].cpu().numpy(), orc.forward(a, b, p, np.float64), orc.forward(a, b, p, np.float32),
           f"score_pairs {want} {shape} B={B}", reg, shape, fcr.V2 if B > 1000 else fcr.SMALL, "s")
    _assert_all(results)


# embed (no saved activations): N = 2000 -> 1000 units, N = 40 074 -> 20 037 units (v2 in MODE_EMBED, or the balanced-tile
# kernel where the pair dispatch picks it for that many units).  Measured on MI355X, worst rms / max: z 1.52 / 2.11, q 1.68 / 2.06.
@pytest.mark.parametrize("N", [2000, 40074])
@pytest.mark.parametrize("shape", fcr.SHAPES)
def test_embed(hip_lib, shape, N):
    from neuralplda_amd import ops
    D0, D1, D2 = shape
    p, packed = _model(shape)
    x = _randn(N, D0, N + D0)
    z, q = ops.embed(x, packed)
    assert bool((z[:, D2:] == 0).all()), "pad columns are not exactly zero"
    mid = _pair_kernels(shape)[0] == MID
    reg = fu.Regions(N, 16 if mid else (32 if N == 2000 else 256), seed=N)
    sel = torch.from_numpy(reg.idx).cuda()
    xr = x[sel].cpu().numpy()
    z64, z32 = orc.extract_plda_embeddings(xr, p, np.float64), orc.extract_plda_embeddings(xr, p, np.float32)
    results = []
    kernel = fcr.SMALL if N == 2000 else fcr.V2
    _check(results, z[sel][:, :D2].cpu().numpy(), z64, z32, f"embed {shape} N={N} z", reg, shape, kernel, "z")
    _check(results, q[sel].cpu().numpy(), orc.self_term(z64, p, np.float64), orc.self_term(z32, p, np.float32),
           f"embed {shape} N={N} q", reg, shape, kernel, "s")
    _assert_all(results)
