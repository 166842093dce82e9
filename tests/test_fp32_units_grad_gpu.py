"""Gradient kernels in units of an fp32 computation (tests/fp32_units.py): the parameter and input gradients of every
backward path csrc/nplda_backward.hip can pick, the one-call training step, embed_backward and the score-epilogue backward,
each tensor on its own, against orc.backward / orc.input_grads / orc.embed_backward / orc.embscore_backward in fp64 with the
same functions in float32 as the unit.  Default thresholds rms_ratio <= 3, max_ratio <= 5; measured ratios next to the case
tables."""
import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc
from tests import fp32_units as fu
from tests.test_forward_gpu import rand_params, to_dev

pytestmark = pytest.mark.gpu
NAMES = ("W1", "b1", "W2", "b2", "P_sqrt", "Q")
# Batches of <= 8 pairs measure 4.5 / 5.7 (rms / max) at worst, dP_sqrt of (400, 180, 192) at B = 3, and 3.3 / 4.4 for the
# half-tile step at B = 8, where every larger batch stays <= 1.9 / 2.5.  There the layer-2-side gradients (W2, b2, P_sqrt, Q)
# are sums of <= 16 rows, so they carry the error of the forward's saved y / z, not that of a batch sum.  What was checked
# (backward of forward_train, six seeds per shape): the ratios hold across seeds (3.2 - 4.5 at B = 3, 2.2 - 3.3 at B = 8);
# recomputing the four gradients in fp64 from the device's own saved y / z leaves only 7 - 30 % of the RMS error, so the
# backward's arithmetic is not the source.
# The cause is the UNIT, not the kernels (tests/test_fp32_units_fwd_train_gpu.py, tests/test_fwd_chain_ref_cpu.py):
#  * Measured directly, rows of many launches pooled and the oracle run once on the pooled rows, the saved y / z of the
#    training-mode forward are 1.00 / 1.25 units at (400, 180, 192), 1.40 / 1.50 at (500, 150, 160) and 0.74 / 1.18 at
#    (512, 150, 150) — the same at B = 1, 3, 8, 17 and 1003, and to two digits what a numpy restatement of the kernels'
#    summation order with one rounding per product gives on the CPU (tests/fwd_chain_ref.py, FMAF: 1.00 / 1.25, 1.40 / 1.50,
#    0.73 / 1.19).  The 100 - 125-step accumulator chains of D0 = 400 / 500 are worth 1.0 - 1.4 units, not 3; the K-split of
#    D0 = 512 halves that.  The forward has no excess at any batch size.
#  * numpy's float32 matmul takes another BLAS path when it is handed a handful of rows (OpenBLAS 0.3.29: up to 6 rows at
#    (400, 180, 192), up to 8 at (500, 150, 160) and (512, 150, 150)), and there the float32 oracle's own rms error is
#    2.3 - 3.1 x smaller (y: 0.88e-8 against 2.70e-8, 1.03e-8 against 2.38e-8).  orc.backward embeds x1 and x2 separately, B rows
#    per call, so at B = 3 — and at D0 = 512 still at B = 8 — its float32 run is that much closer to fp64 and every ratio
#    that much larger.  The same numpy restatement, measured against a 6-row oracle, reads 3.1 - 3.2 (y) and 3.6 - 3.7 (z)
#    units at D0 = 400 / 500: the "3.0 / 3.8" first reported here for the kernel.  At D0 = 512, B = 8 the forward's 0.74 /
#    1.18 read 1.7 / 2.7 in the 8-row unit, the range of the gradients' 2.2 - 3.3 there (the gradients themselves were not
#    measured again against a pooled oracle: a batch sum cannot be pooled).
# These cases keep 6 / 8 instead of 3 / 5 (the half-tile mutant measures 8.6 / 8.6 at B = 8): the tests below hand the oracle
# the batch as it is, so the small unit stays in their measurement.
TINY_B = dict(rms_max=6.0, max_max=8.0)


def _inputs(seed, D0, D1, D2, B):
    rng = np.random.default_rng(seed)
    p = rand_params(rng, D0, D1, D2)
    x1 = rng.standard_normal((B, D0)).astype(np.float32)
    x2 = rng.standard_normal((B, D0)).astype(np.float32)
    return rng, p, x1, x2


def _check_grads(got, r64, r32, what, names=NAMES, thr=None):
    return {name: fu.assert_fp32_level(got[name], r64[name], r32[name], f"{what} d{name}", **(thr or {})) for name in names}


# (D0, D1, D2, B): the small-batch K-A path (B <= 16 384); bwd_data_stream_kernel with the wide wgrad_fm_kernel (NB 10 and 11);
# the generic data-gradient path of NB < 8; the weight-gradient fall-backs of a part-filled last 32-column tile (the comment
# above tests/test_train_gpu.py::test_backward_matches_oracle) at 3 and 4097 rows.  Measured worst rms / max ratio over every
# tensor and dx: 1.55 / 1.98 (B >= 4097), 4.47 / 5.73 at B = 3 (TINY_B above).
BACKWARD_CASES = [(512, 150, 150, 3000), (512, 170, 170, 4097), (512, 150, 150, 20037), (512, 170, 170, 20037),
                  (512, 150, 150, 70001), (512, 170, 170, 70001), (64, 24, 20, 20037),
                  (500, 150, 160, 3), (500, 150, 160, 4097), (400, 180, 192, 3), (400, 180, 192, 4097)]


@pytest.mark.parametrize("want_dx", [False, True])
@pytest.mark.parametrize("D0,D1,D2,B", BACKWARD_CASES)
def test_backward(hip_lib, D0, D1, D2, B, want_dx):
    from neuralplda_amd import ops
    rng, p, x1, x2 = _inputs(D1 * 7 + B, D0, D1, D2, B)
    g = (rng.standard_normal(B) / B).astype(np.float32)
    dev = to_dev(p)
    packed = ops.pack_params(*dev)
    _, saved = ops.forward_train(torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda(), packed)
    out = ops.backward(saved, torch.from_numpy(g).cuda(), packed, dev[4], want_dx=want_dx)
    flat = out[0] if want_dx else out
    got = {k: t.cpu().numpy() for k, t in zip(NAMES, ops.split_flat_grad(flat, D0, D1, D2))}
    what = f"backward ({D0}, {D1}, {D2}) B={B} dx={want_dx}"
    _check_grads(got, orc.backward(x1, x2, g, p, np.float64), orc.backward(x1, x2, g, p, np.float32), what,
                 thr=TINY_B if B <= 8 else None)
    if want_dx:
        d64, d32 = orc.input_grads(x1, x2, g, p, np.float64), orc.input_grads(x1, x2, g, p, np.float32)
        reg = fu.Regions(B, 16, seed=B)
        for i in range(2):
            fu.assert_fp32_level(out[1 + i].cpu().numpy()[reg.idx], d64[i][reg.idx], d32[i][reg.idx], f"{what} dx{i + 1}", reg)


def _loss_setup(lossname, B, rng):
    from neuralplda_amd import ops
    t = (rng.random(B) < 0.3).astype(np.float32)
    t[0], t[-1] = 1.0, 0.0
    kind = ops.LOSS_SOFTCDET if lossname == "SoftCdet" else ops.LOSS_BCE
    theta = [-0.4, -0.2] if kind == ops.LOSS_SOFTCDET else [0.1]
    betas, alpha = ([99.0, 199.0], 15.0) if kind == ops.LOSS_SOFTCDET else ([], 0.0)
    return t, kind, theta, betas, alpha


def _upstream(s, t, kind, theta, betas, alpha):
    from neuralplda_amd import ops
    if kind == ops.LOSS_SOFTCDET:
        return orc.softcdet_grad(s, t, theta, betas, alpha)[0]
    return orc.crossentropy_grad(s, t, theta[0])[0]


def _step_refs(x1, x2, t, p, kind, theta, betas, alpha, fn):
    """fp64 and fp32 yardsticks of a training step's gradient: the upstream dL/ds is taken (in fp64) on the oracle's own
    scores of the same precision — the kernel forms it from its own fp32 scores, so an fp32 computation of the whole step
    carries the same score-rounding term (alpha |ds| relative, ~15 fp32 ulps at SoftCdet's alpha = 15)."""
    out = []
    for dt in (np.float64, np.float32):
        g = _upstream(orc.forward(x1, x2, p, dt).astype(np.float64), t, kind, theta, betas, alpha)
        out.append(fn(x1, x2, g, p, dt))
    return out


def _adam_state(n, K):
    z = lambda k: torch.zeros(k, device="cuda")  # noqa: E731
    return z(n + K), z(n + K), z(2), z(n + K), torch.zeros((), device="cuda")


# one-call step: B <= 2048 the 8-pair half-tile kernel (nplda_train_fb_half.h), 4096 / 9000 the 16-pair kernel.  Measured worst
# rms / max: 1.65 / 1.51 (B >= 1003), 3.33 / 4.47 at B = 8 (TINY_B); the rows form 1.18 / 1.17; the dx form 2.08 / 3.05.
@pytest.mark.parametrize("lossname", ["SoftCdet", "crossentropy"])
@pytest.mark.parametrize("D,B", [(150, 8), (150, 1003), (150, 2048), (170, 1003), (150, 4096), (170, 9000)])
def test_train_step(hip_lib, lossname, D, B):
    from neuralplda_amd import ops
    rng, p, x1, x2 = _inputs(1000 * D + B, 512, D, D, B)
    t, kind, theta, betas, alpha = _loss_setup(lossname, B, rng)
    prm = to_dev(p)
    packed = ops.pack_params(*prm)
    n = int(sum(q.numel() for q in prm))
    m, v, step, out, lbuf = _adam_state(n, len(theta))
    ops.train_step(torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda(), torch.from_numpy(t).cuda(), prm,
                   [torch.tensor([th], device="cuda") for th in theta], betas, alpha, kind, m, v, step, 1e-3, 0.9, 0.999, 1e-8,
                   1e-5, packed, ops.train_step_workspace(B, packed), lbuf, grad_out=out)
    got = {k: a.cpu().numpy() for k, a in zip(NAMES, ops.split_flat_grad(out[:n], 512, D, D))}
    r64, r32 = _step_refs(x1, x2, t, p, kind, theta, betas, alpha, orc.backward)
    _check_grads(got, r64, r32, f"train_step {lossname} D={D} B={B}", thr=TINY_B if B <= 8 else None)


@pytest.mark.parametrize("lossname", ["SoftCdet", "crossentropy"])
def test_train_step_rows(hip_lib, lossname):
    from neuralplda_amd import ops
    D, B, N = 150, 1003, 5000
    rng, p, table, _ = _inputs(D + B + 1, 512, D, D, N)
    r1, r2 = rng.integers(0, N, B), rng.integers(0, N, B)
    t, kind, theta, betas, alpha = _loss_setup(lossname, B, rng)
    prm = to_dev(p)
    packed = ops.pack_params(*prm)
    n = int(sum(q.numel() for q in prm))
    m, v, step, out, lbuf = _adam_state(n, len(theta))
    ops.train_step_rows(torch.from_numpy(table).cuda(), torch.from_numpy(r1).cuda(), torch.from_numpy(r2).cuda(),
                        torch.from_numpy(t).cuda(), prm, [torch.tensor([th], device="cuda") for th in theta], betas, alpha,
                        kind, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1e-5, packed, ops.train_step_workspace(B, packed, rows=True),
                        lbuf, grad_out=out)
    got = {k: a.cpu().numpy() for k, a in zip(NAMES, ops.split_flat_grad(out[:n], 512, D, D))}
    r64, r32 = _step_refs(table[r1], table[r2], t, p, kind, theta, betas, alpha, orc.backward)
    _check_grads(got, r64, r32, f"train_step_rows {lossname}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("lossname", ["SoftCdet", "crossentropy"])
@pytest.mark.parametrize("D,B", [(150, 1003), (170, 4096)])
def test_train_step_dx(hip_lib, lossname, bf16, D, B):
    """train_step_dx's dL/dx1, dL/dx2.  With bf16 rows the inputs are the bf16 values and the outputs are stored in bf16: the
    fp32 unit is then the fp32 oracle's dx rounded to bf16 (the storage rounding dominates both)."""
    from neuralplda_amd import ops
    rng, p, x1, x2 = _inputs(D + B + 2 + bf16, 512, D, D, B)
    dt = torch.bfloat16 if bf16 else torch.float32
    X1, X2 = torch.from_numpy(x1).cuda().to(dt), torch.from_numpy(x2).cuda().to(dt)
    x1, x2 = X1.float().cpu().numpy(), X2.float().cpu().numpy()
    t, kind, theta, betas, alpha = _loss_setup(lossname, B, rng)
    prm = to_dev(p)
    packed = ops.pack_params(*prm)
    n = int(sum(q.numel() for q in prm))
    m, v, step, _, lbuf = _adam_state(n, len(theta))
    dx1, dx2 = torch.empty_like(X1), torch.empty_like(X2)
    ws = ops.train_step_dx_workspace(B, packed, bf16)
    assert ws is not None
    ops.train_step_dx(X1, X2, torch.from_numpy(t).cuda(), prm, [torch.tensor([th], device="cuda") for th in theta], betas,
                      alpha, kind, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1e-5, packed, ws, lbuf, dx1, dx2)
    r64, r32 = _step_refs(x1, x2, t, p, kind, theta, betas, alpha, orc.input_grads)
    reg = fu.Regions(B, 16, seed=B)
    for i, dx in enumerate((dx1, dx2)):
        ref32 = r32[i]
        if bf16:
            ref32 = torch.from_numpy(ref32.astype(np.float32)).to(torch.bfloat16).float().numpy()
        fu.assert_fp32_level(dx.float().cpu().numpy(), r64[i], ref32, f"train_step_dx {lossname} bf16={bf16} D={D} B={B} dx{i + 1}",
                             reg)


@pytest.mark.parametrize("D0,D,N", [(512, 150, 3000), (512, 170, 20037), (64, 24, 777)])  # measured 1.16 / 1.22
def test_embed_backward(hip_lib, D0, D, N):
    from neuralplda_amd import ops
    rng, p, x, _ = _inputs(D + N + 3, D0, D, D, N)
    gz = (rng.standard_normal((N, D)) / N).astype(np.float32)
    packed = ops.pack_params(*to_dev(p))
    _, saved = ops.embed_train(torch.from_numpy(x).cuda(), packed)
    flat, dx = ops.embed_backward(saved, torch.from_numpy(gz).cuda(), packed, want_dx=True)
    grads = [a.cpu().numpy() for a in ops.split_flat_grad(flat, D0, D, D)]
    assert np.all(grads[4] == 0) and np.all(grads[5] == 0)
    got = dict(zip(NAMES[:4], grads[:4]), x=dx.cpu().numpy())
    r64, r32 = orc.embed_backward(x, gz, p, np.float64), orc.embed_backward(x, gz, p, np.float32)
    _check_grads(got, r64, r32, f"embed_backward ({D0}, {D}) N={N}", names=NAMES[:4] + ("x",))


@pytest.mark.parametrize("D,B", [(150, 20037), (170, 1000)])  # measured 0.79 / 1.00
def test_score_embeddings_bwd(hip_lib, D, B):
    from neuralplda_amd import ops
    rng = np.random.default_rng(D + B)
    p = rand_params(rng, 512, D, D)
    z1 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    z2 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    g = (rng.standard_normal(B) / B).astype(np.float32)
    dz1, dz2, dps, dq = ops.score_embeddings_bwd(*(torch.from_numpy(a).cuda() for a in (z1, z2, p.P_sqrt, p.Q, g)))
    got = dict(z1=dz1.cpu().numpy(), z2=dz2.cpu().numpy(), P_sqrt=dps.cpu().numpy(), Q=dq.cpu().numpy())
    _check_grads(got, orc.embscore_backward(z1, z2, g, p, np.float64), orc.embscore_backward(z1, z2, g, p, np.float32),
                 f"score_embeddings_bwd D={D} B={B}", names=("z1", "z2", "P_sqrt", "Q"))
