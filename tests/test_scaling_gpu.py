"""Power-of-two scaling relations, bit for bit.  A rescaling by 2^k commutes with every fp32 / bf16 rounding while nothing
overflows, underflows or turns denormal, and the library's sqrtf and divisions are correctly rounded (no fast-math flag in
neuralplda_amd/build.py), so these hold EXACTLY for every kernel — any hidden absolute constant, eps or scale-dependent branch
breaks them:
  * (x1, x2, b1) -> 2^k (x1, x2, b1): u scales, the normalised y does not: scores, z and q are unchanged;
  * (W2, b2) -> 2^k (W2, b2), or (Q, P_sqrt) -> (4^k Q, 2^k P_sqrt): scores x 4^k (v6's split layer 2 included: its bf16 pieces
    scale exactly);
  * g -> 2^k g: every gradient x 2^k;
  * scores -> 2^k scores: detection costs and EER unchanged, thresholds x 2^k.
The cohort statistics hold absolute constants in their proposal stage (which rows take the exact fall-back may change with
scale), so they are checked within the fp32-unit thresholds instead, and for the fall-back bound nfb <= R // 20.
k = -6 / 5 keep the inputs (standard normal) and every intermediate far from fp32's denormal and overflow ranges."""
import numpy as np
import pytest
import torch

from oracle import nplda_oracle as orc
from tests import fp32_units as fu
from tests.test_forward_gpu import rand_params, to_dev

pytestmark = pytest.mark.gpu
KS = [-6, 5]


def _scaled(p, **f):
    t = dict(zip(("W1", "b1", "W2", "b2", "P_sqrt", "Q"), p.tensors()))
    for k, v in f.items():
        t[k] = (t[k] * np.float32(v)).astype(np.float32)
    return orc.Params(t["W1"], t["b1"], t["W2"], t["b2"], t["P_sqrt"], t["Q"])


def _inputs(seed, D0, D, B):
    rng = np.random.default_rng(seed)
    p = rand_params(rng, D0, D, D)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return p, torch.randn(B, D0, device="cuda", generator=gen), torch.randn(B, D0, device="cuda", generator=gen)


def _eq(a, b, what):
    a, b = a.float(), b.float()
    assert torch.equal(a, b), f"{what}: max |d| = {(a - b).abs().max().item()} over {int((a != b).sum())} values"


# (D0, D, B, precision, bf16 rows): the balanced-tile, small, v6 (split layer 2), FWD_SPLIT, v5, v3 kernels, bf16 rows, bf16x3
PAIR_CASES = [(512, 150, 1000, "fp32", False), (512, 150, 3000, "fp32", False), (512, 150, 32768, "fp32", False),
              (512, 150, 131072 + 77, "fp32", False), (512, 170, 32768, "fp32", False), (512, 170, 20037, "fp32", False),
              (512, 128, 20037, "fp32", False), (72, 150, 20037, "fp32", False), (512, 150, 32768, "fp32", True),
              (512, 170, 32768, "fp32", True), (512, 150, 1000, "bf16x3", False), (512, 150, 20037, "bf16x3", False)]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D0,D,B,precision,bf16", PAIR_CASES)
def test_pair_scores_scale_exactly(hip_lib, D0, D, B, precision, bf16, k):
    from neuralplda_amd import ops
    p, x1, x2 = _inputs(B + D, D0, D, B)
    if bf16:
        x1, x2 = x1.bfloat16(), x2.bfloat16()
    f, f2 = 2.0 ** k, 4.0 ** k
    score = lambda q, a, b: ops.score_pairs(a, b, ops.pack_params(*to_dev(q), precision=precision))  # noqa: E731
    s = score(p, x1, x2)
    _eq(score(_scaled(p, b1=f), x1 * f, x2 * f), s, "(x1, x2, b1) x 2^k")
    _eq(score(_scaled(p, W2=f, b2=f), x1, x2), s * f2, "(W2, b2) x 2^k")
    _eq(score(_scaled(p, Q=f2, P_sqrt=f), x1, x2), s * f2, "(Q, P_sqrt) x (4^k, 2^k)")


@pytest.mark.parametrize("k", KS)
# balanced-tile, small, v2 (tests/test_fp32_units_fwd_gpu.py: EMBED_CASES, pinned by tests/test_fp32_units_dispatch_cpu.py)
@pytest.mark.parametrize("D,N", [(150, 1000), (150, 5000), (170, 262144 - 153)])
def test_embeddings_scale_exactly(hip_lib, D, N, k):
    from neuralplda_amd import ops
    p, x, xb = _inputs(N + D + 1, 512, D, N)
    f = 2.0 ** k
    pk, pks, pkw = (ops.pack_params(*to_dev(q)) for q in (p, _scaled(p, b1=f), _scaled(p, W2=f, b2=f)))
    z, q = ops.embed(x, pk)
    zs, qs = ops.embed(x * f, pks)
    _eq(zs, z, "embed z, (x, b1) x 2^k")
    _eq(qs, q, "embed q, (x, b1) x 2^k")
    zw, qw = ops.embed(x, pkw)
    _eq(zw, z * f, "embed z, (W2, b2) x 2^k")
    _eq(qw, q * f * f, "embed q, (W2, b2) x 2^k")
    if N <= 5000:
        rows = torch.from_numpy(np.random.default_rng(N).integers(0, N, 1501)).cuda()
        _eq(ops.embed_rows(x * f, rows, pks)[0], ops.embed_rows(x, rows, pk)[0], "embed_rows z")
        (za, _), (zb, _) = ops.embed_pair(x[:700] * f, xb[:801] * f, pks)
        (za0, _), (zb0, _) = ops.embed_pair(x[:700], xb[:801], pk)
        _eq(za, za0, "embed_pair a")
        _eq(zb, zb0, "embed_pair b")
        r1, r2 = (torch.from_numpy(np.random.default_rng(N + i).integers(0, N, 20037)).cuda() for i in range(2))
        s = ops.score_pairs_rows(x, r1, r2, pk)
        _eq(ops.score_pairs_rows(x * f, r1, r2, pks), s, "score_pairs_rows")
        _eq(ops.score_indexed(z, q, r1, r2, pk), ops.score_indexed(zs, qs, r1, r2, pks), "score_indexed")
        _eq(ops.score_indexed(zw, qw, r1, r2, pkw), ops.score_indexed(z, q, r1, r2, pk) * f * f, "score_indexed (W2, b2)")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D0,D1,D2,B", [(512, 150, 150, 3000), (512, 170, 170, 20037), (512, 150, 150, 70001),
                                        (64, 24, 20, 20037), (500, 150, 160, 4097)])
def test_gradients_scale_with_the_upstream_gradient(hip_lib, D0, D1, D2, B, k):
    from neuralplda_amd import ops
    rng = np.random.default_rng(D1 + B)
    p = rand_params(rng, D0, D1, D2)
    dev = to_dev(p)
    packed = ops.pack_params(*dev)
    x1, x2 = (torch.from_numpy(rng.standard_normal((B, D0)).astype(np.float32)).cuda() for _ in range(2))
    g = torch.from_numpy((rng.standard_normal(B) / B).astype(np.float32)).cuda()
    f = 2.0 ** k
    _, saved = ops.forward_train(x1, x2, packed)
    flat, dx1, dx2 = ops.backward(saved, g, packed, dev[4], want_dx=True)
    flat_s, dx1_s, dx2_s = ops.backward(saved, g * f, packed, dev[4], want_dx=True)
    _eq(flat_s, flat * f, "backward flat")
    _eq(dx1_s, dx1 * f, "backward dx1")
    _eq(dx2_s, dx2 * f, "backward dx2")
    _eq(ops.backward(saved, g * f, packed, dev[4]), ops.backward(saved, g, packed, dev[4]) * f, "backward flat (no dx)")
    # embed_backward and the score-epilogue backward
    _, es = ops.embed_train(x1, packed)
    gz = torch.from_numpy((rng.standard_normal((B, D2)) / B).astype(np.float32)).cuda()
    fl, dx = ops.embed_backward(es, gz, packed, want_dx=True)
    fl_s, dx_s = ops.embed_backward(es, gz * f, packed, want_dx=True)
    _eq(fl_s, fl * f, "embed_backward flat")
    _eq(dx_s, dx * f, "embed_backward dx")
    z1, z2 = (torch.from_numpy((rng.standard_normal((B, D2)) * 0.3).astype(np.float32)).cuda() for _ in range(2))
    a = ops.score_embeddings_bwd(z1, z2, dev[4], dev[5], g)
    b = ops.score_embeddings_bwd(z1, z2, dev[4], dev[5], g * f)
    for name, u, v in zip(("dz1", "dz2", "dP_sqrt", "dQ"), a, b):
        _eq(v, u * f, "score_embeddings_bwd " + name)


@pytest.mark.parametrize("k", [-6, 5, 20])
@pytest.mark.parametrize("B", [1000, 50000])
def test_detection_costs_are_scale_free(hip_lib, B, k):
    from neuralplda_amd import metrics
    rng = np.random.default_rng(B)
    t = torch.from_numpy((rng.random(B) < 0.1).astype(np.float32)).cuda()
    s = torch.from_numpy((rng.standard_normal(B) + 2 * t.cpu().numpy()).astype(np.float32)).cuda()
    f = 2.0 ** k
    betas = [99.0, 199.0]
    for sem in (True, False):
        c, th = metrics.minc(s, t, betas, reference_semantics=sem)
        cs, ths = metrics.minc(s * f, t, betas, reference_semantics=sem)
        _eq(cs, c, f"minc cost (reference semantics {sem})")
        for b in betas:
            _eq(ths[b], th[b] * f, f"minc threshold beta={b} (reference semantics {sem})")
    c, th = metrics.minc_exact(s, t, betas)
    cs, ths = metrics.minc_exact(s * f, t, betas)
    _eq(cs, c, "minc_exact cost")
    for b in betas:
        _eq(ths[b], th[b] * f, f"minc_exact threshold beta={b}")
    assert metrics.eer(s * f, t) == metrics.eer(s, t)


@pytest.mark.parametrize("D,R,M,topn", [(150, 300, 10000, 500), (170, 129, 4096, 100)])
def test_cohort_statistics_scale_with_the_embeddings(hip_lib, D, R, M, topn):
    """z of the rows and the cohort x 2^k (q x 4^k): all four columns x 4^k within the fp32-unit thresholds (fused split form),
    and the rows handed to the exact fall-back stay within the bound of tests/test_cohort_fused_gpu.py at every scale."""
    from neuralplda_amd import ops
    from tests.test_fp32_units_fwd_gpu import _cohort_setup, check_cohort, cohort_refs
    p, packed, zr, qr, zc, qc = _cohort_setup(D, R, M, D + R + 29)
    r64, r32 = cohort_refs(p, zr, qr, zc, qc, D, topn)
    for k in (-8, 0, 8):
        f = 2.0 ** k
        got, nfb = ops.cohort_stats(zr * f, qr * f * f, zc * f, qc * f * f, packed, topn=topn, return_fallback_rows=True)
        assert nfb is not None and nfb <= R // 20, (k, nfb)
        check_cohort(got.cpu().numpy() / (f * f), r64, r32, f"cohort stats at 2^{k}")
