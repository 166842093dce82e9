"""torch.optim.Adam's update as csrc/nplda_adam_math.h computes it, against tests/adam_ref.py in fp32 units.

Compared: the parameter update p' - p (formed in float64 from the stored float32 values), m' and v', per tensor, in units
of the error the float32 evaluation of the same formulas makes (tests/fp32_units.py, default gates 3 rms / 5 max).  The
reference takes the bias corrections 1 - beta^t from float64 in both precisions (torch computes them in double on the host).
A ratio over a handful of values is a draw, so tensors of fewer than fp32_units.REGION_ROWS elements are pooled per magnitude
class and the pool is gated; the largest tensor is also gated per region of fp32_units.Regions(n, 1024, full=True): first
tile, last full tile, the ragged 1029-element tail behind the second grid-stride pass, and the rest.  Where a pool stays
below REGION_ROWS (the K thresholds of the fused steps, the small per-t groups of the host-logic test) there is no ratio;
those elements, like every element of every tensor, are held to adam_ref.bounds, the worst-case float32 rounding error of
p', m' and v' derived there (the float32 reference reaches 0.98 of it, tests/test_loss_adam_ref_cpu.py keeps it inside).

States: |p| ~ 1e-4 (where the store of p' does not mask the update's own arithmetic) and |p| ~ 0.05; g log-uniform in
1e-12 .. 1e2 with random sign and 2 % exact zeros; m, v from two earlier gradients (zero at t = 1).

(a) nplda_adam_step_f32 through FusedAdam, state loaded with load_state_dict: 25 tensors (launches of 12 + 12 + 1, sizes
    around the 256-thread block and the 1024-element block share, one zero-element tensor inside a launch) and one tensor
    of 2 097 152 + 1029 elements followed by two small ones (2048 blocks, a grid-stride pass, the segment search behind a
    large segment), at t = 1, 2, 3, 10, 1000, 100 000 and three sets of hyper-parameters.
(b) FusedAdam's host logic: 14 tensors, 6 steps, gradients missing in a fixed pattern and freshly allocated every step
    (more than 16 distinct launch blocks), a state_dict round trip after step 3; every state[p]["step"] is torch's count.
(c) the same update inside ops.train_step (three consecutive steps, the thresholds and the refreshed packed image included)
    and inside ops.dplda_update / dplda_update_loss.

Measured on MI355X (worst rms / max ratio of p' - p over the tensors and pools of a case):

    case                                           bias corrections in float32 (before)        in double (now)
    ---------------------------------------------  ------------------------------------------  ---------------
    (a) t = 1                                      1.00 / 1.03                                 1.00 / 1.03
        t = 2, beta = (0.9, 0.999)                 42.9 - 48.3 / 11.1 - 23.0                   1.00 / 1.08
        t = 3, beta = (0.9, 0.999)                 41.3 - 45.4 / 9.7 - 18.1                    1.00 / 1.30
        t = 2, 3, beta = (0.8, 0.99)               3.03 - 4.74 / 1.52 - 2.76                   1.00 / 1.13
        t = 10, beta = (0.9, 0.999)                3.01 - 3.25 / 1.60 - 2.00                   1.00 / 1.00
        t = 1000, 100 000                          1.00 / 1.20                                 1.00 / 1.20
    (b) host logic, worst of 6 steps               36.9 / 15.5 (step 2)                        1.00 / 1.20
    (c) train_step, D = 150 / 170, B = 1003 / 4096 (not measured)                              1.00 / 1.01
        dplda_update, dplda_update_loss            (not measured)                              1.00 / 1.01

    2 M-element tensor, worst over the whole and its regions (first tile, last full tile, ragged tail, rest), now:
        t = 1 .. 100 000                           0.88 - 0.95 / 0.90 - 1.10
    empty segments (last, first, alone, only)      counters exact, neighbours inside adam_ref.bounds

The "before" column is what made csrc/nplda_adam_math.h form 1 - beta^t in double (see consts_for there); it also needed a
zero-element tensor, whose null pointers nplda_adam_step_f32 used to refuse, to be accepted.
"""
import numpy as np
import pytest
import torch

from tests import adam_ref
from tests import fp32_units as fu

pytestmark = pytest.mark.gpu

HYPER = {  # lr, beta1, beta2, eps, weight decay
    "default": (1e-3, 0.9, 0.999, 1e-8, 1e-5),
    "no-decay": (5e-4, 0.9, 0.999, 1e-8, 0.0),
    "fast-betas": (1e-3, 0.8, 0.99, 1e-6, 1e-5),
}
SMALL_SIZES = [1, 3, 255, 256, 257, 1023, 1024, 1025, 4099, 7, 300, 64, 0, 513, 2, 100, 31, 2048, 5, 129, 640, 12, 1, 77, 333]
BIG_SIZES = [2097152 + 1029, 3, 700]


def make_state(sizes, t, hp, seed):
    """Per tensor (p, g, m, v) as float32; tensors alternate between the two magnitude classes."""
    rng = np.random.default_rng(seed)
    _, b1, b2, _, _ = hp
    out = []
    for i, n in enumerate(sizes):
        scale = 1e-4 if i % 2 == 0 else 0.05
        p = (scale * rng.standard_normal(n)).astype(np.float32)
        g = (10.0 ** rng.uniform(-12, 2, n) * rng.choice([-1.0, 1.0], n))
        g[rng.random(n) < 0.02] = 0.0
        g = g.astype(np.float32)
        if t > 1:
            g0 = g * np.exp(0.5 * rng.standard_normal(n)) * rng.choice([1.0, 1.0, 1.0, -1.0], n)
            g1 = g * np.exp(0.5 * rng.standard_normal(n))
            m = (b1 * (1 - b1) * g0 + (1 - b1) * g1).astype(np.float32)
            v = (b2 * (1 - b2) * g0 * g0 + (1 - b2) * g1 * g1).astype(np.float32)
        else:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        out.append((p, g, m, v))
    return out


def gate(got, r64, r32, p, what, regions=None):
    """fp32-units gate of (p' - p, m', v') of one tensor or pool, over the whole of it and every region; returns the worst
    ratios of p' - p."""
    p = p.astype(np.float64)
    res = None
    for name, i in (("dp", 0), ("m", 1), ("v", 2)):
        a, b, c = (x[i].astype(np.float64) - (p if i == 0 else 0.0) for x in (got, r64, r32))
        r = fu.assert_fp32_level(a, b, c, f"{what} {name}", regions=regions)
        res = res or (max(x[0] for x in r.values()), max(x[1] for x in r.values()))
    return res


def check_tensors(state, got, t, hp, what, classes=None):
    """state: [(p, g, m, v)], got: [(p', m', v')] from the device; the reference steps every tensor from `state`.
    classes: the magnitude class of every tensor (default: they alternate).  Every element of every tensor is held to
    adam_ref.bounds (worst-case rounding); tensors and pools of >= REGION_ROWS elements also to the fp32-units gate, the
    tensors above 2^20 elements per region as well (Regions(..., full=True): its positions are then row numbers)."""
    worst = [0.0, 0.0]
    pools = {}
    for i, ((p, g, m, v), dev) in enumerate(zip(state, got)):
        r64 = adam_ref.step(p, g, m, v, t, *hp, dtype=np.float64)
        r32 = adam_ref.step(p, g, m, v, t, *hp, dtype=np.float32)
        for name, a, b, bd in zip(("p'", "m'", "v'"), dev, r64, adam_ref.bounds(p, g, m, v, t, *hp)):
            err = np.abs(a.astype(np.float64) - b)
            assert np.all(err <= bd), f"{what} tensor {i} ({p.size}) {name}: {(err / bd).max(initial=0.0):.2f} of the rounding bound"
        if p.size >= fu.REGION_ROWS:
            regions = fu.Regions(p.size, 1024, full=True) if p.size > 1 << 20 else None
            r = gate(dev, r64, r32, p, f"{what} tensor {i} ({p.size})", regions)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        else:
            pools.setdefault(classes[i] if classes else i % 2, []).append((dev, r64, r32, p))
    for cls, items in pools.items():
        cat = lambda j: tuple(np.concatenate([it[j][q] for it in items]) for q in range(3))  # noqa: E731
        pp = np.concatenate([it[3] for it in items])
        if pp.size >= fu.REGION_ROWS:  # (a smaller pool is too few values for a statistic: the bounds above are its check)
            r = gate(cat(0), cat(1), cat(2), pp, f"{what} pool of small tensors, class {cls} ({pp.size})")
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    return worst


def run_fused_adam(state, t, hp):
    from neuralplda_amd.optim import FusedAdam
    lr, b1, b2, eps, wd = hp
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()) for p, _, _, _ in state]
    opt = FusedAdam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    if t > 1:
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()),
                           "exp_avg_sq": torch.from_numpy(v.copy())} for i, (_, _, m, v) in enumerate(state)}
        opt.load_state_dict(sd)
    for q, (_, g, _, _) in zip(params, state):
        q.grad = torch.from_numpy(g.copy()).cuda()
    opt.step()
    torch.cuda.synchronize()
    got = [(q.detach().cpu().numpy(), opt.state[q]["exp_avg"].cpu().numpy().reshape(-1),
            opt.state[q]["exp_avg_sq"].cpu().numpy().reshape(-1)) for q in params]
    steps = [float(opt.state[q]["step"]) for q in params]
    return got, steps


@pytest.mark.parametrize("hyper", list(HYPER))
@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 100000])
@pytest.mark.parametrize("layout", ["25 tensors", "2 M + 2"])
def test_adam_step_kernel(hip_lib, layout, t, hyper):
    sizes = SMALL_SIZES if layout == "25 tensors" else BIG_SIZES
    hp = HYPER[hyper]
    state = make_state(sizes, t, hp, seed=t + len(sizes))
    got, steps = run_fused_adam(state, t, hp)
    # the device counter of every launch (12 + 12 + 1 tensors; the zero-element tensor's launch too) advanced by exactly one
    assert steps == [float(t)] * len(sizes), steps
    worst = check_tensors(state, got, t, hp, f"adam_step {layout} t={t} {hyper}")
    print(f"adam_step {layout} t={t} {hyper}: dp {worst[0]:.2f}/{worst[1]:.2f}")


@pytest.mark.parametrize("sizes", [[300, 5, 0], [0, 0], [7] * 12 + [0], [0, 260]], ids=["empty last", "only empty", "empty alone in its launch", "empty first"])
def test_adam_step_empty_segments(hip_lib, sizes):
    """A zero-element tensor (null pointers) as the last segment of a launch, as the first, alone in a launch of its own
    (the 13th tensor) and a launch of nothing but empty tensors (total == 0: one block that only counts the step): the
    others take the step of the reference and every counter advances by exactly one, over two consecutive steps."""
    hp = HYPER["default"]
    for t in (1, 2):
        state = make_state(sizes, t, hp, seed=t)
        got, steps = run_fused_adam(state, t, hp)
        assert steps == [float(t)] * len(sizes), steps
        check_tensors(state, got, t, hp, f"empty segments {sizes} t={t}")
        for (p, _, _, _), (p1, m1, v1) in zip(state, got):
            assert p1.size == p.size and m1.size == p.size and v1.size == p.size


HOST_SIZES = [300, 1, 17, 1024, 5, 260, 64, 2, 700, 33, 256, 3, 129, 400]


def _has_grad(step, i):
    """The fixed pattern of missing gradients: parameter 5 starts late, every third skips step 1, every fourth steps 2-3."""
    return not ((i == 5 and step == 0) or (i % 3 == 1 and step == 1) or (i % 4 == 2 and step in (2, 3)))


def test_fused_adam_host_logic(hip_lib):
    from neuralplda_amd.optim import FusedAdam
    hp = HYPER["default"]
    lr, b1, b2, eps, wd = hp
    rng = np.random.default_rng(7)
    p0 = [((1e-4 if i % 2 == 0 else 0.05) * rng.standard_normal(n)).astype(np.float32) for i, n in enumerate(HOST_SIZES)]
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in p0]
    opt = FusedAdam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    count = [0] * len(params)
    # torch.optim.Adam on the CPU over the same pattern of missing gradients (one element per parameter): its step counts
    tq = [torch.zeros(1, requires_grad=True) for _ in params]
    topt = torch.optim.Adam(tq, lr=lr)
    keep = []  # every gradient stays alive: each step's live at addresses of their own
    worst = [0.0, 0.0]
    for step in range(6):
        grads = [(10.0 ** rng.uniform(-6, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) if _has_grad(step, i) else None
                 for i, n in enumerate(HOST_SIZES)]
        before = []
        for q in params:
            st = opt.state.get(q, {})
            z = np.zeros(q.numel(), np.float32)
            before.append((q.detach().cpu().numpy().copy(),
                           st["exp_avg"].cpu().numpy().reshape(-1).copy() if "exp_avg" in st else z,
                           st["exp_avg_sq"].cpu().numpy().reshape(-1).copy() if "exp_avg_sq" in st else z))
        for q, g in zip(params, grads):
            q.grad = None if g is None else torch.from_numpy(g).cuda()
            if q.grad is not None:
                keep.append(q.grad)
        opt.step()
        torch.cuda.synchronize()
        for q, g in zip(tq, grads):
            q.grad = None if g is None else torch.ones(1)
        topt.step()
        ts = set()
        for i, (q, g) in enumerate(zip(params, grads)):
            now = q.detach().cpu().numpy()
            if g is None:
                assert np.array_equal(now, before[i][0]), f"step {step}: parameter {i} had no gradient and moved"
                continue
            count[i] += 1
            ts.add(count[i])
        for tval in sorted(ts):  # (parameters that have taken the same number of steps share the reference's t)
            idx = [i for i, g in enumerate(grads) if g is not None and count[i] == tval]
            state = [(before[i][0], grads[i], before[i][1], before[i][2]) for i in idx]
            got = [(params[i].detach().cpu().numpy(), opt.state[params[i]]["exp_avg"].cpu().numpy().reshape(-1),
                    opt.state[params[i]]["exp_avg_sq"].cpu().numpy().reshape(-1)) for i in idx]
            w = check_tensors(state, got, tval, hp, f"host logic step {step} t={tval}", classes=[i % 2 for i in idx])
            worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        for i, q in enumerate(params):
            torch_count = float(topt.state[tq[i]]["step"]) if tq[i] in topt.state else 0.0
            assert torch_count == count[i], (step, i)
            if q in opt.state and "step" in opt.state[q]:
                assert float(opt.state[q]["step"]) == torch_count, (step, i, float(opt.state[q]["step"]), torch_count)
            else:
                assert torch_count == 0
        if step == 2:  # a state_dict round trip after the third step, into a fresh optimiser
            sd = opt.state_dict()
            opt = FusedAdam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
            opt.load_state_dict(sd)
    assert count == [sum(_has_grad(s, i) for s in range(6)) for i in range(len(params))]
    assert len(set(count)) >= 3 and len(keep) > 16
    print(f"host logic: dp {worst[0]:.2f}/{worst[1]:.2f}")


# ---- (c) the Adam update inside the fused training step -----------------------------------------------------------------
def _rand_params(rng, D0, D1, D2):
    k1, k2 = 1 / np.sqrt(D0), 1 / np.sqrt(D1)
    return [rng.uniform(-k1, k1, (D1, D0)).astype(np.float32), rng.uniform(-k1, k1, D1).astype(np.float32),
            rng.uniform(-k2, k2, (D2, D1)).astype(np.float32), rng.uniform(-k2, k2, D2).astype(np.float32),
            rng.uniform(0, 1, D2).astype(np.float32), rng.uniform(0, 1, D2).astype(np.float32)]


@pytest.mark.parametrize("lossname", ["SoftCdet", "crossentropy"])
@pytest.mark.parametrize("D,B", [(150, 1003), (170, 1003), (150, 4096), (170, 4096)])
def test_fused_train_step_updates(hip_lib, lossname, D, B):
    """ops.train_step, three consecutive steps (t = 1, 2, 3): after each, the device's OWN gradient (grad_out: the flat
    gradient of the six tensors, then dL/dtheta) goes to adam_ref together with the parameters and moments the step started
    from; the six tensors, the thresholds (updated in the loss tail, whose step count the small-batch kernel has already
    bumped) and m / v are gated in fp32 units, and the refreshed packed image equals ops.pack_params of the updated tensors
    bit for bit.  (150 / 170: the two kernel families; 1003: the 8-pair half-tile kernel with a ragged tile, 4096: the 16-pair one.)"""
    from neuralplda_amd import ops
    hp = HYPER["default"]
    rng = np.random.default_rng(10 * D + B)
    prm = [torch.from_numpy(a).cuda() for a in _rand_params(rng, 512, D, D)]
    kind = ops.LOSS_SOFTCDET if lossname == "SoftCdet" else ops.LOSS_BCE
    theta = [-0.4, -0.2] if kind == ops.LOSS_SOFTCDET else [0.1]
    betas, alpha = ([99.0, 199.0], 15.0) if kind == ops.LOSS_SOFTCDET else ([], 0.0)
    ths = [torch.tensor([x], device="cuda") for x in theta]
    K = len(ths)
    packed = ops.pack_params(*prm)
    sizes = [q.numel() for q in prm] + [1] * K
    n = sum(sizes) - K
    m, v, step = torch.zeros(n + K, device="cuda"), torch.zeros(n + K, device="cuda"), torch.zeros(2, device="cuda")
    out, lbuf = torch.zeros(n + K, device="cuda"), torch.zeros((), device="cuda")
    ws = ops.train_step_workspace(B, packed)
    classes = [0, 0, 0, 0, 1, 1] + [2] * K  # weights and biases ~ 0.04, P_sqrt / Q ~ 0.5, thresholds
    split = lambda a: np.split(a, np.cumsum(sizes)[:-1])  # noqa: E731
    worst = [0.0, 0.0]
    for it in range(3):
        x1 = torch.from_numpy(rng.standard_normal((B, 512)).astype(np.float32)).cuda()
        x2 = torch.from_numpy(rng.standard_normal((B, 512)).astype(np.float32)).cuda()
        t = (rng.random(B) < 0.3).astype(np.float32)
        t[0], t[-1] = 1.0, 0.0
        p0 = [q.cpu().numpy().reshape(-1).copy() for q in prm + ths]
        m0, v0 = split(m.cpu().numpy()), split(v.cpu().numpy())
        ops.train_step(x1, x2, torch.from_numpy(t).cuda(), prm, ths, betas, alpha, kind, m, v, step, *hp, packed, ws, lbuf,
                       grad_out=out)
        torch.cuda.synchronize()
        assert step[0].item() == it + 1.0
        g = split(out.cpu().numpy())
        m1, v1 = split(m.cpu().numpy()), split(v.cpu().numpy())
        state = [(p0[i], g[i], m0[i], v0[i]) for i in range(6 + K)]
        got = [(q.cpu().numpy().reshape(-1), m1[i], v1[i]) for i, q in enumerate(prm + ths)]
        w = check_tensors(state, got, it + 1, hp, f"train_step {lossname} D={D} B={B} step {it + 1}", classes=classes)
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        fresh = ops.pack_params(*prm)
        assert torch.equal(packed.buf, fresh.buf), f"step {it + 1}: the packed image is not that of the updated tensors"
    print(f"train_step {lossname} D={D} B={B}: dp {worst[0]:.2f}/{worst[1]:.2f}")


@pytest.mark.parametrize("form", ["dplda_update", "dplda_update_loss"])
@pytest.mark.parametrize("D1,B", [(24, 100), (170, 777)])
def test_dplda_update_steps(hip_lib, form, D1, B):
    """The DPlda update (csrc/nplda_moments.hip: gradient fold + Adam per element of [weight | bias], the K thresholds in the
    same launch), three consecutive steps: the applied gradient the call reports (grad_out) and the dL/dtheta it was given
    (dplda_update) or formed itself (dplda_update_loss) go to adam_ref with the state the step started from."""
    from neuralplda_amd import ops
    hp = HYPER["default"]
    rng = np.random.default_rng(D1 + B)
    K = 2
    n = 2 * D1 * D1 + D1
    wlr = torch.from_numpy((0.05 * rng.standard_normal(n)).astype(np.float32)).cuda()
    blr = torch.from_numpy(np.array([0.3], np.float32)).cuda()
    ths = [torch.tensor([x], dtype=torch.float32, device="cuda") for x in (-0.8, -0.6)]
    m, v, step = torch.zeros(n + 1 + K, device="cuda"), torch.zeros(n + 1 + K, device="cuda"), torch.zeros(2, device="cuda")
    gout = torch.zeros(n + 1, device="cuda")
    sizes = [n, 1] + [1] * K
    split = lambda a: np.split(a, np.cumsum(sizes)[:-1])  # noqa: E731
    worst = [0.0, 0.0]
    for it in range(3):
        paired = torch.from_numpy(rng.standard_normal((B, 2 * D1)).astype(np.float32)).cuda()
        s = (rng.standard_normal(B) * 2.5 - 1).astype(np.float32)
        t = (rng.random(B) < 0.15).astype(np.float32)
        t[0], t[1] = 1.0, 0.0
        p0 = [q.cpu().numpy().reshape(-1).copy() for q in [wlr, blr] + ths]
        m0, v0 = split(m.cpu().numpy()), split(v.cpu().numpy())
        if form == "dplda_update":
            g = torch.from_numpy((rng.standard_normal(B) / B).astype(np.float32)).cuda()
            dth = torch.from_numpy((1e-2 * rng.standard_normal(K)).astype(np.float32)).cuda()
            ops.dplda_update(paired, g, wlr, blr, m, v, step, *hp, thetas=ths, dtheta=dth, grad_out=gout)
        else:
            res = ops.dplda_update_loss(paired, torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), ths, [99.0, 199.0], 15.0,
                                        ops.LOSS_SOFTCDET, wlr, blr, m, v, step, *hp, thetas=ths, grad_out=gout)
            assert res is not None
            dth = res[1]
        torch.cuda.synchronize()
        assert step[0].item() == it + 1.0
        ga = gout.cpu().numpy()
        grads = [ga[:n], ga[n:]] + [x.reshape(1) for x in dth.cpu().numpy()[:K]]
        m1, v1 = split(m.cpu().numpy()), split(v.cpu().numpy())
        state = [(p0[i], grads[i], m0[i], v0[i]) for i in range(2 + K)]
        got = [(q.cpu().numpy().reshape(-1), m1[i], v1[i]) for i, q in enumerate([wlr, blr] + ths)]
        w = check_tensors(state, got, it + 1, hp, f"{form} D1={D1} B={B} step {it + 1}", classes=[0, 1] + [1] * K)
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    print(f"{form} D1={D1} B={B}: dp {worst[0]:.2f}/{worst[1]:.2f}")
