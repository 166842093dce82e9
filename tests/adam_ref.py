"""torch.optim.Adam's element update in numpy (a plain helper of the Adam tests, not a conftest).

L2 weight decay folded into the gradient, bias-corrected moments, eps added to the root, no amsgrad:

    g' = g + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g' g'
    p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

`dtype=np.float64` is the reference, `dtype=np.float32` the unit of tests/fp32_units.py (every element operation rounded to
float32).  The hyper-parameters are the float32 values the C ABI receives.  The bias corrections 1 - beta^t are scalars that
torch evaluates in double on the host, so BOTH precisions take them from float64 and only round the two derived constants
(lr / bc1, 1 / sqrt(bc2)) to `dtype`: an implementation that forms 1 - beta^t in float32 then shows as an error in these
units, which is the point.
"""
import numpy as np


def step(p, g, m, v, t, lr, b1, b2, eps, wd, dtype=np.float64):
    """One update at step count t (steps taken including this one) -> (p', m', v') in `dtype`."""
    c = lambda x: dtype(np.float32(x))  # noqa: E731
    lr_, b1_, b2_, eps_, wd_ = (c(x) for x in (lr, b1, b2, eps, wd))
    p, g, m, v = (np.asarray(a).astype(dtype) for a in (p, g, m, v))
    bc1 = 1.0 - float(np.float32(b1)) ** int(t)
    bc2 = 1.0 - float(np.float32(b2)) ** int(t)
    step_size, inv_sqrt_bc2 = dtype(float(np.float32(lr)) / bc1), dtype(bc2 ** -0.5)
    one = dtype(1)
    gg = wd_ * p + g
    m2 = b1_ * m + (one - b1_) * gg
    v2 = b2_ * v + ((one - b2_) * gg) * gg
    den = np.sqrt(v2) * inv_sqrt_bc2 + eps_
    return (p - step_size * (m2 / den)).astype(dtype), m2.astype(dtype), v2.astype(dtype)


U = 2.0 ** -24  # unit roundoff of float32


def bounds(p, g, m, v, t, lr, b1, b2, eps, wd):
    """Worst-case float32 rounding error of (p', m', v'), per element, to first order in u = 2^-24 with 1 % on top: what any
    float32 evaluation of the formulas above stays inside (with or without fused multiply-adds), given exact bias
    corrections.  Used where there are too few values for a ratio in fp32 units to be a statistic.
      g'  = wd p + g                    a product and a sum:           dg <= u (|wd p| + |g'|)
      m'  = b1 m + ((1 - b1) g')        1 - b1, two products, a sum:   dm <= (1 - b1) dg + u (2 (1 - b1) |g'| + |b1 m| + |m'|)
      v'  = b2 v + ((1 - b2) g') g'     1 - b2, three products, a sum: dv <= 2 (1 - b2) |g'| dg + u (3 (1 - b2) g'^2 + b2 v + v')
      r   = sqrt(v')                                                   dr <= dv / (2 r) + u r
      den = r c2 + eps                  c2 rounded, a product, a sum:  dden <= c2 dr + u (2 r c2 + den)
      q   = m' / den                                                   dq <= dm / den + |q| dden / den + u |q|
      p'  = p - c1 q                    c1 rounded, a product, a sum:  dp' <= c1 dq + 2 u c1 |q| + u |p'|
    (the last term, half an ulp of the stored p', dominates for |p| >> lr)."""
    f = lambda x: float(np.float32(x))  # noqa: E731
    lr, b1, b2, eps, wd = (f(x) for x in (lr, b1, b2, eps, wd))
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    c1, c2 = lr / (1.0 - b1 ** int(t)), (1.0 - b2 ** int(t)) ** -0.5
    gg = wd * p + g
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    r = np.sqrt(v2)
    den = r * c2 + eps
    q = m2 / den
    p2 = p - c1 * q
    dg = U * (np.abs(wd * p) + np.abs(gg))
    dm = (1 - b1) * dg + U * (2 * (1 - b1) * np.abs(gg) + np.abs(b1 * m) + np.abs(m2))
    dv = 2 * (1 - b2) * np.abs(gg) * dg + U * (3 * (1 - b2) * gg * gg + b2 * v + v2)
    dr = np.divide(dv, 2 * r, out=np.zeros_like(r), where=r > 0) + U * r
    dden = c2 * dr + U * (2 * r * c2 + den)
    dq = dm / den + np.abs(q) * dden / den + U * np.abs(q)
    dp = c1 * dq + 2 * U * c1 * np.abs(q) + U * np.abs(p2)
    tiny = 2.0 ** -126  # (one denormal step, should a term underflow)
    return 1.01 * dp + tiny, 1.01 * dm + tiny, 1.01 * dv + tiny


class Driver:
    """Several parameters over several steps with per-parameter step counts, as torch counts them: a parameter whose
    gradient is None is skipped and does not count the step.  State is kept in `dtype`."""

    def __init__(self, params, lr, b1, b2, eps, wd, dtype=np.float64):
        self.hp = (lr, b1, b2, eps, wd)
        self.dtype = dtype
        self.p = [np.asarray(a).astype(dtype) for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t = [0] * len(self.p)

    def load(self, i, p=None, m=None, v=None, t=None):
        for name, val in (("p", p), ("m", m), ("v", v)):
            if val is not None:
                getattr(self, name)[i] = np.asarray(val).astype(self.dtype)
        if t is not None:
            self.t[i] = int(t)

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.t[i] += 1
            self.p[i], self.m[i], self.v[i] = step(self.p[i], g, self.m[i], self.v[i], self.t[i], *self.hp, dtype=self.dtype)
