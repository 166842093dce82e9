// nplda_adam_math.h — torch.optim.Adam's element update (L2 weight decay folded into the gradient, bias-corrected
// moments, eps outside the square root, no amsgrad), shared by nplda_optim.hip and the fused training step.
#pragma once
#include "nplda_common.h"

namespace nplda_adam {

struct Consts { float beta1, beta2, eps, wd, step_size, inv_sqrt_bc2; };

// beta^t for a whole number t >= 1 by squaring, in double: 2 log2(t) products, no pow().  t is the launch's step counter
// (a float that holds a whole number below 2^24), so the loop runs at most 24 times and its trip count is the same for
// every thread of the launch: no divergence.
__device__ __forceinline__ double pow_whole(float beta, float t) {
    double r = 1.0, b = (double)beta;
    for (unsigned n = (unsigned)t; n; n >>= 1) {
        if (n & 1u) r *= b;
        b *= b;
    }
    return r;
}

// t = steps taken including this one.  The bias corrections 1 - beta^t are formed in double, as torch forms them on the
// host: in float32, 1.0f - powf(beta, t) cancels at small t (beta2 = 0.999, t = 2: 1 - 0.998001 keeps 14 bits), which put
// inv_sqrt_bc2 40-55 ulps off and the whole step's p' - p ~45 fp32 units (rms) off at t = 2, 3 (tests/test_adam_fp32_gpu.py).
__device__ __forceinline__ Consts consts_for(float t, float lr, float beta1, float beta2, float eps, float wd) {
    const double bc1 = 1.0 - pow_whole(beta1, t);
    const double bc2 = 1.0 - pow_whole(beta2, t);
    return Consts{beta1, beta2, eps, wd, (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2))};
}

// returns the updated parameter; m, v are updated in place.  Every contraction is spelled out: left to the compiler
// (fp-contract=fast) the two kernels this is inlined into fuse beta m + (1 - beta) g differently and their
// trajectories part in the last bit at the second step.
__device__ __forceinline__ float update(float p, float grad, float& m, float& v, const Consts& c) {
    const float g = fmaf(c.wd, p, grad);
    m = fmaf(c.beta1, m, (1.0f - c.beta1) * g);
    v = fmaf(c.beta2, v, ((1.0f - c.beta2) * g) * g);
    const float denom = fmaf(sqrtf(v), c.inv_sqrt_bc2, c.eps);
    return fmaf(-c.step_size, m / denom, p);
}

}  // namespace nplda_adam
