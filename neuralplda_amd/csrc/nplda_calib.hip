// Score calibration and fusion on gfx950 — counterpart of utils/score_calibration.py (Gaussian calibration) plus what
// the field uses in its place: prior-weighted linear logistic regression over K <= 8 systems, and the two metrics
// that only make sense for calibrated scores (Cllr, the cost at the Bayes threshold).  design/k16_calibration.md.
//
// Every sum over trials here is a fixed-order tree in fp64: a grid-stride loop per lane (the grid is a function of N
// alone), an xor butterfly over the 64 lanes of a wave, the four waves of a block through LDS, and a finishing kernel
// of one block over the <= kMaxBlocks block partials.  No floating-point atomics: the same input gives the same bits.
// Counts travel through the same tree as doubles (integers below 2^53 add exactly).
//
// The fit is a FIXED budget of (pass, finish + Newton step) launch pairs on the caller's stream, no host
// synchronisation, no device-side "until converged" loop: once the state's `done` word is set the remaining launches
// return at their first instruction.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nplda_trials.h"

namespace {

constexpr int kMaxK = 8;
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;                                       // 4 blocks of 256 on each of 256 CUs
constexpr int kMaxQ = 1 + (kMaxK + 1) + (kMaxK + 1) * (kMaxK + 2) / 2;  // J, g, upper triangle of H: 55
constexpr int kPartStride = 64;                                        // doubles per block partial (>= every NQ here)
constexpr int kMaxThr = 8;
constexpr int kMaxHalvings = 20;
constexpr int kMaxPasses = 256;
constexpr size_t kHeaderBytes = 4096;
constexpr long long kMaxN = 0x7fffffffll;

__host__ __device__ constexpr int nq_of(int K) { return 1 + (K + 1) + (K + 1) * (K + 2) / 2; }

// Head of the workspace.  Written by the kernels only; the host never reads it.
struct State {
    unsigned long long nt, nn;   // class counts (integer atomics: exact, order-free)
    double cur[kPartStride];     // finished sums of the last launch: J, g, H (l2 terms included) or the Gaussian sums
    double trial[kMaxK + 1];     // theta the next pass evaluates
    double acc[kMaxK + 1];       // last accepted theta
    double dir[kMaxK + 1];       // Newton direction at the accepted point
    double j_acc, ginf_acc, alpha;
    int halvings, iterations, passes;
    int done, converged, notfinite, stalled, have_acc;
};
static_assert(sizeof(State) <= kHeaderBytes, "state must fit the workspace header");

__host__ __device__ inline int blocks_for(long long n) {
    const long long b = (n + kBlock - 1) / kBlock;
    return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// lane -> wave -> block, fixed order; thread q < NQ of the block stores partial q
template <int NQ>
__device__ __forceinline__ void block_reduce_store(double (&v)[NQ], double* __restrict__ part_row) {
    __shared__ double red[kBlock / 64][NQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double x = wave_sum(v[q]);
        if (lane == 0) red[wave][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int q = threadIdx.x;
        part_row[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// one block of kBlock threads: sh[q] = sum over the block partials, q < nq; ends with a barrier
__device__ __forceinline__ void reduce_partials(const double* __restrict__ part, int nblocks, int nq, double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < nq; q += kBlock / 64) {
        double x = 0.0;
        for (int j = lane; j < nblocks; j += 64) x += part[(size_t)j * kPartStride + q];
        x = wave_sum(x);
        if (lane == 0) sh[q] = x;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void count_kernel(const float* __restrict__ t, long long n, State* st) {
    if (st->done) return;
    unsigned ct = 0, cn = 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const int l = trials::label_class(t[i]);  // 1 target, 0 non-target, -1 neither
        ct += l == 1;
        cn += l == 0;
    }
    ct = wave_sum(ct);
    cn = wave_sum(cn);
    if ((threadIdx.x & 63) == 0) {
        if (ct) atomicAdd(&st->nt, (unsigned long long)ct);
        if (cn) atomicAdd(&st->nn, (unsigned long long)cn);
    }
}

// ---- (a) the logistic pass -------------------------------------------------------------------------------------------
// z = a . x + b + tau; with e = exp(-|z|), r = 1 / (1 + e):  sigma = z >= 0 ? r : e r,  1 - sigma = z >= 0 ? e r : r,
// softplus(+-z) = max(+-z, 0) + log1p(e): one exp, one log1p and one division per trial, nothing overflows.
template <int K, typename T>
__global__ __launch_bounds__(kBlock) void pass_kernel(const T* __restrict__ X, long long n, long long ldx,
                                                      const float* __restrict__ t, const double* __restrict__ theta,
                                                      const State* __restrict__ st, double p_target, double tau,
                                                      double* __restrict__ part) {
    if (st->done) return;
    constexpr int NQ = nq_of(K);
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    double a[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) a[k] = theta[k];
    const double wt = p_target / (double)st->nt, wn = (1.0 - p_target) / (double)st->nn;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const int l = trials::label_class(t[i]);
        if (l < 0) continue;  // neither class: weight 0, the row is not read
        double x[K + 1];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = (double)X[i * ldx + k];
        x[K] = 1.0;
        double z = a[K] + tau;
#pragma unroll
        for (int k = 0; k < K; ++k) z = fma(a[k], x[k], z);
        const double e = exp(-fabs(z));
        const double r = 1.0 / (1.0 + e);
        const double er = e * r;
        const bool pos = z >= 0.0;
        const double sig = pos ? r : er, one_m = pos ? er : r;
        const double w = l ? wt : wn;
        const double sp = log1p(e) + fmax(l ? -z : z, 0.0);
        acc[0] += w * sp;
        const double gs = w * (l ? -one_m : sig);
        const double hs = w * (sig * one_m);
#pragma unroll
        for (int k = 0; k <= K; ++k) acc[1 + k] = fma(gs, x[k], acc[1 + k]);
#pragma unroll
        for (int j = 0; j <= K; ++j) {
            const double hx = hs * x[j];
#pragma unroll
            for (int k = j; k <= K; ++k) {
                const int q = K + 2 + j * (K + 1) - j * (j - 1) / 2 + (k - j);  // row j of the upper triangle
                acc[q] = fma(hx, x[k], acc[q]);
            }
        }
    }
    block_reduce_store<NQ>(acc, part + (size_t)blockIdx.x * kPartStride);
}

// cur = finished J, g, H with the ridge terms of the theta the pass used
__device__ __forceinline__ void finish_pass(const double* part, int nblocks, int K, const double* theta, double l2,
                                            double* cur) {
    reduce_partials(part, nblocks, nq_of(K), cur);
    if (threadIdx.x == 0) {
        double s2 = 0.0;
        int q = K + 2;
        for (int j = 0; j <= K; ++j) {
            if (j < K) {
                s2 = fma(theta[j], theta[j], s2);
                cur[1 + j] = fma(l2, theta[j], cur[1 + j]);
                cur[q] += l2;
            }
            q += K + 1 - j;
        }
        cur[0] = fma(0.5 * l2, s2, cur[0]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void pass_finish_kernel(State* st, const double* __restrict__ part, int nblocks,
                                                             int K, const double* __restrict__ theta, double l2,
                                                             double* __restrict__ out) {
    __shared__ double cur[kPartStride];
    finish_pass(part, nblocks, K, theta, l2, cur);
    const int nq = nq_of(K);
    if (threadIdx.x == 0) {
        out[0] = (double)st->nt;
        out[1] = (double)st->nn;
    }
    if (threadIdx.x < nq) out[2 + threadIdx.x] = cur[threadIdx.x];
}

// ---- (b) the Newton step ---------------------------------------------------------------------------------------------
// H d = g by Cholesky (H = L L^T from the packed upper triangle); false on a pivot that is not positive and finite
// (L: (kMaxK + 1)^2 doubles of LDS — indexed at run time, so not a register array)
__device__ bool solve_spd(const double* hu, const double* g, int n, double* d, double* L) {
    for (int j = 0; j < n; ++j)
        for (int k = j; k < n; ++k) L[k * n + j] = hu[j * n - j * (j - 1) / 2 + (k - j)];  // row j of the triangle
    for (int j = 0; j < n; ++j) {
        double s = L[j * n + j];
        for (int m = 0; m < j; ++m) s -= L[j * n + m] * L[j * n + m];
        if (!(s > 0.0) || !isfinite(s)) return false;
        const double piv = sqrt(s);
        L[j * n + j] = piv;
        for (int k = j + 1; k < n; ++k) {
            double v = L[k * n + j];
            for (int m = 0; m < j; ++m) v -= L[k * n + m] * L[j * n + m];
            L[k * n + j] = v / piv;
        }
    }
    for (int j = 0; j < n; ++j) {  // L y = g
        double v = g[j];
        for (int m = 0; m < j; ++m) v -= L[j * n + m] * d[m];
        d[j] = v / L[j * n + j];
    }
    for (int j = n - 1; j >= 0; --j) {  // L^T d = y
        double v = d[j];
        for (int m = j + 1; m < n; ++m) v -= L[m * n + j] * d[m];
        d[j] = v / L[j * n + j];
    }
    for (int j = 0; j < n; ++j)
        if (!isfinite(d[j])) return false;
    return true;
}

__device__ void write_report(const State* st, double* report) {
    report[0] = st->j_acc;
    report[1] = st->ginf_acc;
    report[2] = (double)st->iterations;
    report[3] = (double)st->passes;
    report[4] = (double)st->converged;
    report[5] = (double)st->notfinite;
    report[6] = (double)st->stalled;
    report[7] = (double)st->nt;
    report[8] = (double)st->nn;
    report[9] = st->alpha;
}

// One lane: judge the pass at `trial`, move `acc` / `theta` and choose the next trial.
__device__ void newton_step(State* st, int K, double tol, double* theta, double* report, double* chol) {
    const int n = K + 1, nq = nq_of(K);
    const double* cur = st->cur;
    st->passes += 1;
    bool finite = st->nt > 0 && st->nn > 0;
    for (int q = 0; q < nq; ++q) finite = finite && isfinite(cur[q]);
    if (!finite) {
        st->notfinite = 1;
        st->done = 1;
        write_report(st, report);
        return;
    }
    const double J = cur[0];
    // "did not increase": up to the rounding of the sum itself (a few ulp of J), so that a step whose true decrease is
    // below one ulp of J is not halved twenty times for noise
    const bool accept = !st->have_acc || J <= st->j_acc + 8.0 * 2.220446049250313e-16 * fabs(st->j_acc);
    if (accept) {
        double ginf = 0.0;
        for (int k = 0; k < n; ++k) {
            st->acc[k] = st->trial[k];
            theta[k] = st->trial[k];
            ginf = fmax(ginf, fabs(cur[1 + k]));
        }
        st->j_acc = J;
        st->ginf_acc = ginf;
        st->have_acc = 1;
        if (ginf <= tol) {
            st->converged = 1;
            st->done = 1;
            write_report(st, report);
            return;
        }
        if (!solve_spd(cur + 1 + n, cur + 1, n, st->dir, chol)) {
            st->notfinite = 1;
            st->done = 1;
            write_report(st, report);
            return;
        }
        st->alpha = 1.0;
        st->halvings = 0;
        st->iterations += 1;
    } else {
        if (st->halvings >= kMaxHalvings) {
            st->stalled = 1;
            st->done = 1;
            write_report(st, report);
            return;
        }
        st->halvings += 1;
        st->alpha *= 0.5;
    }
    for (int k = 0; k < n; ++k) st->trial[k] = st->acc[k] - st->alpha * st->dir[k];
    write_report(st, report);
}

__global__ __launch_bounds__(kBlock) void fit_finish_kernel(State* st, const double* __restrict__ part, int nblocks,
                                                            int K, double l2, double tol, double* theta,
                                                            double* report) {
    __shared__ double chol[(kMaxK + 1) * (kMaxK + 1)];
    if (st->done) return;
    finish_pass(part, nblocks, K, st->trial, l2, st->cur);
    if (threadIdx.x == 0) newton_step(st, K, tol, theta, report, chol);
}

__global__ void fit_init_kernel(State* st, int K, const double* __restrict__ theta, double* report) {
    if (threadIdx.x != 0) return;
    st->nt = st->nn = 0;
    for (int k = 0; k <= kMaxK; ++k) {
        const double v = k <= K ? theta[k] : 0.0;
        st->trial[k] = v;
        st->acc[k] = v;
        st->dir[k] = 0.0;
    }
    st->j_acc = st->ginf_acc = NAN;
    st->alpha = 1.0;
    st->halvings = st->iterations = st->passes = 0;
    st->done = st->converged = st->notfinite = st->stalled = st->have_acc = 0;
    write_report(st, report);
}

__global__ void clear_kernel(State* st) {
    if (threadIdx.x != 0) return;
    st->nt = st->nn = 0;
    st->done = 0;
}

// ---- (d) the Gaussian fit: sums, then squared deviations about the means (never sum s^2 - (sum s)^2 / n) ---------------
template <typename T>
__global__ __launch_bounds__(kBlock) void gauss_sum_kernel(const T* __restrict__ s, const float* __restrict__ t,
                                                           long long n, double* __restrict__ part) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // n_tgt, sum_tgt, n_non, sum_non
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const int l = trials::label_class(t[i]);
        if (l < 0) continue;
        const double v = (double)s[i];
        acc[0] += l ? 1.0 : 0.0;  // adding 0.0 is exact: both classes in straight-line code
        acc[1] += l ? v : 0.0;
        acc[2] += l ? 0.0 : 1.0;
        acc[3] += l ? 0.0 : v;
    }
    block_reduce_store<4>(acc, part + (size_t)blockIdx.x * kPartStride);
}

__global__ __launch_bounds__(kBlock) void gauss_mean_kernel(State* st, const double* __restrict__ part, int nblocks) {
    __shared__ double sh[4];
    reduce_partials(part, nblocks, 4, sh);
    if (threadIdx.x == 0) {
        st->cur[0] = sh[0];
        st->cur[1] = sh[1] / sh[0];
        st->cur[2] = sh[2];
        st->cur[3] = sh[3] / sh[2];
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gauss_dev_kernel(const T* __restrict__ s, const float* __restrict__ t,
                                                           long long n, const State* __restrict__ st,
                                                           double* __restrict__ part) {
    const double mt = st->cur[1], mn = st->cur[3];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // sum d_tgt, sum d_tgt^2, sum d_non, sum d_non^2
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const int l = trials::label_class(t[i]);
        if (l < 0) continue;
        const double v = (double)s[i];
        const double d = v - (l ? mt : mn);
        acc[0] += l ? d : 0.0;
        acc[1] = fma(l ? d : 0.0, d, acc[1]);
        acc[2] += l ? 0.0 : d;
        acc[3] = fma(l ? 0.0 : d, d, acc[3]);
    }
    block_reduce_store<4>(acc, part + (size_t)blockIdx.x * kPartStride);
}

// out: n_tgt, mean_tgt, std_tgt, n_non, mean_non, std_non; the first-order terms correct the rounding of the means
__global__ __launch_bounds__(kBlock) void gauss_finish_kernel(const State* st, const double* __restrict__ part,
                                                              int nblocks, double* __restrict__ out) {
    __shared__ double sh[4];
    reduce_partials(part, nblocks, 4, sh);
    if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        const double cnt = st->cur[2 * c], mean = st->cur[2 * c + 1];
        const double sd = sh[2 * c], sd2 = sh[2 * c + 1];
        const double var = (sd2 - sd * sd / cnt) / cnt;
        out[3 * c] = cnt;
        out[3 * c + 1] = mean + sd / cnt;
        out[3 * c + 2] = sqrt(fmax(var, 0.0));
    }
}

// ---- (e) apply -------------------------------------------------------------------------------------------------------
template <int K, typename T, typename O>
__global__ __launch_bounds__(kBlock) void apply_linear_kernel(const T* __restrict__ X, long long n, long long ldx,
                                                              const double* __restrict__ theta, O* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double z = theta[K];
#pragma unroll
    for (int k = 0; k < K; ++k) z = fma(theta[k], (double)X[i * ldx + k], z);
    out[i] = (O)z;
}

template <typename T, typename O>
__global__ __launch_bounds__(kBlock) void apply_gauss_kernel(const T* __restrict__ s, long long n, double mt, double st,
                                                             double mn, double sn, O* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double v = (double)s[i];
    const double dt = v - mt, dn = v - mn;
    out[i] = (O)(log(sn) - log(st) - dt * dt / (2.0 * st * st) + dn * dn / (2.0 * sn * sn));
}

// ---- (f) costs -------------------------------------------------------------------------------------------------------
struct Thresholds {
    double th[kMaxThr];
    int n;
};
constexpr int kCostQ = 4 + 2 * kMaxThr;  // n_tgt, n_non, sum_tgt softplus(-llr), sum_non softplus(llr), miss[], fa[]

template <typename T>
__global__ __launch_bounds__(kBlock) void costs_kernel(const T* __restrict__ llr, const float* __restrict__ t,
                                                       long long n, const Thresholds th, double* __restrict__ part) {
    double acc[kCostQ];
#pragma unroll
    for (int q = 0; q < kCostQ; ++q) acc[q] = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const int l = trials::label_class(t[i]);
        if (l < 0) continue;
        const double v = (double)llr[i];
        const double sp = log1p(exp(-fabs(v))) + fmax(l ? -v : v, 0.0);
        acc[0] += l ? 1.0 : 0.0;
        acc[1] += l ? 0.0 : 1.0;
        acc[2] += l ? sp : 0.0;
        acc[3] += l ? 0.0 : sp;
#pragma unroll
        for (int k = 0; k < kMaxThr; ++k) {
            if (k < th.n) {
                acc[4 + k] += (l && v < th.th[k]) ? 1.0 : 0.0;
                acc[4 + kMaxThr + k] += (!l && v >= th.th[k]) ? 1.0 : 0.0;
            }
        }
    }
    block_reduce_store<kCostQ>(acc, part + (size_t)blockIdx.x * kPartStride);
}

// counts: n_tgt, n_non, miss[nth], fa[nth]; sums: the two Cllr sums in bits
__global__ __launch_bounds__(kBlock) void costs_finish_kernel(const double* __restrict__ part, int nblocks, int nth,
                                                              long long* __restrict__ counts,
                                                              double* __restrict__ sums) {
    __shared__ double sh[kCostQ];
    reduce_partials(part, nblocks, kCostQ, sh);
    const int k = threadIdx.x;
    if (k < 2) {
        counts[k] = (long long)sh[k];
        sums[k] = sh[2 + k] * 1.4426950408889634;  // 1 / ln 2
    }
    if (k < nth) {
        counts[2 + k] = (long long)sh[4 + k];
        counts[2 + nth + k] = (long long)sh[4 + kMaxThr + k];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
size_t ws_bytes_for(long long n) { return kHeaderBytes + (size_t)blocks_for(n) * kPartStride * sizeof(double); }

int check_ws(const void* ws, size_t bytes, long long n) {
    if (!ws || !nplda_aligned16(ws)) return NPLDA_EINVAL;
    return bytes < ws_bytes_for(n) ? NPLDA_ENOSPC : NPLDA_OK;
}

int check_logreg(const void* X, int64_t N, int64_t ldx, int K, const void* target, const void* theta, double p_target,
                 double l2, const void* out, const void* ws, size_t ws_bytes) {
    if (K < 1 || K > kMaxK) return NPLDA_EUNSUPPORTED;
    if (!X || !target || !theta || !out || N < 2 || ldx < K) return NPLDA_EINVAL;
    if (!(p_target > 0.0 && p_target < 1.0) || !(l2 >= 0.0) || !std::isfinite(l2)) return NPLDA_EINVAL;
    if (N > kMaxN) return NPLDA_EUNSUPPORTED;
    return check_ws(ws, ws_bytes, N);
}

template <int K, typename T>
void launch_pass_k(int nb, hipStream_t s, const T* X, long long N, long long ldx, const float* t, const double* theta,
                   const State* st, double p, double tau, double* part) {
    hipLaunchKernelGGL((pass_kernel<K, T>), dim3(nb), dim3(kBlock), 0, s, X, N, ldx, t, theta, st, p, tau, part);
}

template <typename T>
void launch_pass(int K, int nb, hipStream_t s, const T* X, long long N, long long ldx, const float* t,
                 const double* theta, const State* st, double p, double tau, double* part) {
    switch (K) {
        case 1: launch_pass_k<1, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        case 2: launch_pass_k<2, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        case 3: launch_pass_k<3, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        case 4: launch_pass_k<4, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        case 5: launch_pass_k<5, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        case 6: launch_pass_k<6, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        case 7: launch_pass_k<7, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
        default: launch_pass_k<8, T>(nb, s, X, N, ldx, t, theta, st, p, tau, part); break;
    }
}

template <typename T>
int logreg_pass(const T* X, int64_t N, int64_t ldx, int K, const float* target, const double* theta, double p_target,
                double l2, double* out, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    if (int rc = check_logreg(X, N, ldx, K, target, theta, p_target, l2, out, ws, ws_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    State* st = (State*)ws;
    double* part = (double*)((char*)ws + kHeaderBytes);
    const int nb = blocks_for(N);
    hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(64), 0, s, st);
    hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kBlock), 0, s, target, (long long)N, st);
    launch_pass<T>(K, nb, s, X, N, ldx, target, theta, st, p_target, std::log(p_target) - std::log1p(-p_target), part);
    hipLaunchKernelGGL(pass_finish_kernel, dim3(1), dim3(kBlock), 0, s, st, (const double*)part, nb, K, theta, l2, out);
    return nplda_launch_status();
}

template <typename T>
int logreg_fit(const T* X, int64_t N, int64_t ldx, int K, const float* target, double* theta, double p_target,
               double l2, int max_passes, double tol, int resume, double* report, void* ws, size_t ws_bytes,
               nplda_stream_t stream) {
    if (int rc = check_logreg(X, N, ldx, K, target, theta, p_target, l2, report, ws, ws_bytes)) return rc;
    if (max_passes < 1 || max_passes > kMaxPasses || !(tol >= 0.0)) return NPLDA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    State* st = (State*)ws;
    double* part = (double*)((char*)ws + kHeaderBytes);
    const int nb = blocks_for(N);
    const double tau = std::log(p_target) - std::log1p(-p_target);
    if (!resume) {
        hipLaunchKernelGGL(fit_init_kernel, dim3(1), dim3(64), 0, s, st, K, (const double*)theta, report);
        hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kBlock), 0, s, target, (long long)N, st);
    }
    for (int p = 0; p < max_passes; ++p) {
        launch_pass<T>(K, nb, s, X, N, ldx, target, st->trial, st, p_target, tau, part);
        hipLaunchKernelGGL(fit_finish_kernel, dim3(1), dim3(kBlock), 0, s, st, (const double*)part, nb, K, l2, tol, theta,
                           report);
    }
    return nplda_launch_status();
}

template <typename T>
int gauss_fit(const T* scores, const float* target, int64_t N, double* out, void* ws, size_t ws_bytes,
              nplda_stream_t stream) {
    if (!scores || !target || !out || N < 2) return NPLDA_EINVAL;
    if (N > kMaxN) return NPLDA_EUNSUPPORTED;
    if (int rc = check_ws(ws, ws_bytes, N)) return rc;
    hipStream_t s = (hipStream_t)stream;
    State* st = (State*)ws;
    double* part = (double*)((char*)ws + kHeaderBytes);
    const int nb = blocks_for(N);
    hipLaunchKernelGGL((gauss_sum_kernel<T>), dim3(nb), dim3(kBlock), 0, s, scores, target, (long long)N, part);
    hipLaunchKernelGGL(gauss_mean_kernel, dim3(1), dim3(kBlock), 0, s, st, (const double*)part, nb);
    hipLaunchKernelGGL((gauss_dev_kernel<T>), dim3(nb), dim3(kBlock), 0, s, scores, target, (long long)N,
                       (const State*)st, part);
    hipLaunchKernelGGL(gauss_finish_kernel, dim3(1), dim3(kBlock), 0, s, (const State*)st, (const double*)part, nb, out);
    return nplda_launch_status();
}

template <int K, typename T>
void launch_apply_k(hipStream_t s, const T* X, long long N, long long ldx, const double* theta, void* out, int f64) {
    const dim3 grid((unsigned)((N + kBlock - 1) / kBlock));
    if (f64) hipLaunchKernelGGL((apply_linear_kernel<K, T, double>), grid, dim3(kBlock), 0, s, X, N, ldx, theta, (double*)out);
    else hipLaunchKernelGGL((apply_linear_kernel<K, T, float>), grid, dim3(kBlock), 0, s, X, N, ldx, theta, (float*)out);
}

template <typename T>
int apply_linear(const T* X, int64_t N, int64_t ldx, int K, const double* theta, void* out, int out_f64,
                 nplda_stream_t stream) {
    if (K < 1 || K > kMaxK) return NPLDA_EUNSUPPORTED;
    if (N < 0 || ldx < K || !theta) return NPLDA_EINVAL;
    if (N > kMaxN) return NPLDA_EUNSUPPORTED;
    if (N == 0) return NPLDA_OK;
    if (!X || !out) return NPLDA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (K) {
        case 1: launch_apply_k<1, T>(s, X, N, ldx, theta, out, out_f64); break;
        case 2: launch_apply_k<2, T>(s, X, N, ldx, theta, out, out_f64); break;
        case 3: launch_apply_k<3, T>(s, X, N, ldx, theta, out, out_f64); break;
        case 4: launch_apply_k<4, T>(s, X, N, ldx, theta, out, out_f64); break;
        case 5: launch_apply_k<5, T>(s, X, N, ldx, theta, out, out_f64); break;
        case 6: launch_apply_k<6, T>(s, X, N, ldx, theta, out, out_f64); break;
        case 7: launch_apply_k<7, T>(s, X, N, ldx, theta, out, out_f64); break;
        default: launch_apply_k<8, T>(s, X, N, ldx, theta, out, out_f64); break;
    }
    return nplda_launch_status();
}

template <typename T>
int apply_gauss(const T* scores, int64_t N, double mu_tgt, double std_tgt, double mu_imp, double std_imp, void* out,
                int out_f64, nplda_stream_t stream) {
    if (N < 0) return NPLDA_EINVAL;
    if (!(std_tgt > 0.0) || !(std_imp > 0.0) || !std::isfinite(std_tgt) || !std::isfinite(std_imp) ||
        !std::isfinite(mu_tgt) || !std::isfinite(mu_imp))
        return NPLDA_EINVAL;
    if (N > kMaxN) return NPLDA_EUNSUPPORTED;
    if (N == 0) return NPLDA_OK;
    if (!scores || !out) return NPLDA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + kBlock - 1) / kBlock));
    if (out_f64)
        hipLaunchKernelGGL((apply_gauss_kernel<T, double>), grid, dim3(kBlock), 0, s, scores, (long long)N, mu_tgt,
                           std_tgt, mu_imp, std_imp, (double*)out);
    else
        hipLaunchKernelGGL((apply_gauss_kernel<T, float>), grid, dim3(kBlock), 0, s, scores, (long long)N, mu_tgt, std_tgt,
                           mu_imp, std_imp, (float*)out);
    return nplda_launch_status();
}

template <typename T>
int costs(const T* llr, const float* target, int64_t N, const double* thresholds, int nth, int64_t* counts,
          double* sums, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    if (nth < 0 || nth > kMaxThr) return NPLDA_EUNSUPPORTED;
    if (!llr || !target || !counts || !sums || N < 1 || (nth > 0 && !thresholds)) return NPLDA_EINVAL;
    if (N > kMaxN) return NPLDA_EUNSUPPORTED;
    Thresholds th;
    th.n = nth;
    for (int k = 0; k < kMaxThr; ++k) {
        th.th[k] = k < nth ? thresholds[k] : 0.0;
        if (th.th[k] != th.th[k]) return NPLDA_EINVAL;  // a NaN threshold decides nothing
    }
    if (int rc = check_ws(ws, ws_bytes, N)) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)((char*)ws + kHeaderBytes);
    const int nb = blocks_for(N);
    hipLaunchKernelGGL((costs_kernel<T>), dim3(nb), dim3(kBlock), 0, s, llr, target, (long long)N, th, part);
    hipLaunchKernelGGL(costs_finish_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)part, nb, nth,
                       (long long*)counts, sums);
    return nplda_launch_status();
}

}  // namespace

extern "C" {

size_t nplda_calib_workspace_bytes(int64_t N, int K) {
    if (N < 2 || N > kMaxN || K < 1 || K > kMaxK) return 0;
    return ws_bytes_for(N);
}

int nplda_calib_sweep_rows(void) { return kMaxBlocks * kBlock; }

int nplda_calib_logreg_pass_f32(const float* X, int64_t N, int64_t ldx, int K, const float* target, const double* theta,
                                double p_target, double l2, double* out, void* workspace, size_t workspace_bytes,
                                nplda_stream_t stream) {
    return logreg_pass<float>(X, N, ldx, K, target, theta, p_target, l2, out, workspace, workspace_bytes, stream);
}
int nplda_calib_logreg_pass_f64(const double* X, int64_t N, int64_t ldx, int K, const float* target, const double* theta,
                                double p_target, double l2, double* out, void* workspace, size_t workspace_bytes,
                                nplda_stream_t stream) {
    return logreg_pass<double>(X, N, ldx, K, target, theta, p_target, l2, out, workspace, workspace_bytes, stream);
}

int nplda_calib_logreg_fit_f32(const float* X, int64_t N, int64_t ldx, int K, const float* target, double* theta,
                               double p_target, double l2, int max_passes, double tol, int resume, double* report,
                               void* workspace, size_t workspace_bytes, nplda_stream_t stream) {
    return logreg_fit<float>(X, N, ldx, K, target, theta, p_target, l2, max_passes, tol, resume, report, workspace,
                             workspace_bytes, stream);
}
int nplda_calib_logreg_fit_f64(const double* X, int64_t N, int64_t ldx, int K, const float* target, double* theta,
                               double p_target, double l2, int max_passes, double tol, int resume, double* report,
                               void* workspace, size_t workspace_bytes, nplda_stream_t stream) {
    return logreg_fit<double>(X, N, ldx, K, target, theta, p_target, l2, max_passes, tol, resume, report, workspace,
                              workspace_bytes, stream);
}

int nplda_calib_gauss_fit_f32(const float* scores, const float* target, int64_t N, double* out, void* workspace,
                              size_t workspace_bytes, nplda_stream_t stream) {
    return gauss_fit<float>(scores, target, N, out, workspace, workspace_bytes, stream);
}
int nplda_calib_gauss_fit_f64(const double* scores, const float* target, int64_t N, double* out, void* workspace,
                              size_t workspace_bytes, nplda_stream_t stream) {
    return gauss_fit<double>(scores, target, N, out, workspace, workspace_bytes, stream);
}

int nplda_calib_apply_linear_f32(const float* X, int64_t N, int64_t ldx, int K, const double* theta, void* out,
                                 int out_f64, nplda_stream_t stream) {
    return apply_linear<float>(X, N, ldx, K, theta, out, out_f64, stream);
}
int nplda_calib_apply_linear_f64(const double* X, int64_t N, int64_t ldx, int K, const double* theta, void* out,
                                 int out_f64, nplda_stream_t stream) {
    return apply_linear<double>(X, N, ldx, K, theta, out, out_f64, stream);
}

int nplda_calib_apply_gauss_f32(const float* scores, int64_t N, double mu_tgt, double std_tgt, double mu_imp,
                                double std_imp, void* out, int out_f64, nplda_stream_t stream) {
    return apply_gauss<float>(scores, N, mu_tgt, std_tgt, mu_imp, std_imp, out, out_f64, stream);
}
int nplda_calib_apply_gauss_f64(const double* scores, int64_t N, double mu_tgt, double std_tgt, double mu_imp,
                                double std_imp, void* out, int out_f64, nplda_stream_t stream) {
    return apply_gauss<double>(scores, N, mu_tgt, std_tgt, mu_imp, std_imp, out, out_f64, stream);
}

int nplda_calib_costs_f32(const float* llr, const float* target, int64_t N, const double* thresholds, int nth,
                          int64_t* counts, double* sums, void* workspace, size_t workspace_bytes, nplda_stream_t stream) {
    return costs<float>(llr, target, N, thresholds, nth, counts, sums, workspace, workspace_bytes, stream);
}
int nplda_calib_costs_f64(const double* llr, const float* target, int64_t N, const double* thresholds, int nth,
                          int64_t* counts, double* sums, void* workspace, size_t workspace_bytes, nplda_stream_t stream) {
    return costs<double>(llr, target, N, thresholds, nth, counts, sums, workspace, workspace_bytes, stream);
}

}  // extern "C"
