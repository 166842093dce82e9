// nplda_xvec_bn.hip — the E-TDNN extractor trained with batch-statistics batch norm (gfx950): forward and backward of
// XVectorNet_ETDNN_12Layer.extract (utils/models.py:170-186) under a plain model.train(), where each tdnn is unfold,
// Linear, ReLU, nn.BatchNorm1d(affine=False) on the statistics of the batch (utils/models.py:90-93).  The GEMMs, the
// weight gradient, the bias sums, pooling and lin11 are those of the running-statistics path (nplda_xvec_body.h,
// nplda_xvec_bwd.hip), reached through the chains of nplda_xvec_train.h; this file adds the memory-bound part around
// them (design/k27_xvec_batch_stats.md) and keeps its own two layer loops.
//
// V_l = rows whose index inside their utterance is < T_u - ctx_l (rem[row] > ctx_l), n_l = |V_l|.
//
//  * xvbn_gemm_kernel<EpiTrainRaw>  layer forward: stores R_l = ReLU(y + b) un-normalised and the ReLU mask byte ANDed
//                                   with the row's validity.
//  * xvbn_sums_kernel<false>        per column, fp64 sum and sum of squares of R_l over V_l: fixed row splits, four waves
//                                   of a block take rows r0 + wave, r0 + wave + 4, ..., combined in wave order.
//  * xvbn_stats_finish_kernel       sums the splits (eight runs of consecutive splits, each in split order, then the runs
//                                   in run order): mu_l, s_l = 1 / sqrt(v_l + eps) (fp64, rounded once), and for the
//                                   host the mean, the unbiased variance and n_l.
//  * xvbn_norm_kernel               O_l = (R_l - mu_l) s_l in place over the live rows, 16 bytes per lane.
//  * xvbn_gemm_kernel<EpiStore>     data gradient G_{l-1} = sum_j dA_l[t - j d] W_l[:, tap j], stored raw.
//  * xvbn_pool_bwd_kernel           statistics-pooling backward, raw: G_10 on V_10 (the caller zeroes the other rows).
//  * xvbn_sums_kernel<true>         per column, fp64 sums of G_l and of G_l O_l over V_l (one pass over both).
//  * xvbn_pair_finish_kernel        a_l, c_l = those sums / n_l.
//  * xvbn_apply_kernel              dA_l = mask_l ? s_l (G_l - a_l - O_l c_l) : 0, in place over G_l.
//
// No atomics; every sum has a fixed partition and order, so two calls give the same bits.
#include "nplda_xvec_train.h"

namespace {

using namespace nplda_xvec_train;

constexpr int kBnSplits = 512;    // row splits of the column statistics at most
constexpr int kBnSplitRows = 64;  // rows per split at least
constexpr int kBnCols = 256;      // columns per block of the sums kernels: 64 lanes x 4
constexpr int kBnRows = 16;       // rows per block of the element-wise kernels: 4 waves x 4

inline int bn_splits(long long live) {
    const long long want = (live + kBnSplitRows - 1) / kBnSplitRows;
    return want < 1 ? 1 : (want > kBnSplits ? kBnSplits : (int)want);
}

inline size_t stats_offset(int l) {  // floats: mean[out_ld] then unbiased var[out_ld] per layer
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += 2 * (size_t)out_ld(i);
    return o;
}
inline size_t stats_bytes() { return stats_offset(kTdnn) * 4 + (size_t)kTdnn * 8; }

struct BnSavedLayout {
    SavedLayout base;
    size_t oMu[kTdnn], oInv[kTdnn], oPart, oCnt, total;  // bytes
    int S;
};

BnSavedLayout bn_saved_layout(long long R, long long U) {
    BnSavedLayout b;
    b.base = saved_layout(R, U);
    b.S = bn_splits(b.base.live);
    size_t o = b.base.total;
    for (int l = 0; l < kTdnn; ++l) {
        b.oMu[l] = o;
        o = align256(o + (size_t)out_ld(l) * 4);
        b.oInv[l] = o;
        o = align256(o + (size_t)out_ld(l) * 4);
    }
    b.oPart = o;
    o = align256(o + (size_t)b.S * 2 * out_ld(kTdnn - 1) * 8);
    b.oCnt = o;
    b.total = align256(o + (size_t)b.S * 8);
    return b;
}

struct BnWsLayout {
    WsLayoutB base;
    size_t oAC, oPart, oCnt, total;  // bytes
    int S;
};

BnWsLayout bn_bwd_layout(long long R, long long U) {
    BnWsLayout w;
    w.base = bwd_layout(R, U);
    w.S = bn_splits(saved_layout(R, U).live);
    size_t o = w.base.total;
    w.oAC = o;
    o = align256(o + 2 * (size_t)out_ld(kTdnn - 1) * 4);
    w.oPart = o;
    o = align256(o + (size_t)w.S * 2 * out_ld(kTdnn - 1) * 8);
    w.oCnt = o;
    w.total = align256(o + (size_t)w.S * 8);
    return w;
}

// every layer needs two valid rows at least (n_l = R - U ctx_l when every utterance is longer than 22 frames)
inline bool enough_rows(long long R, long long U) { return R - U * (long long)kCtx[kTdnn - 1] >= 2; }

// ---- epilogues -------------------------------------------------------------------------------------------------

struct EpiTrainRaw {
    uint8_t* mask;
    long long ldm;
    const int* rem;
    int ctx;
    __device__ __forceinline__ void operator()(const GemmArgs& a, long long row, int col, f32x4 v) const {
        v = v + *reinterpret_cast<const f32x4*>(a.bias + col);
        const bool valid = rem[row] > ctx;
        unsigned mk = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (valid && v[c] > 0.f) mk |= 1u << (8 * c);
            v[c] = fmaxf(v[c], 0.f);
        }
        *reinterpret_cast<f32x4*>(a.out + row * a.ld_out + col) = v;
        *reinterpret_cast<unsigned*>(mask + row * ldm + col) = mk;
    }
};

struct EpiStore {
    __device__ __forceinline__ void operator()(const GemmArgs& a, long long row, int col, f32x4 v) const {
        *reinterpret_cast<f32x4*>(a.out + row * a.ld_out + col) = v;
    }
};

template <class Epi>
__global__ __launch_bounds__(256, 2) void xvbn_gemm_kernel(const GemmArgs a, const Epi e) {
    xvec_gemm_body(a, e);
}

// ---- column sums over V_l ----------------------------------------------------------------------------------------

// part[(2 split + k) N + col]: k = 0 the sum of x, k = 1 the sum of x x (kPair: x y); cnt[split] = valid rows of the split
template <bool kPair>
__global__ __launch_bounds__(256) void xvbn_sums_kernel(const float* __restrict__ x, long long ldx,
                                                         const float* __restrict__ y, long long ldy,
                                                         const int* __restrict__ rem, int ctx, long long nrows,
                                                         long long rps, int N, double* __restrict__ part,
                                                         long long* __restrict__ cnt) {
    __shared__ double red[3][8][64];
    __shared__ long long rc[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * kBnCols + 4 * lane;
    const bool active = col < N;
    const long long r0 = (long long)blockIdx.y * rps, r1 = r0 + rps < nrows ? r0 + rps : nrows;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    long long n = 0;
    if (active) {
#pragma unroll 4
        for (long long r = r0 + wave; r < r1; r += 4) {
            const bool valid = rem[r] > ctx;
            const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * ldx + col);
            f32x4 b = a;
            if (kPair) b = *reinterpret_cast<const f32x4*>(y + r * ldy + col);
            if (valid) {
                ++n;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    s[c] += (double)a[c];
                    q[c] += (double)a[c] * (double)b[c];
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            red[wave - 1][c][lane] = s[c];
            red[wave - 1][4 + c][lane] = q[c];
        }
        if (lane == 0) rc[wave - 1] = n;
    }
    __syncthreads();
    if (wave == 0 && active) {
        for (int w = 0; w < 3; ++w) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s[c] += red[w][c][lane];
                q[c] += red[w][4 + c][lane];
            }
        }
        double* ps = part + (size_t)(2 * blockIdx.y) * N + col;
        double* pq = ps + N;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            ps[c] = s[c];
            pq[c] = q[c];
        }
        if (blockIdx.x == 0 && lane == 0) cnt[blockIdx.y] = n + rc[0] + rc[1] + rc[2];
    }
}

// Sums one column's partials over the splits: eight lanes of the block take consecutive runs of the splits, each in
// split order, and lane 0 adds the eight run sums in run order (a fixed tree: the same bits every call, and 64 dependent
// additions in a row where one thread over 512 splits spends 160 us on load latency).  True for the thread that holds a
// column's totals.
constexpr int kFinCols = 32, kFinRuns = 8;

__device__ __forceinline__ bool xvbn_reduce_splits(const double* __restrict__ part, const long long* __restrict__ cnt,
                                                   int S, int N, int& col, double& s, double& q, long long& n) {
    __shared__ double rs[kFinRuns][kFinCols], rq[kFinRuns][kFinCols];
    __shared__ long long rn[kFinRuns][kFinCols];
    const int c = threadIdx.x % kFinCols, g = threadIdx.x / kFinCols;
    col = blockIdx.x * kFinCols + c;
    const int run = (S + kFinRuns - 1) / kFinRuns, i0 = g * run, i1 = i0 + run < S ? i0 + run : S;
    s = 0.0;
    q = 0.0;
    n = 0;
    if (col < N) {
#pragma unroll 8
        for (int i = i0; i < i1; ++i) {
            n += cnt[i];
            s += part[(size_t)(2 * i) * N + col];
            q += part[(size_t)(2 * i + 1) * N + col];
        }
    }
    rs[g][c] = s;
    rq[g][c] = q;
    rn[g][c] = n;
    __syncthreads();
    if (g != 0 || col >= N) return false;
    for (int w = 1; w < kFinRuns; ++w) {
        s += rs[w][c];
        q += rq[w][c];
        n += rn[w][c];
    }
    return true;
}

__global__ __launch_bounds__(kFinCols * kFinRuns) void xvbn_stats_finish_kernel(
    const double* __restrict__ part, const long long* __restrict__ cnt, int S, int N, float eps, float* __restrict__ mu,
    float* __restrict__ inv, float* __restrict__ tmean, float* __restrict__ tvar, long long* __restrict__ tcount) {
    int col;
    long long n;
    double s, q;
    if (!xvbn_reduce_splits(part, cnt, S, N, col, s, q, n)) return;
    const double mean = s / (double)n;
    double var = q / (double)n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    mu[col] = (float)mean;
    inv[col] = (float)(1.0 / sqrt(var + (double)eps));
    tmean[col] = (float)mean;
    tvar[col] = (float)(var * ((double)n / (double)(n - 1)));
    if (col == 0) *tcount = n;
}

__global__ __launch_bounds__(kFinCols * kFinRuns) void xvbn_pair_finish_kernel(
    const double* __restrict__ part, const long long* __restrict__ cnt, int S, int N, float* __restrict__ a,
    float* __restrict__ c) {
    int col;
    long long n;
    double s, q;
    if (!xvbn_reduce_splits(part, cnt, S, N, col, s, q, n)) return;
    a[col] = (float)(s / (double)n);
    c[col] = (float)(q / (double)n);
}

// ---- element-wise kernels: block = 4 waves x 4 rows, lane = 4 columns -------------------------------------------------

__global__ __launch_bounds__(256) void xvbn_norm_kernel(float* __restrict__ o, long long ld, long long nrows, int N,
                                                         const float* __restrict__ mu, const float* __restrict__ inv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.y * kBnCols + 4 * lane;
    if (col >= N) return;
    const f32x4 m = *reinterpret_cast<const f32x4*>(mu + col), s = *reinterpret_cast<const f32x4*>(inv + col);
    const long long r0 = (long long)blockIdx.x * kBnRows + 4 * wave;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long r = r0 + i;
        if (r >= nrows) break;
        f32x4* p = reinterpret_cast<f32x4*>(o + r * ld + col);
        *p = (*p - m) * s;
    }
}

__global__ __launch_bounds__(256) void xvbn_apply_kernel(float* __restrict__ g, long long ldg,
                                                          const float* __restrict__ o, long long ldo,
                                                          const uint8_t* __restrict__ mask, long long ldm,
                                                          long long nrows, int N, const float* __restrict__ inv,
                                                          const float* __restrict__ av, const float* __restrict__ cv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.y * kBnCols + 4 * lane;
    if (col >= N) return;
    const f32x4 s = *reinterpret_cast<const f32x4*>(inv + col), a = *reinterpret_cast<const f32x4*>(av + col),
                c = *reinterpret_cast<const f32x4*>(cv + col);
    const long long r0 = (long long)blockIdx.x * kBnRows + 4 * wave;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long r = r0 + i;
        if (r >= nrows) break;
        f32x4* p = reinterpret_cast<f32x4*>(g + r * ldg + col);
        const f32x4 G = *p, O = *reinterpret_cast<const f32x4*>(o + r * ldo + col);
        const unsigned mk = *reinterpret_cast<const unsigned*>(mask + r * ldm + col);
        f32x4 d;
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = ((mk >> (8 * k)) & 0xffu) ? s[k] * (G[k] - a[k] - O[k] * c[k]) : 0.f;
        *p = d;
    }
}

__global__ __launch_bounds__(256) void xvbn_pool_bwd_kernel(const float* __restrict__ O10, long long ld,
                                                             const float* __restrict__ pooled,
                                                             const float* __restrict__ dpool,
                                                             const int64_t* __restrict__ offsets, long long R,
                                                             int pooling, float* __restrict__ G) {
    const long long u = blockIdx.x / kPoolBlocks;
    const int cb = (int)(blockIdx.x - u * kPoolBlocks), col = cb * 256 + threadIdx.x;
    if (col >= kPoolDim) return;
    long long b = offsets[u], e = offsets[u + 1];
    b = b < 0 ? 0 : (b > R ? R : b);
    e = e < b ? b : (e > R ? R : e);
    const long long n = e - b - kContext;
    const double mean = pooled[u * kPooledLd + col], sd = pooled[u * kPooledLd + kPoolDim + col];
    const double dm = dpool[u * kPooledLd + col], ds = dpool[u * kPooledLd + kPoolDim + col];
    const double a0 = dm / (double)n;
    // a channel whose pooled rows are all equal (a unit dead over a short utterance) has std 0: torch's std backward
    // passes 0 there, not 0 / 0.  (The running-statistics path masks G_10 by the ReLU branch, which hides such units;
    // here G_10 enters the column sums raw.)
    const double k = pooling == NPLDA_XVEC_POOL_VAR ? 2.0 * ds / (double)(n - 1)
                                                    : (sd > 0.0 ? ds / ((double)(n - 1) * sd) : 0.0);
    for (long long t = 0; t < n; ++t) {
        const long long off = (b + t) * ld + col;
        G[off] = (float)(a0 + k * ((double)O10[off] - mean));
    }
}

// ---- host helpers ----------------------------------------------------------------------------------------------

template <bool kPair>
int launch_sums(const float* x, long long ldx, const float* y, long long ldy, const int* rem, int ctx, long long nrows,
                int S, int N, double* part, long long* cnt, hipStream_t st) {
    const long long rps = (nrows + S - 1) / S;
    hipLaunchKernelGGL(xvbn_sums_kernel<kPair>, dim3((unsigned)((N + kBnCols - 1) / kBnCols), (unsigned)S), dim3(256), 0,
                       st, x, ldx, y, ldy, rem, ctx, nrows, rps, N, part, cnt);
    return nplda_launch_status();
}

inline dim3 rows_grid(long long nrows, int N) {
    return dim3((unsigned)((nrows + kBnRows - 1) / kBnRows), (unsigned)((N + kBnCols - 1) / kBnCols));
}

bool bad_sizes(int64_t n_utts, int64_t total_frames) {
    return n_utts > 0x7fffffffLL / kPoolBlocks || total_frames > 0x7fffffffLL * (long long)kBnRows - kRowsPerBlock;
}

}  // namespace

extern "C" {

size_t nplda_xvec_train_bn_saved_bytes(int64_t total_frames, int64_t n_utts) {
    if (total_frames < 0 || n_utts < 0) return 0;
    return bn_saved_layout(total_frames, n_utts).total;
}

size_t nplda_xvec_bn_stats_bytes(void) { return stats_bytes(); }

int nplda_xvec_bn_mask_layout(int64_t total_frames, int64_t n_utts, int layer, size_t* offset, int64_t* row_stride) {
    if (total_frames < 0 || n_utts < 0 || layer < 0 || layer >= kTdnn || !offset || !row_stride) return NPLDA_EINVAL;
    *offset = saved_layout(total_frames, n_utts).oM[layer];
    *row_stride = out_ld(layer);
    return NPLDA_OK;
}

int nplda_xvec_extract_train_bn_f32(const float* x, int layout, int64_t ld_in, const int64_t* offsets, int64_t n_utts,
                                    int64_t total_frames, int pooling, const void* packed, const float* eps, float* out,
                                    int64_t ldx, void* saved, size_t saved_bytes, void* stats, size_t stats_bytes_,
                                    nplda_stream_t stream) {
    bool nothing;
    const int bad = check_forward(n_utts, total_frames, layout, pooling, ld_in, ldx,
                                  {x, offsets, packed, eps, out, saved, stats}, {packed, out, saved, stats}, &nothing);
    if (bad || nothing) return bad;
    if (!enough_rows(total_frames, n_utts)) return NPLDA_EINVAL;
    if (bad_sizes(n_utts, total_frames)) return NPLDA_EUNSUPPORTED;
    const BnSavedLayout B = bn_saved_layout(total_frames, n_utts);
    const SavedLayout& L = B.base;
    if (saved_bytes < B.total || stats_bytes_ < stats_bytes()) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)saved;
    const int* rem = (const int*)(base + L.oRem);
    double* part = (double*)(base + B.oPart);
    long long* cnt = (long long*)(base + B.oCnt);
    float* table = (float*)stats;
    long long* counts = (long long*)((char*)stats + stats_offset(kTdnn) * 4);
    const float* P = (const float*)packed;
    if (int rc = train_forward_head(x, layout, ld_in, offsets, n_utts, total_frames, L, base, st)) return rc;
    const float* in = (const float*)(base + L.oX);
    long long ld = kFeatP;
    for (int l = 0; l < kTdnn; ++l) {
        const int N = out_ld(l);
        float* o = (float*)(base + L.oO[l]);
        float* mu = (float*)(base + B.oMu[l]);
        float* inv = (float*)(base + B.oInv[l]);
        const GemmArgs a = gemm_args(P, geomF(l), in, ld, o, N, L.live, kShape[l].d, 0);
        const EpiTrainRaw e{(uint8_t*)(base + L.oM[l]), (long long)N, rem, kCtx[l]};
        if (int rc = launch_gemm(xvbn_gemm_kernel<EpiTrainRaw>, a, L.live, st, e)) return rc;
        if (int rc = launch_sums<false>(o, N, o, N, rem, kCtx[l], L.live, B.S, N, part, cnt, st)) return rc;
        hipLaunchKernelGGL(xvbn_stats_finish_kernel, dim3((unsigned)((N + kFinCols - 1) / kFinCols)),
                           dim3(kFinCols * kFinRuns), 0, st, part, cnt, B.S,
                           N, eps[l], mu, inv, table + stats_offset(l), table + stats_offset(l) + N, counts + l);
        if (int rc = nplda_launch_status()) return rc;
        hipLaunchKernelGGL(xvbn_norm_kernel, rows_grid(L.live, N), dim3(256), 0, st, o, (long long)N, L.live, N, mu, inv);
        if (int rc = nplda_launch_status()) return rc;
        in = o;
        ld = N;
    }
    return train_forward_tail(P, offsets, n_utts, total_frames, pooling, L, base, out, ldx, st);
}

size_t nplda_xvec_backward_bn_workspace_bytes(int64_t total_frames, int64_t n_utts) {
    if (total_frames < 0 || n_utts < 0) return 0;
    return bn_bwd_layout(total_frames, n_utts).total;
}

int nplda_xvec_backward_bn_f32(const void* saved, size_t saved_bytes, const int64_t* offsets, int64_t n_utts,
                               int64_t total_frames, int pooling, const float* dxvec, int64_t lddx, const void* packed,
                               const void* packed_t, float* grad, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    bool nothing;
    const int bad = check_backward(n_utts, total_frames, pooling, lddx, saved, offsets, dxvec, packed, packed_t, grad, ws,
                                   &nothing);
    if (bad || nothing) return bad;
    if (!enough_rows(total_frames, n_utts)) return NPLDA_EINVAL;
    if (bad_sizes(n_utts, total_frames)) return NPLDA_EUNSUPPORTED;
    const BnSavedLayout B = bn_saved_layout(total_frames, n_utts);
    const SavedLayout& L = B.base;
    const BnWsLayout BW = bn_bwd_layout(total_frames, n_utts);
    if (saved_bytes < B.total || ws_bytes < BW.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const BwdBuffers b = bwd_buffers(L, BW.base, saved, ws);
    const char* sb = b.sb;
    char* wb = (char*)ws;
    const float* PT = (const float*)packed_t;
    float* av = (float*)(wb + BW.oAC);
    float* cv = av + out_ld(kTdnn - 1);
    double* spart = (double*)(wb + BW.oPart);
    long long* cnt = (long long*)(wb + BW.oCnt);
    const int* rem = (const int*)(sb + L.oRem);
    float* dA;
    long long ldA;
    if (int rc = backward_head(b, L, n_utts, dxvec, lddx, PT, grad, st, &dA, &ldA)) return rc;
    // tdnn10: pooling backward into G_10 (every other row zero)
    hipLaunchKernelGGL(xvbn_pool_bwd_kernel, dim3((unsigned)(n_utts * kPoolBlocks)), dim3(256), 0, st,
                       (const float*)(sb + L.oO[kTdnn - 1]), ldA, b.pooled, b.dpool, offsets, (long long)total_frames,
                       pooling, dA);
    if (int rc = nplda_launch_status()) return rc;
    for (int l = kTdnn - 1; l >= 0; --l) {
        const int N = out_ld(l);
        const float* O = (const float*)(sb + L.oO[l]);
        // batch-norm and ReLU backward in place: G_l -> dA_l
        if (int rc = launch_sums<true>(dA, ldA, O, N, rem, kCtx[l], L.live, BW.S, N, spart, cnt, st)) return rc;
        hipLaunchKernelGGL(xvbn_pair_finish_kernel, dim3((unsigned)((N + kFinCols - 1) / kFinCols)),
                           dim3(kFinCols * kFinRuns), 0, st, spart, cnt, BW.S,
                           N, av, cv);
        if (int rc = nplda_launch_status()) return rc;
        hipLaunchKernelGGL(xvbn_apply_kernel, rows_grid(L.live, N), dim3(256), 0, st, dA, ldA, O, (long long)N,
                           (const uint8_t*)(sb + L.oM[l]), (long long)N, L.live, N, (const float*)(sb + B.oInv[l]), av,
                           cv);
        if (int rc = nplda_launch_status()) return rc;
        if (int rc = layer_param_grads(l, dA, ldA, b, L, grad, st)) return rc;
        if (l == 0) break;
        const GemmArgs a = data_grad_args(l, PT, dA, ldA, b, L.live);
        if (int rc = launch_gemm(xvbn_gemm_kernel<EpiStore>, a, L.live, st, EpiStore{})) return rc;
        dA = a.out;
        ldA = a.ld_out;
    }
    return NPLDA_OK;
}

}  // extern "C"
