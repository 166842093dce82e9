// nplda_xvec_bwd.hip — backward through the E-TDNN x-vector extractor (gfx950, exact fp32 MFMA): the gradients of
// tdnn1..tdnn10 and lin11 (weight and bias) of XVectorNet_ETDNN_12Layer.extract (utils/models.py:170-186) with the tdnn
// batch norms on their running statistics (Etdnn_Xvec_NeuralPlda.train1, utils/models.py:238-249).  No dL/dMFCC.
//
//  * xvtr_gemm_kernel<EpiTrain>   the training forward: the extraction GEMM (nplda_xvec_body.h, same main loop and
//                                 epilogue arithmetic, so the x-vectors are extract()'s bit for bit) that also stores a
//                                 ReLU mask byte per output, taken from the pre-activation and ANDed with the row's
//                                 validity (index inside its utterance < T_u - ctx_l).  Every layer's normalised output,
//                                 the masks, the padded input image and the pooled rows stay in the caller's `saved`.
//  * xvtr_gemm_kernel<EpiBwd>     data gradient dO_{l-1}[t] = sum_j dA_l[t - j d] W_l[:, j Din:(j+1) Din]: the same
//                                 implicit gather at negative taps, A operand a second packed image of W per tap
//                                 transposed; epilogue dA_{l-1} = mask_{l-1} ? dO s_{l-1} : 0.  A row's taps outside its
//                                 utterance land on zeros (the previous utterance's invalid rows, or 16 zeroed leading
//                                 slack rows), so there is no per-tap bounds test.
//  * xvtr_gemm_kernel<EpiExtract> lin11 forward, and dpooled = dxvec W11 (bias-free transposed image).
//  * xvbwd_pool_kernel            statistics-pooling backward fused with tdnn10's ReLU / batch-norm backward: for the
//                                 n = T_u - 22 valid rows dO = dmean / n + dstd (O - mean) / ((n - 1) std) (var:
//                                 2 dvar (O - mean) / (n - 1)), then dA10 = mask10 ? dO s10 : 0 (fp64 arithmetic).
//  * xvbwd_wgrad_kernel           dW_l[o, j Din + i] = sum_t dA_l[t, o] O_{l-1}[t + j d, i]: both operands row-major in
//                                 frames, staged 16 frames at a time through double-buffered LDS, transposed on the way
//                                 in (rows of 24 floats: conflict-free ds_read_b128), 128 x 128 tile per block, split-K
//                                 over frames into per-split partials; xvbwd_reduce_kernel sums the splits in a fixed
//                                 order and writes torch layout (Dout, c Din).  No atomics: two calls give equal bits.
//  * xvbwd_colsum_kernel          bias gradients: per-split fp64 column sums, then a fixed-order finish.
// The host chains both training paths run around their own layer loops (nplda_xvec_train.h) are defined here, once.
#include "nplda_xvec_train.h"

namespace {

using namespace nplda_xvec_train;

constexpr int kWgLd = 24;     // LDS row stride (floats) of the transposed chunk

// ---- epilogues -------------------------------------------------------------------------------------------------

struct EpiTrain {
    uint8_t* mask;
    long long ldm;
    const int* rem;
    int ctx;
    __device__ __forceinline__ void operator()(const GemmArgs& a, long long row, int col, f32x4 v) const {
        v = v + *reinterpret_cast<const f32x4*>(a.bias + col);
        const f32x4 m = *reinterpret_cast<const f32x4*>(a.mean + col);
        const f32x4 s = *reinterpret_cast<const f32x4*>(a.inv + col);
        const bool valid = rem[row] > ctx;
        unsigned mk = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (valid && v[c] > 0.f) mk |= 1u << (8 * c);
            v[c] = (fmaxf(v[c], 0.f) - m[c]) * s[c];
        }
        *reinterpret_cast<f32x4*>(a.out + row * a.ld_out + col) = v;
        *reinterpret_cast<unsigned*>(mask + row * ldm + col) = mk;
    }
};

struct EpiBwd {
    const uint8_t* mask;
    long long ldm;
    const float* inv;
    __device__ __forceinline__ void operator()(const GemmArgs& a, long long row, int col, f32x4 v) const {
        const unsigned mk = *reinterpret_cast<const unsigned*>(mask + row * ldm + col);
        const f32x4 s = *reinterpret_cast<const f32x4*>(inv + col);
        f32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = ((mk >> (8 * c)) & 0xffu) ? v[c] * s[c] : 0.f;
        *reinterpret_cast<f32x4*>(a.out + row * a.ld_out + col) = o;
    }
};

template <class Epi>
__global__ __launch_bounds__(256, 2) void xvtr_gemm_kernel(const GemmArgs a, const Epi e) {
    xvec_gemm_body(a, e);
}

// ---- small kernels ---------------------------------------------------------------------------------------------

// frames left in the row's utterance (this one included), 0 outside every utterance
__global__ void xvtr_rem_kernel(const int64_t* __restrict__ offsets, long long U, long long R, long long rows,
                                int* __restrict__ rem) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int v = 0;
    if (r < R) {
        long long lo = 0, hi = U;  // largest u with offsets[u] <= r
        while (hi - lo > 1) {
            const long long mid = (lo + hi) / 2;
            if (offsets[mid] <= r) lo = mid; else hi = mid;
        }
        long long e = offsets[lo + 1];
        e = e > R ? R : e;
        const long long left = e - r;
        v = left <= 0 ? 0 : (left > (1 << 30) ? (1 << 30) : (int)left);
    }
    rem[r] = v;
}

__global__ void xvtr_pack_t_kernel(const float* __restrict__ W, int Din, int Dout, int c, int Doutp, int XBp,
                                   size_t total, float* __restrict__ frag) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const size_t blk = idx >> 8;
    const int xb = (int)(blk % XBp), kb = (int)(blk / XBp);
    const int n = 16 * xb + (lane & 15), kp = 16 * kb + 4 * (lane >> 4) + i;
    const int j = kp / Doutp, o = kp - j * Doutp;
    float v = 0.f;
    if (n < Din && j < c && o < Dout) v = W[(size_t)o * c * Din + (size_t)j * Din + n];
    frag[idx] = v;
}

__global__ void xvtr_fill_vec_kernel(int Nv, float* __restrict__ ob, float* __restrict__ om, float* __restrict__ oi) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Nv) return;
    ob[n] = 0.f;
    om[n] = 0.f;
    oi[n] = 1.f;
}

__global__ __launch_bounds__(256) void xvbwd_pool_kernel(const float* __restrict__ O10, long long ld,
                                                          const uint8_t* __restrict__ mask10,
                                                          const float* __restrict__ inv10,
                                                          const float* __restrict__ pooled,
                                                          const float* __restrict__ dpool,
                                                          const int64_t* __restrict__ offsets, long long R, int pooling,
                                                          float* __restrict__ dA) {
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
    const double k = pooling == NPLDA_XVEC_POOL_VAR ? 2.0 * ds / (double)(n - 1) : ds / ((double)(n - 1) * sd);
    const double s = inv10[col];
    for (long long t = 0; t < n; ++t) {
        const long long off = (b + t) * ld + col;
        const double d = a0 + k * ((double)O10[off] - mean);
        dA[off] = mask10[off] ? (float)(d * s) : 0.f;
    }
}

struct WgArgs {
    const float* a;  // dA rows [t][o]
    long long lda;
    int acols;       // columns of a that may be read
    const float* b;  // O_{l-1} rows [t][i]
    long long ldb;
    int Dinp, c, d;
    long long kmax, nchunks;
    int cps;
    float* part;     // [S][Mt 128][Nt 128]
    int Mp, Np;
};

__global__ __launch_bounds__(256, 2) void xvbwd_wgrad_kernel(const WgArgs w) {
    __shared__ float lds[2][2][128 * kWgLd];  // [buf][dA | O][row][frame], 48 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int o0 = blockIdx.y * 128, n0 = blockIdx.x * 128;
    const long long c0 = (long long)blockIdx.z * w.cps;
    const long long c1 = c0 + w.cps < w.nchunks ? c0 + w.cps : w.nchunks;
    f32x4 ra[2], rb[2];
    auto load = [&](long long ch) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + 256 * q, f = idx & 15, p = idx >> 4;
            const long long t = ch * kWgKC + f;
            const int o = o0 + 4 * p, n = n0 + 4 * p;
            const int jt = n / w.Dinp, i = n - jt * w.Dinp;
            ra[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            rb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < w.kmax && o + 4 <= w.acols) ra[q] = *reinterpret_cast<const f32x4*>(w.a + t * w.lda + o);
            if (t < w.kmax && jt < w.c)
                rb[q] = *reinterpret_cast<const f32x4*>(w.b + (t + (long long)jt * w.d) * w.ldb + i);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + 256 * q, f = idx & 15, p = idx >> 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                lds[buf][0][(4 * p + c) * kWgLd + f] = ra[q][c];
                lds[buf][1][(4 * p + c) * kWgLd + f] = rb[q][c];
            }
        }
    };
    f32x4 acc[2][8];
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[rg][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(c0);
    store(0);
    __syncthreads();
    for (long long ch = c0; ch < c1; ++ch) {
        const int buf = (int)((ch - c0) & 1);
        const bool more = ch + 1 < c1;
        if (more) load(ch + 1);
        f32x4 av[2], bv[8];
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
            av[rg] = *reinterpret_cast<const f32x4*>(&lds[buf][0][(32 * wave + 16 * rg + j) * kWgLd + 4 * g]);
#pragma unroll
        for (int u = 0; u < 8; ++u) bv[u] = *reinterpret_cast<const f32x4*>(&lds[buf][1][(16 * u + j) * kWgLd + 4 * g]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc[0][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[u][r], av[0][r], acc[0][u], 0, 0, 0);
                acc[1][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[u][r], av[1][r], acc[1][u], 0, 0, 0);
            }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
    // lane (j, g): dW[o = o0 + 32 wave + 16 rg + j][n0 + 16 u + 4 g + i]
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) {
        const int o = o0 + 32 * wave + 16 * rg + j;
        float* dst = w.part + ((size_t)blockIdx.z * w.Mp + o) * w.Np + n0 + 4 * g;
#pragma unroll
        for (int u = 0; u < 8; ++u) *reinterpret_cast<f32x4*>(dst + 16 * u) = acc[rg][u];
    }
}

__global__ void xvbwd_reduce_kernel(const float* __restrict__ part, int S, int Mp, int Np, int Dout, int Din, int Dinp,
                                    int c, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long K = (long long)c * Din;
    if (idx >= (long long)Dout * K) return;
    const int o = (int)(idx / K), k = (int)(idx - (long long)o * K);
    const int jt = k / Din, np = jt * Dinp + (k - jt * Din);
    const size_t stride = (size_t)Mp * Np;
    const float* p = part + (size_t)o * Np + np;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += p[i * stride];
    out[idx] = s;
}

__global__ void xvbwd_colsum_kernel(const float* __restrict__ a, long long lda, long long nrows, int N, long long rps,
                                    double* __restrict__ part) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    const long long r0 = (long long)blockIdx.y * rps, r1 = r0 + rps < nrows ? r0 + rps : nrows;
    double s = 0.0;
    for (long long r = r0; r < r1; ++r) s += (double)a[r * lda + col];
    part[(size_t)blockIdx.y * N + col] = s;
}

__global__ void xvbwd_colsum_finish_kernel(const double* __restrict__ part, int S, int N, float* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += part[(size_t)i * N + col];
    out[col] = (float)s;
}

// ---- host helpers ----------------------------------------------------------------------------------------------

// dW_l (torch layout) from dA rows and the layer's input rows: split-K partials in `part`, summed in split order
int launch_wgrad(int l, const float* A, long long lda, int acols, const float* B, long long ldb, long long kmax,
                 float* part, float* out, hipStream_t st) {
    const Layer s = kShape[l];
    const WgPlan p = wg_plan(l, kmax);
    WgArgs w;
    w.a = A; w.lda = lda; w.acols = acols; w.b = B; w.ldb = ldb;
    w.Dinp = round_up(s.Din, 16); w.c = s.c; w.d = s.d;
    w.kmax = kmax; w.nchunks = p.nchunks; w.cps = p.cps;
    w.part = part; w.Mp = p.Mt * 128; w.Np = p.Nt * 128;
    hipLaunchKernelGGL(xvbwd_wgrad_kernel, dim3((unsigned)p.Nt, (unsigned)p.Mt, (unsigned)p.S), dim3(256), 0, st, w);
    if (int rc = nplda_launch_status()) return rc;
    const long long total = (long long)s.Dout * s.c * s.Din;
    hipLaunchKernelGGL(xvbwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, p.S, w.Mp,
                       w.Np, s.Dout, s.Din, w.Dinp, s.c, out);
    return nplda_launch_status();
}

// out[col] = sum over nrows of A[:, col]: fp64 partials in `part` (kColSplits x N doubles at most), fixed order
int launch_colsum(const float* A, long long lda, long long nrows, int N, double* part, float* out, hipStream_t st) {
    const long long want = (nrows + 255) / 256;  // at least 256 rows per split
    const int S = want < 1 ? 1 : (want > kColSplits ? kColSplits : (int)want);
    const long long rps = (nrows + S - 1) / S;
    hipLaunchKernelGGL(xvbwd_colsum_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)S), dim3(256), 0, st, A, lda,
                       nrows, N, rps, part);
    if (int rc = nplda_launch_status()) return rc;
    hipLaunchKernelGGL(xvbwd_colsum_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, part, S, N, out);
    return nplda_launch_status();
}

}  // namespace

// ---- the chains both training paths run (nplda_xvec_train.h) -------------------------------------------------------

namespace nplda_xvec_train {

int train_forward_head(const float* x, int layout, long long ld_in, const int64_t* offsets, long long U, long long R,
                       const SavedLayout& L, char* saved, hipStream_t st) {
    const long long T = layout == NPLDA_XVEC_LAYOUT_BCT ? R / U : 0;
    const long long n0 = L.rows * kFeatP;
    hipLaunchKernelGGL(xvec_prep_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, x, layout, ld_in, T, R,
                       L.rows, (float*)(saved + L.oX));
    if (int rc = nplda_launch_status()) return rc;
    hipLaunchKernelGGL(xvtr_rem_kernel, dim3((unsigned)((L.rows + 255) / 256)), dim3(256), 0, st, offsets, U, R, L.rows,
                       (int*)(saved + L.oRem));
    if (int rc = nplda_launch_status()) return rc;
    // slack rows: read by the last tile's taps here and by the weight gradient's (finite zeros, never NaN patterns)
    for (int l = 0; l < kTdnn; ++l)
        if (hipMemsetAsync(saved + L.oO[l] + (size_t)L.live * out_ld(l) * 4, 0, (size_t)kRowSlack * out_ld(l) * 4, st) !=
            hipSuccess)
            return NPLDA_EINVAL;
    return NPLDA_OK;
}

int train_forward_tail(const float* P, const int64_t* offsets, long long U, long long R, int pooling,
                       const SavedLayout& L, char* saved, float* out, long long ldx, hipStream_t st) {
    float* pooled = (float*)(saved + L.oP);
    hipLaunchKernelGGL(xvec_pool_kernel, dim3((unsigned)(U * kPoolBlocks)), dim3(256), 0, st,
                       (const float*)(saved + L.oO[kTdnn - 1]), (long long)out_ld(kTdnn - 1), offsets, R, pooling, pooled);
    if (int rc = nplda_launch_status()) return rc;
    if (L.urows > U && hipMemsetAsync(pooled + U * kPooledLd, 0, (size_t)(L.urows - U) * kPooledLd * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    const GemmArgs a = gemm_args(P, geomF(kTdnn), pooled, kPooledLd, out, ldx, U, 1, 0);
    return launch_gemm(xvtr_gemm_kernel<EpiExtract>, a, L.urows, st, EpiExtract{});
}

int backward_head(const BwdBuffers& b, const SavedLayout& L, long long U, const float* dxvec, long long lddx,
                  const float* PT, float* grad, hipStream_t st, float** dA, long long* ldA) {
    // dxvec -> (urows, 512) zero-padded
    if (hipMemcpy2DAsync(b.dx, kEmbDim * 4, dxvec, (size_t)lddx * 4, kEmbDim * 4, (size_t)U, hipMemcpyDeviceToDevice,
                         st) != hipSuccess)
        return NPLDA_EINVAL;
    if (L.urows > U && hipMemsetAsync(b.dx + U * kEmbDim, 0, (size_t)(L.urows - U) * kEmbDim * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    // lin11: dW11 = dxvec^T pooled, db11 = sum dxvec, dpooled = dxvec W11
    float* g11 = grad + grad_offset(kTdnn);
    if (int rc = launch_wgrad(kTdnn, b.dx, kEmbDim, kEmbDim, b.pooled, kPooledLd, U, b.part, g11, st)) return rc;
    if (int rc = launch_colsum(b.dx, kEmbDim, U, kEmbDim, b.colp, g11 + (size_t)kEmbDim * kShape[kTdnn].Din, st))
        return rc;
    const GemmArgs a =
        gemm_args(PT, geomT(kTdnn, packedT_offset(kTdnn)), b.dx, kEmbDim, b.dpool, kPooledLd, L.urows, 1, 0);
    if (int rc = launch_gemm(xvtr_gemm_kernel<EpiExtract>, a, L.urows, st, EpiExtract{})) return rc;
    // dA10 is written on the valid rows only (every other row zero); the ping-pong pair needs its leading rows zero
    const int ld10 = out_ld(kTdnn - 1);
    if (hipMemsetAsync(b.bufX, 0, (size_t)b.brow * ld10 * 4, st) != hipSuccess ||
        hipMemsetAsync(b.bufY, 0, (size_t)kLead * kEmbDim * 4, st) != hipSuccess ||
        hipMemsetAsync(b.bufZ, 0, (size_t)kLead * kEmbDim * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    *dA = b.bufX + (size_t)kLead * ld10;
    *ldA = ld10;
    return NPLDA_OK;
}

int layer_param_grads(int l, const float* dA, long long ldA, const BwdBuffers& b, const SavedLayout& L, float* grad,
                      hipStream_t st) {
    const Layer s = kShape[l];
    const float* Oin = l == 0 ? (const float*)(b.sb + L.oX) : (const float*)(b.sb + L.oO[l - 1]);
    const long long ldin = l == 0 ? kFeatP : out_ld(l - 1);
    if (int rc = launch_wgrad(l, dA, ldA, (int)ldA, Oin, ldin, L.live, b.part, grad + grad_offset(l), st)) return rc;
    return launch_colsum(dA, ldA, L.live, s.Dout, b.colp, grad + grad_offset(l) + (size_t)s.Dout * s.c * s.Din, st);
}

}  // namespace nplda_xvec_train

extern "C" {

size_t nplda_xvec_train_saved_bytes(int64_t total_frames, int64_t n_utts) {
    if (total_frames < 0 || n_utts < 0) return 0;
    return saved_layout(total_frames, n_utts).total;
}

size_t nplda_xvec_packed_t_bytes(void) { return packedT_floats() * sizeof(float); }

int nplda_xvec_pack_t_f32(const float* const* W, void* packed_t, size_t packed_t_bytes, nplda_stream_t stream) {
    if (!W || !packed_t || !nplda_aligned16(packed_t)) return NPLDA_EINVAL;
    if (packed_t_bytes < nplda_xvec_packed_t_bytes()) return NPLDA_ENOSPC;
    for (int l = 1; l < kLayers; ++l)
        if (!W[l]) return NPLDA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* P = (float*)packed_t;
    size_t o = 0;
    for (int l = 1; l < kLayers; ++l) {
        const LayerGeom G = geomT(l, o);
        o = G.end;
        const size_t total = (size_t)G.nkbp * G.XBp * 256;
        hipLaunchKernelGGL(xvtr_pack_t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W[l],
                           kShape[l].Din, kShape[l].Dout, G.c, G.Dinp, G.XBp, total, P + G.oFrag);
        if (int rc = nplda_launch_status()) return rc;
        const int Nv = G.XBp * 16;
        hipLaunchKernelGGL(xvtr_fill_vec_kernel, dim3((unsigned)((Nv + 255) / 256)), dim3(256), 0, st, Nv, P + G.oBias,
                           P + G.oMean, P + G.oInv);
        if (int rc = nplda_launch_status()) return rc;
    }
    return NPLDA_OK;
}

int nplda_xvec_extract_train_f32(const float* x, int layout, int64_t ld_in, const int64_t* offsets, int64_t n_utts,
                                 int64_t total_frames, int pooling, const void* packed, float* out, int64_t ldx,
                                 void* saved, size_t saved_bytes, nplda_stream_t stream) {
    bool nothing;
    const int bad = check_forward(n_utts, total_frames, layout, pooling, ld_in, ldx, {x, offsets, packed, out, saved},
                                 {packed, out, saved}, &nothing);
    if (bad || nothing) return bad;
    if (n_utts > 0x7fffffffLL / kPoolBlocks) return NPLDA_EUNSUPPORTED;
    const SavedLayout L = saved_layout(total_frames, n_utts);
    if (saved_bytes < L.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)saved;
    const int* rem = (const int*)(base + L.oRem);
    const float* P = (const float*)packed;
    if (int rc = train_forward_head(x, layout, ld_in, offsets, n_utts, total_frames, L, base, st)) return rc;
    const float* in = (const float*)(base + L.oX);
    long long ld = kFeatP;
    for (int l = 0; l < kTdnn; ++l) {
        float* o = (float*)(base + L.oO[l]);
        const GemmArgs a = gemm_args(P, geomF(l), in, ld, o, out_ld(l), L.live, kShape[l].d, 1);
        const EpiTrain e{(uint8_t*)(base + L.oM[l]), (long long)out_ld(l), rem, kCtx[l]};
        if (int rc = launch_gemm(xvtr_gemm_kernel<EpiTrain>, a, L.live, st, e)) return rc;
        in = o;
        ld = out_ld(l);
    }
    return train_forward_tail(P, offsets, n_utts, total_frames, pooling, L, base, out, ldx, st);
}

size_t nplda_xvec_grad_floats(void) { return grad_offset(kLayers); }

size_t nplda_xvec_backward_workspace_bytes(int64_t total_frames, int64_t n_utts) {
    if (total_frames < 0 || n_utts < 0) return 0;
    return bwd_layout(total_frames, n_utts).total;
}

int nplda_xvec_backward_f32(const void* saved, size_t saved_bytes, const int64_t* offsets, int64_t n_utts,
                            int64_t total_frames, int pooling, const float* dxvec, int64_t lddx, const void* packed,
                            const void* packed_t, float* grad, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    bool nothing;
    const int bad = check_backward(n_utts, total_frames, pooling, lddx, saved, offsets, dxvec, packed, packed_t, grad, ws,
                                   &nothing);
    if (bad || nothing) return bad;
    if (n_utts > 0x7fffffffLL / kPoolBlocks) return NPLDA_EUNSUPPORTED;
    const SavedLayout L = saved_layout(total_frames, n_utts);
    const WsLayoutB W = bwd_layout(total_frames, n_utts);
    if (saved_bytes < L.total || ws_bytes < W.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const BwdBuffers b = bwd_buffers(L, W, saved, ws);
    const float* P = (const float*)packed;
    const float* PT = (const float*)packed_t;
    float* dA;
    long long ldA;
    if (int rc = backward_head(b, L, n_utts, dxvec, lddx, PT, grad, st, &dA, &ldA)) return rc;
    // tdnn10: pooling backward into dA10 (every other row zero)
    hipLaunchKernelGGL(xvbwd_pool_kernel, dim3((unsigned)(n_utts * kPoolBlocks)), dim3(256), 0, st,
                       (const float*)(b.sb + L.oO[kTdnn - 1]), ldA, (const uint8_t*)(b.sb + L.oM[kTdnn - 1]),
                       P + geomF(kTdnn - 1).oInv, b.pooled, b.dpool, offsets, (long long)total_frames, pooling, dA);
    if (int rc = nplda_launch_status()) return rc;
    for (int l = kTdnn - 1; l >= 0; --l) {
        if (int rc = layer_param_grads(l, dA, ldA, b, L, grad, st)) return rc;
        if (l == 0) break;
        const EpiBwd e{(const uint8_t*)(b.sb + L.oM[l - 1]), (long long)out_ld(l - 1), P + geomF(l - 1).oInv};
        const GemmArgs a = data_grad_args(l, PT, dA, ldA, b, L.live);
        if (int rc = launch_gemm(xvtr_gemm_kernel<EpiBwd>, a, L.live, st, e)) return rc;
        dA = a.out;
        ldA = a.ld_out;
    }
    return NPLDA_OK;
}

}  // extern "C"
