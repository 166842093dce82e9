// nplda_xvec.hip — E-TDNN x-vector extraction (gfx950, exact fp32 MFMA): XVectorNet_ETDNN_12Layer.extract
// (utils/models.py:170-186) over a ragged batch of utterances.
//
//  * xvec_prep_kernel     caller's frames ((total, 30) rows with any stride, or the reference's (B, 30, T)) -> a
//                         (rows, 32) zero-padded image; rows past the last frame are zero.  The only kernel that reads
//                         the caller's input.
//  * xvec_gemm_kernel     one TDNN layer (or lin11): out[r, n] = epi(sum_k in[r + j(k) d, i(k)] W[n, k]) over ALL rows of
//                         the batch in one launch.  The dilated context is gathered implicitly: k16-block kb of row r
//                         reads frame r + (kb / (Dinp / 16)) d.  A row's result depends only on its own input rows, so an
//                         utterance's frames come out the same whatever else is in the batch; the rows near an
//                         utterance's end read into the next one and are never read by a valid frame downstream.
//                         Block: 4 waves, 128 rows x 128 columns; each wave 32 rows (two 16-row groups) x 8 column
//                         blocks = 16 accumulators of v_mfma_f32_16x16x4_f32.  The weights are the A operand, staged in
//                         chunks of 4 k16-blocks (4 x 8 x 1 KB) into a double-buffered LDS image (64 KB: two blocks per
//                         CU), the next chunk's global loads issued while the current one is consumed, one barrier per
//                         chunk; fragments come back as conflict-free ds_read_b128.  The data rows are the B operand,
//                         one float4 per lane per k16-block straight from the activations (the k permutation of
//                         nplda_matmul.hip's rows_matmul_kernel), prefetched one k-block ahead.  Epilogue: bias, ReLU,
//                         (y - running_mean) * inv_std, each switchable, stored as 16-byte rows.
//  * xvec_pool_kernel     statistics pooling (utils/models.py:152-156): per utterance and feature, mean and unbiased
//                         std / var over the T_u - 22 valid tdnn10 rows, two passes with fp64 sums, one thread per
//                         feature (fixed order: deterministic).
//  * xvec_pool_windows_kernel  the same pooling over a table of (overlapping) row windows of ONE dense pass: sliding-window
//                         x-vectors without running a frame through the layers once per window (design/k23).
// The GEMM body, xvec_prep_kernel and xvec_pool_kernel live in nplda_xvec_body.h, shared with the training forward and
// backward (nplda_xvec_bwd.hip), and so do the host pieces the family shares: gemm_args, launch_gemm and the argument
// checks of a forward entry point (check_forward); the workspace arithmetic (align256, whole_tiles, out_ld, geomF) is
// nplda_xvec.h's.
#include "nplda_xvec_body.h"

namespace {

using namespace nplda_xvec;

__global__ void xvec_pack_frag_kernel(const float* __restrict__ W, int Din, int Dout, int c, int Dinp, int XBp,
                                      size_t total, float* __restrict__ frag) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const size_t blk = idx >> 8;
    const int xb = (int)(blk % XBp), kb = (int)(blk / XBp);
    const int n = 16 * xb + (lane & 15), kp = 16 * kb + 4 * (lane >> 4) + i;
    const int j = kp / Dinp, col = kp - j * Dinp;
    float v = 0.f;
    if (n < Dout && j < c && col < Din) v = W[(size_t)n * c * Din + (size_t)j * Din + col];
    frag[idx] = v;
}

__global__ void xvec_pack_vec_kernel(const float* __restrict__ b, const float* __restrict__ mean,
                                     const float* __restrict__ var, float eps, int Dout, int Nv, float* __restrict__ ob,
                                     float* __restrict__ om, float* __restrict__ oi) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Nv) return;
    const bool ok = n < Dout;
    ob[n] = ok ? b[n] : 0.f;
    om[n] = ok && mean ? mean[n] : 0.f;
    oi[n] = ok && var ? (float)(1.0 / sqrt((double)var[n] + (double)eps)) : 1.f;
}

__global__ __launch_bounds__(256, 2) void xvec_gemm_kernel(const GemmArgs a) { xvec_gemm_body(a, EpiExtract{}); }

struct WsLayout {
    long long rows, urows;
    size_t o0, oA, oB, oP, total;  // bytes
};

WsLayout ws_layout(long long R, long long U) {
    WsLayout w;
    w.rows = whole_tiles(R) + kRowSlack;
    w.urows = whole_tiles(U);
    w.o0 = 0;
    w.oA = align256(w.o0 + (size_t)w.rows * kFeatP * 4);
    w.oB = align256(w.oA + (size_t)w.rows * kEmbDim * 4);
    w.oP = align256(w.oB + (size_t)w.rows * out_ld(kTdnn - 1) * 4);
    w.total = align256(w.oP + (size_t)w.urows * kPooledLd * 4);
    return w;
}

int launch_layer(int l, const float* packed, const float* in, long long ld_in, long long rows, float* out,
                 long long ld_out, long long row_limit, hipStream_t st) {
    const GemmArgs a = gemm_args(packed, geomF(l), in, ld_in, out, ld_out, row_limit, kShape[l].d, l < kTdnn ? 1 : 0);
    return launch_gemm(xvec_gemm_kernel, a, rows, st);
}

// lin11 over the n pooled rows (prows of them allocated: whole tiles, the padding rows zeroed)
int lin11(const float* P, float* pooled, long long n, long long prows, float* out, long long ldx, hipStream_t st) {
    if (prows > n && hipMemsetAsync(pooled + n * kPooledLd, 0, (size_t)(prows - n) * kPooledLd * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    return launch_layer(kTdnn, P, pooled, kPooledLd, prows, out, ldx, n, st);
}

// Prep and tdnn1..tdnn10 over total_frames rows: the common part of both extraction entry points.  Leaves the dense
// tdnn10 rows (ld 1504) in the workspace's B buffer and returns it in *h.
int dense_pass(const float* x, int layout, long long ld_in, long long T, long long total_frames, const WsLayout& w,
               char* base, const float* P, hipStream_t st, const float** h) {
    float* b0 = (float*)(base + w.o0);
    float* bA = (float*)(base + w.oA);
    float* bB = (float*)(base + w.oB);
    const long long n0 = w.rows * kFeatP;
    hipLaunchKernelGGL(xvec_prep_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, x, layout, ld_in, T,
                       total_frames, w.rows, b0);
    if (int rc = nplda_launch_status()) return rc;
    // the slack rows of the activation buffers are read by the last tile's context taps (results discarded): zeroed
    const long long live = w.rows - kRowSlack, ld10 = out_ld(kTdnn - 1);
    if (hipMemsetAsync(bA + live * kEmbDim, 0, (size_t)kRowSlack * kEmbDim * 4, st) != hipSuccess ||
        hipMemsetAsync(bB + live * kEmbDim, 0, (size_t)kRowSlack * kEmbDim * 4, st) != hipSuccess ||
        hipMemsetAsync(bB + live * ld10, 0, (size_t)kRowSlack * ld10 * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    const float* in = b0;
    long long ld = kFeatP;
    for (int l = 0; l < kTdnn; ++l) {
        float* o = (l & 1) ? bB : bA;
        const long long ldo = out_ld(l);
        if (int rc = launch_layer(l, P, in, ld, live, o, ldo, live, st)) return rc;
        in = o;
        ld = ldo;
    }
    *h = bB;
    return NPLDA_OK;
}

// Statistics pooling over a table of row windows: window w pools the dense tdnn10 rows [begin[w], end[w] - 22), the
// value xvec_pool_kernel gives for the same rows as an utterance, bit for bit (every column is one sequential fp64 chain
// in row order, twice; nothing is reduced across threads).  One thread owns FOUR adjacent columns: a row is one 16-byte
// load per lane (the rows are 16-byte aligned: ld 1504) and the four chains run interleaved, which hides the latency of
// the dependent fp64 adds that the one-column mapping waits on.  128 threads per block, 3 blocks per window (375 column
// quads).  The second pass re-reads rows this block has just read (128 x 16 B per row: they come back from the cache).
constexpr int kWinPoolThreads = 128;
constexpr int kWinPoolBlocks = (kPoolLd / 4 + kWinPoolThreads - 1) / kWinPoolThreads;

__global__ __launch_bounds__(kWinPoolThreads) void xvec_pool_windows_kernel(const float* __restrict__ h,
                                                                            const int64_t* __restrict__ begin,
                                                                            const int64_t* __restrict__ end, long long R,
                                                                            int pooling, float* __restrict__ pooled) {
    const long long w = blockIdx.x / kWinPoolBlocks;
    const int cb = (int)(blockIdx.x - w * kWinPoolBlocks), c4 = cb * kWinPoolThreads + threadIdx.x;
    float* prow = pooled + w * kPooledLd;
    if (cb == 0 && threadIdx.x < kPooledLd - 2 * kPoolDim) prow[2 * kPoolDim + threadIdx.x] = 0.f;
    if (c4 >= kPoolDim / 4) return;  // 1500 = 4 x 375: no quad straddles the last column
    long long b = begin[w], e = end[w];  // clamped as xvec_pool_kernel clamps a bad offset table
    b = b < 0 ? 0 : (b > R ? R : b);
    e = e < b ? b : (e > R ? R : e);
    const long long n = e - b - kContext;
    const f32x4* p = reinterpret_cast<const f32x4*>(h + b * kPoolLd) + c4;
    constexpr long long ld4 = kPoolLd / 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (long long t = 0; t < n; ++t) {
        const f32x4 v = p[t * ld4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += (double)v[i];
    }
    double mean[4], q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) mean[i] = n > 0 ? s[i] / (double)n : __builtin_nan("");
#pragma unroll 4
    for (long long t = 0; t < n; ++t) {
        const f32x4 v = p[t * ld4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double dv = (double)v[i] - mean[i];
            q[i] += dv * dv;
        }
    }
    f32x4 om, os;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double var = n > 1 ? q[i] / (double)(n - 1) : __builtin_nan("");  // unbiased: NaN at n = 1
        om[i] = (float)mean[i];
        os[i] = (float)(pooling == NPLDA_XVEC_POOL_VAR ? var : sqrt(var));
    }
    *reinterpret_cast<f32x4*>(prow + 4 * c4) = om;
    *reinterpret_cast<f32x4*>(prow + kPoolDim + 4 * c4) = os;
}

}  // namespace

extern "C" {

size_t nplda_xvec_packed_bytes(void) { return packed_floats() * sizeof(float); }

int nplda_xvec_pack_f32(const float* const* W, const float* const* b, const float* const* running_mean,
                        const float* const* running_var, const float* eps, void* packed, size_t packed_bytes,
                        nplda_stream_t stream) {
    if (!W || !b || !running_mean || !running_var || !eps || !packed || !nplda_aligned16(packed)) return NPLDA_EINVAL;
    if (packed_bytes < nplda_xvec_packed_bytes()) return NPLDA_ENOSPC;
    for (int l = 0; l < kLayers; ++l) {
        if (!W[l] || !b[l]) return NPLDA_EINVAL;
        if (l < kTdnn && (!running_mean[l] || !running_var[l] || !(eps[l] >= 0.f))) return NPLDA_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float* P = (float*)packed;
    size_t o = 0;
    for (int l = 0; l < kLayers; ++l) {
        const LayerGeom G = geom(l, o);
        o = G.end;
        const size_t total = (size_t)G.nkbp * G.XBp * 256;
        hipLaunchKernelGGL(xvec_pack_frag_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W[l], G.Din,
                           G.Dout, G.c, G.Dinp, G.XBp, total, P + G.oFrag);
        if (int rc = nplda_launch_status()) return rc;
        const int Nv = G.XBp * 16;
        const bool bn = l < kTdnn;
        hipLaunchKernelGGL(xvec_pack_vec_kernel, dim3((unsigned)((Nv + 255) / 256)), dim3(256), 0, st, b[l],
                           bn ? running_mean[l] : (const float*)nullptr, bn ? running_var[l] : (const float*)nullptr,
                           bn ? eps[l] : 0.f, G.Dout, Nv, P + G.oBias, P + G.oMean, P + G.oInv);
        if (int rc = nplda_launch_status()) return rc;
    }
    return NPLDA_OK;
}

size_t nplda_xvec_workspace_bytes(int64_t total_frames, int64_t n_utts) {
    if (total_frames < 0 || n_utts < 0) return 0;
    return ws_layout(total_frames, n_utts).total;
}

int nplda_xvec_extract_f32(const float* x, int layout, int64_t ld_in, const int64_t* offsets, int64_t n_utts,
                           int64_t total_frames, int pooling, const void* packed, float* out, int64_t ldx, void* ws,
                           size_t ws_bytes, nplda_stream_t stream) {
    bool nothing;
    const int bad = check_forward(n_utts, total_frames, layout, pooling, ld_in, ldx, {x, offsets, packed, out, ws},
                                 {packed, out, ws}, &nothing);
    if (bad || nothing) return bad;
    if (n_utts > 0x7fffffffLL / kPoolBlocks) return NPLDA_EUNSUPPORTED;
    const WsLayout w = ws_layout(total_frames, n_utts);
    if (ws_bytes < w.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    float* pooled = (float*)(base + w.oP);
    const float* P = (const float*)packed;
    const long long T = layout == NPLDA_XVEC_LAYOUT_BCT ? total_frames / n_utts : 0;
    const float* h;
    if (int rc = dense_pass(x, layout, ld_in, T, total_frames, w, base, P, st, &h)) return rc;
    hipLaunchKernelGGL(xvec_pool_kernel, dim3((unsigned)(n_utts * kPoolBlocks)), dim3(256), 0, st, h,
                       (long long)out_ld(kTdnn - 1), offsets, (long long)total_frames, pooling, pooled);
    if (int rc = nplda_launch_status()) return rc;
    return lin11(P, pooled, n_utts, w.urows, out, ldx, st);
}

size_t nplda_xvec_windows_workspace_bytes(int64_t total_frames, int64_t n_windows) {
    if (total_frames < 0 || n_windows < 0) return 0;
    return ws_layout(total_frames, n_windows).total;
}

int nplda_xvec_extract_windows_f32(const float* x, int64_t ld_in, int64_t total_frames, const int64_t* win_begin,
                                   const int64_t* win_end, int64_t n_windows, int pooling, const void* packed, float* out,
                                   int64_t ldx, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    bool nothing;
    const int bad = check_forward(n_windows, total_frames, NPLDA_XVEC_LAYOUT_ROWS, pooling, ld_in, ldx,
                                 {x, win_begin, win_end, packed, out, ws}, {packed, out, ws}, &nothing);
    if (bad || nothing) return bad;
    if (n_windows > 0x7fffffffLL / kWinPoolBlocks) return NPLDA_EUNSUPPORTED;
    const WsLayout w = ws_layout(total_frames, n_windows);
    if (ws_bytes < w.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    float* pooled = (float*)(base + w.oP);
    const float* P = (const float*)packed;
    const float* h;
    if (int rc = dense_pass(x, NPLDA_XVEC_LAYOUT_ROWS, ld_in, 0, total_frames, w, base, P, st, &h)) return rc;
    hipLaunchKernelGGL(xvec_pool_windows_kernel, dim3((unsigned)(n_windows * kWinPoolBlocks)), dim3(kWinPoolThreads), 0,
                       st, h, win_begin, win_end, (long long)total_frames, pooling, pooled);
    if (int rc = nplda_launch_status()) return rc;
    return lin11(P, pooled, n_windows, w.urows, out, ldx, st);
}

}  // extern "C"
