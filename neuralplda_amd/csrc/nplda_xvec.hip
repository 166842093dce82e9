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
// The GEMM body, xvec_prep_kernel and xvec_pool_kernel live in nplda_xvec_body.h, shared with the training forward and
// backward (nplda_xvec_bwd.hip).
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

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

WsLayout ws_layout(long long R, long long U) {
    WsLayout w;
    w.rows = (R + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock + kRowSlack;
    w.urows = (U + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock;
    w.o0 = 0;
    w.oA = align256(w.o0 + (size_t)w.rows * kFeatP * 4);
    w.oB = align256(w.oA + (size_t)w.rows * kEmbDim * 4);
    w.oP = align256(w.oB + (size_t)w.rows * 16 * ((kPoolDim + 15) / 16) * 4);
    w.total = align256(w.oP + (size_t)w.urows * kPooledLd * 4);
    return w;
}

int launch_layer(int l, const float* packed, const float* in, long long ld_in, long long rows, float* out,
                 long long ld_out, long long row_limit, hipStream_t st) {
    size_t o = 0;
    LayerGeom G = geom(0, 0);
    for (int i = 0; i <= l; ++i) {
        G = geom(i, o);
        o = G.end;
    }
    GemmArgs a;
    a.in = in; a.ld_in = ld_in;
    a.frag = reinterpret_cast<const f32x4*>(packed + G.oFrag);
    a.bias = packed + G.oBias; a.mean = packed + G.oMean; a.inv = packed + G.oInv;
    a.out = out; a.ld_out = ld_out; a.row_limit = row_limit;
    a.nkb = G.nkb; a.nkbp = G.nkbp; a.XBp = G.XBp; a.Np = G.Np; a.kbt = G.Dinp / 16; a.dil = G.d;
    a.relu_bn = l < kTdnn ? 1 : 0;
    const long long tiles = rows / kRowsPerBlock;
    if (tiles <= 0) return NPLDA_OK;
    if (tiles > 0x7fffffffLL) return NPLDA_EINVAL;
    hipLaunchKernelGGL(xvec_gemm_kernel, dim3((unsigned)tiles, (unsigned)(G.XBp / kNS)), dim3(256), 0, st, a);
    return nplda_launch_status();
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
    if (n_utts < 0 || total_frames < 0) return NPLDA_EINVAL;
    if (layout != NPLDA_XVEC_LAYOUT_ROWS && layout != NPLDA_XVEC_LAYOUT_BCT) return NPLDA_EINVAL;
    if (pooling != NPLDA_XVEC_POOL_STD && pooling != NPLDA_XVEC_POOL_VAR) return NPLDA_EINVAL;
    if (n_utts == 0) return NPLDA_OK;
    if (!x || !offsets || !packed || !out || !ws || !nplda_aligned16(packed) || !nplda_aligned16(out) ||
        !nplda_aligned16(ws) || ldx < kEmbDim || (ldx % 4) != 0)
        return NPLDA_EINVAL;
    if (layout == NPLDA_XVEC_LAYOUT_ROWS && ld_in < kFeat) return NPLDA_EINVAL;
    if (layout == NPLDA_XVEC_LAYOUT_BCT && (total_frames % n_utts) != 0) return NPLDA_EINVAL;
    if (n_utts > 0x7fffffffLL / kPoolBlocks) return NPLDA_EUNSUPPORTED;
    const WsLayout w = ws_layout(total_frames, n_utts);
    if (ws_bytes < w.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    float* b0 = (float*)(base + w.o0);
    float* bA = (float*)(base + w.oA);
    float* bB = (float*)(base + w.oB);
    float* pooled = (float*)(base + w.oP);
    const float* P = (const float*)packed;
    const long long T = layout == NPLDA_XVEC_LAYOUT_BCT ? total_frames / n_utts : 0;
    const long long n0 = w.rows * kFeatP;
    hipLaunchKernelGGL(xvec_prep_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, x, layout,
                       (long long)ld_in, T, (long long)total_frames, w.rows, b0);
    if (int rc = nplda_launch_status()) return rc;
    // the slack rows of the activation buffers are read by the last tile's context taps (results discarded): zeroed
    const long long live = w.rows - kRowSlack;
    const int ldB = 16 * ((kPoolDim + 15) / 16);
    if (hipMemsetAsync(bA + live * kEmbDim, 0, (size_t)kRowSlack * kEmbDim * 4, st) != hipSuccess ||
        hipMemsetAsync(bB + live * kEmbDim, 0, (size_t)kRowSlack * kEmbDim * 4, st) != hipSuccess ||
        hipMemsetAsync(bB + live * ldB, 0, (size_t)kRowSlack * ldB * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    const float* in = b0;
    long long ld = kFeatP;
    for (int l = 0; l < kTdnn; ++l) {
        float* o = (l & 1) ? bB : bA;
        const long long ldo = l == kTdnn - 1 ? ldB : kEmbDim;
        if (int rc = launch_layer(l, P, in, ld, live, o, ldo, live, st)) return rc;
        in = o;
        ld = ldo;
    }
    hipLaunchKernelGGL(xvec_pool_kernel, dim3((unsigned)(n_utts * kPoolBlocks)), dim3(256), 0, st, bB,
                       (long long)ldB, offsets, (long long)total_frames, pooling, pooled);
    if (int rc = nplda_launch_status()) return rc;
    if (w.urows > n_utts &&
        hipMemsetAsync(pooled + n_utts * kPooledLd, 0, (size_t)(w.urows - n_utts) * kPooledLd * 4, st) != hipSuccess)
        return NPLDA_EINVAL;
    return launch_layer(kTdnn, P, pooled, kPooledLd, w.urows, out, ldx, n_utts, st);
}

}  // extern "C"
