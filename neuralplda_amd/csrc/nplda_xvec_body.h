// nplda_xvec_body.h — the body of the E-TDNN GEMM (see nplda_xvec.hip for the design), templated on its epilogue so that
// the extraction kernel (nplda_xvec.hip, one instantiation) and the training forward / data-gradient kernels
// (nplda_xvec_bwd.hip, nplda_xvec_bn.hip) run the same main loop and hence the same fp32 sums, bit for bit; and the host
// side every file of the family uses with it: gemm_args (a layer's GemmArgs), launch_gemm (the one grid computation) and
// check_forward (the argument checks of the four forward entry points).
//
// An epilogue is a functor called once per (row group, 16-column block) with the accumulator of lane (j, g):
//     epi(a, row, col, v)   row = r0 + 16 rg + j (< a.row_limit), col = 16 xb + 4 g (< a.Np), v = the four sums of
//                           out[row, col .. col + 3] before bias.
// A dilation may be negative: the data gradient gathers its taps at row - j d (the caller provides leading slack rows).
#pragma once
#include <initializer_list>
#include "nplda_common.h"
#include "nplda_xvec.h"

namespace nplda_xvec {

struct GemmArgs {
    const float* in;       // activations, rows >= gridDim.x * 128 + kRowSlack, row stride ld_in
    long long ld_in;
    const f32x4* frag;     // [nkbp][XBp][64]
    const float* bias;     // [XBp * 16]
    const float* mean;
    const float* inv;
    float* out;
    long long ld_out, row_limit;
    int nkb, nkbp, XBp, Np, kbt, dil;  // kbt: k16-blocks per context tap (Dinp / 16)
    int relu_bn;
};

// extraction: bias, then ReLU and (y - running_mean) * inv_std when relu_bn (tdnn layers), stored as 16-byte rows
struct EpiExtract {
    __device__ __forceinline__ void operator()(const GemmArgs& a, long long row, int col, f32x4 v) const {
        v = v + *reinterpret_cast<const f32x4*>(a.bias + col);
        if (a.relu_bn) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(a.mean + col);
            const f32x4 s = *reinterpret_cast<const f32x4*>(a.inv + col);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (fmaxf(v[c], 0.f) - m[c]) * s[c];
        }
        *reinterpret_cast<f32x4*>(a.out + row * a.ld_out + col) = v;
    }
};

template <class Epi>
__device__ __forceinline__ void xvec_gemm_body(const GemmArgs& a, const Epi& epi) {
    __shared__ f32x4 wl[2 * kKC * kNS * 64];  // [buf][kk][u][lane], 64 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int xb0 = blockIdx.y * kNS;
    const long long r0 = (long long)blockIdx.x * kRowsPerBlock + 32 * wave;
    const float* src0 = a.in + (r0 + j) * a.ld_in + 4 * g;
    const float* src1 = src0 + 16 * a.ld_in;
    constexpr int kStg = kKC * kNS * 64 / 256;  // float4 per thread per chunk
    const int XBp = a.XBp;
    auto stage_src = [&](int ch, int s) -> const f32x4* {
        const int idx = tid + 256 * s, kk = idx / (kNS * 64), rem = idx - kk * (kNS * 64);
        return a.frag + ((size_t)(ch * kKC + kk) * XBp + xb0) * 64 + rem;
    };
    f32x4 stg[kStg];
#pragma unroll
    for (int s = 0; s < kStg; ++s) stg[s] = *stage_src(0, s);
#pragma unroll
    for (int s = 0; s < kStg; ++s) wl[tid + 256 * s] = stg[s];
    __syncthreads();
    auto data_off = [&](int kb) -> long long {
        const int jt = kb / a.kbt;
        return (long long)jt * a.dil * a.ld_in + 16 * (kb - jt * a.kbt);
    };
    f32x4 acc[2][kNS];
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int u = 0; u < kNS; ++u) acc[rg][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 cur0 = *reinterpret_cast<const f32x4*>(src0), cur1 = *reinterpret_cast<const f32x4*>(src1);
    const int nkb = a.nkb, nkbp = a.nkbp;
    for (int kb = 0; kb < nkbp; ++kb) {
        const int kk = kb & (kKC - 1), buf = (kb / kKC) & 1;
        if (kk == 0 && kb + kKC < nkbp) {
#pragma unroll
            for (int s = 0; s < kStg; ++s) stg[s] = *stage_src(kb / kKC + 1, s);
        }
        const int kn = kb + 1 < nkb ? kb + 1 : nkb - 1;
        const long long on = data_off(kn);
        const f32x4 nxt0 = *reinterpret_cast<const f32x4*>(src0 + on);
        const f32x4 nxt1 = *reinterpret_cast<const f32x4*>(src1 + on);
        if (kb < nkb) {
            const f32x4* w = wl + (buf * kKC + kk) * (kNS * 64) + lane;
            f32x4 av[kNS];
#pragma unroll
            for (int u = 0; u < kNS; ++u) av[u] = w[u * 64];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int u = 0; u < kNS; ++u) {
                    acc[0][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][r], cur0[r], acc[0][u], 0, 0, 0);
                    acc[1][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][r], cur1[r], acc[1][u], 0, 0, 0);
                }
            }
        }
        cur0 = nxt0;
        cur1 = nxt1;
        if (kk == kKC - 1 && kb + 1 < nkbp) {
#pragma unroll
            for (int s = 0; s < kStg; ++s) wl[(buf ^ 1) * (kKC * kNS * 64) + tid + 256 * s] = stg[s];
            __syncthreads();
        }
    }
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) {
        const long long row = r0 + 16 * rg + j;
        if (row >= a.row_limit) continue;
#pragma unroll
        for (int u = 0; u < kNS; ++u) {
            const int col = 16 * (xb0 + u) + 4 * g;
            if (col >= a.Np) continue;
            epi(a, row, col, acc[rg][u]);
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------

// layer geometry G inside the image `img` (packed, or the transposed image of the backward) -> the kernel's arguments
inline GemmArgs gemm_args(const float* img, const LayerGeom& G, const float* in, long long ld_in, float* out,
                          long long ld_out, long long row_limit, int dil, int relu_bn) {
    GemmArgs a;
    a.in = in; a.ld_in = ld_in;
    a.frag = reinterpret_cast<const f32x4*>(img + G.oFrag);
    a.bias = img + G.oBias; a.mean = img + G.oMean; a.inv = img + G.oInv;
    a.out = out; a.ld_out = ld_out; a.row_limit = row_limit;
    a.nkb = G.nkb; a.nkbp = G.nkbp; a.XBp = G.XBp; a.Np = G.Np; a.kbt = G.Dinp / 16; a.dil = dil;
    a.relu_bn = relu_bn;
    return a;
}

// `kernel` is a __global__ wrapper of xvec_gemm_body taking (GemmArgs, epilogue...): rows / 128 row tiles (rows is a
// whole number of tiles) x the layer's column slices
template <class Kernel, class... Epi>
int launch_gemm(Kernel kernel, const GemmArgs& a, long long rows, hipStream_t st, const Epi&... e) {
    const long long tiles = rows / kRowsPerBlock;
    if (tiles <= 0) return NPLDA_OK;
    if (tiles > 0x7fffffffLL) return NPLDA_EINVAL;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)(a.XBp / kNS)), dim3(256), 0, st, a, e...);
    return nplda_launch_status();
}

inline bool none_null(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return false;
    return true;
}
inline bool all_aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!nplda_aligned16(p)) return false;
    return true;
}
inline bool bad_pooling(int pooling) { return pooling != NPLDA_XVEC_POOL_STD && pooling != NPLDA_XVEC_POOL_VAR; }

// The argument checks of a forward entry point (n utterances or windows), in the order that is part of the ABI; the
// caller's grid limits (EUNSUPPORTED) and buffer sizes (ENOSPC) follow them, in that order.  *nothing: n == 0, return OK.
inline int check_forward(int64_t n, int64_t total_frames, int layout, int pooling, int64_t ld_in, int64_t ldx,
                         std::initializer_list<const void*> ptrs, std::initializer_list<const void*> aligned,
                         bool* nothing) {
    *nothing = false;
    if (n < 0 || total_frames < 0) return NPLDA_EINVAL;
    if (layout != NPLDA_XVEC_LAYOUT_ROWS && layout != NPLDA_XVEC_LAYOUT_BCT) return NPLDA_EINVAL;
    if (bad_pooling(pooling)) return NPLDA_EINVAL;
    *nothing = n == 0;
    if (*nothing) return NPLDA_OK;
    if (!none_null(ptrs) || !all_aligned16(aligned) || ldx < kEmbDim || (ldx % 4) != 0) return NPLDA_EINVAL;
    if (layout == NPLDA_XVEC_LAYOUT_ROWS && ld_in < kFeat) return NPLDA_EINVAL;
    if (layout == NPLDA_XVEC_LAYOUT_BCT && (total_frames % n) != 0) return NPLDA_EINVAL;
    return NPLDA_OK;
}

}  // namespace nplda_xvec

namespace {

using namespace nplda_xvec;

// the caller's frames -> the (rows, 32) zero-padded image (the only kernel that reads the caller's input)
__global__ void xvec_prep_kernel(const float* __restrict__ x, int layout, long long ld_in, long long T, long long R,
                                 long long rows, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * kFeatP) return;
    const long long r = idx / kFeatP;
    const int i = (int)(idx - r * kFeatP);
    float v = 0.f;
    if (r < R && i < kFeat) {
        if (layout == NPLDA_XVEC_LAYOUT_ROWS) {
            v = x[r * ld_in + i];
        } else {
            const long long u = r / T, t = r - u * T;
            v = x[(u * kFeat + i) * T + t];
        }
    }
    out[idx] = v;
}

constexpr int kPoolBlocks = (kPoolDim + 255) / 256;  // pooling blocks per utterance

__global__ __launch_bounds__(256) void xvec_pool_kernel(const float* __restrict__ h, long long ldh,
                                                         const int64_t* __restrict__ offsets, long long R, int pooling,
                                                         float* __restrict__ pooled) {
    const long long u = blockIdx.x / kPoolBlocks;
    const int cb = (int)(blockIdx.x - u * kPoolBlocks), col = cb * 256 + threadIdx.x;
    float* prow = pooled + u * kPooledLd;
    if (cb == 0 && threadIdx.x < kPooledLd - 2 * kPoolDim) prow[2 * kPoolDim + threadIdx.x] = 0.f;
    if (col >= kPoolDim) return;
    long long b = offsets[u], e = offsets[u + 1];  // clamped: a bad offset table must not read outside the rows
    b = b < 0 ? 0 : (b > R ? R : b);
    e = e < b ? b : (e > R ? R : e);
    const long long n = e - b - kContext;
    const float* p = h + b * ldh + col;
    double s = 0.0;
    for (long long t = 0; t < n; ++t) s += (double)p[t * ldh];
    const double mean = n > 0 ? s / (double)n : __builtin_nan("");
    double q = 0.0;
    for (long long t = 0; t < n; ++t) {
        const double dv = (double)p[t * ldh] - mean;
        q += dv * dv;
    }
    const double var = n > 1 ? q / (double)(n - 1) : __builtin_nan("");  // unbiased (correction = 1): NaN at n = 1
    prow[col] = (float)mean;
    prow[kPoolDim + col] = (float)(pooling == NPLDA_XVEC_POOL_VAR ? var : sqrt(var));
}

}  // namespace
