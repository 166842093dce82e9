// nplda_augment.hip — K28: augmentation of 16-bit audio on gfx950, the step between the wave files and nplda_mfcc.hip:
// reverberation with a room impulse response and additive noise at a given SNR.  design/k28_augment.md.
//
// The convolution x * h is uniformly partitioned overlap-save with block B = 256 and transform size P = 512:
//   X_b = DFT of samples [(b - 1) B, (b + 1) B) of the zero-extended signal, H_p = DFT of taps [p B, (p + 1) B) padded to P,
//   Y_b = sum over p (ascending) of X_{b-p} . H_p, block b of x * h = the last B samples of the inverse DFT of Y_b.
// A real spectrum is kept as P floats: [0, 256) the real parts of bins 0 .. 255, [256] the Nyquist bin (real), [256 + k] the
// imaginary part of bin k = 1 .. 255.  Both transforms are matrix products against constant tables on
// v_mfma_f32_16x16x4_f32, in the shape of GEMM 1 of nplda_mfcc.hip: the table is the A operand, streamed from its fragment
// image in L2 a k16-step ahead, the tile's 32 columns (consecutive blocks of the batch-wide block list, which may belong to
// several utterances) are the B operand in LDS, the even and the odd k16-steps go to two sets of accumulators.
//
// Launches of a call (the count depends on the shapes only):
//   aug_clear_kernel (the integer sums and counts), aug_power_kernel (P_in), then, if any utterance has a RIR: aug_dft_kernel<SIGNAL> (X),
//   aug_mac_kernel (Y), aug_dft_kernel<SYNTH> (x * h), aug_mac_kernel on the early window, aug_dft_kernel<SYNTH_POWER>
//   (per-block sums of squares only); aug_scalars_kernel<0> (P_in, P_sig, the scales s), aug_mix_sum_kernel (partial sums of
//   P_mix), aug_scalars_kernel<1> (the gains), aug_store_kernel (mix again, scale, round, store).
//
// Every floating-point sum has a fixed order that is anchored at the utterance (blocks, groups and chunks are counted from its
// first sample), the only atomics add integers: two calls give the same bits and a result does not depend on the batch.
#include "nplda_common.h"

#include <limits.h>
#include <math.h>

#include <atomic>

namespace {

constexpr int BS = NPLDA_AUGMENT_BLOCK;  // samples per block
constexpr int PS = 2 * BS;               // transform size = floats per spectrum
constexpr int TM = NPLDA_AUGMENT_TILE;   // columns per thread block: two 16-column groups of the MFMA
constexpr int NT = 256, NW = 4;          // threads, waves per thread block
constexpr int CPW = TM / NW;             // columns a wave loads
constexpr int LDX = PS + 4;              // row stride of the tile: LDX / 4 odd, ds_read_b128 of sixteen rows without conflicts
constexpr int KB = PS / 16;              // k16-steps
constexpr int GRP = NPLDA_AUGMENT_GROUP;
constexpr int CH = NPLDA_AUGMENT_CHUNK;
constexpr int CPT = CH / NT;             // samples per thread of a chunk

static_assert(BS == 256 && NT == BS && TM == 32 && CH % NT == 0, "the kernels are written for these sizes");

// The item that holds global index r of a cumulative int32 table: the last i with off[i] <= r (empty items are stepped over).
__device__ inline int item_of(const int32_t* __restrict__ off, int I, int r) {
    int lo = 0, hi = I;  // invariant: off[lo] <= r < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the two transforms ------------------------------------------------------------------------------------------------------

enum { SIGNAL = 0, FILTER = 1, SYNTH = 2, SYNTH_POWER = 3 };

struct DftArgs {
    const void* src;         // SIGNAL: int16 samples; FILTER: float taps; SYNTH*: spectra, PS floats per column
    const int64_t* src_off;  // SIGNAL / FILTER: the item's first element
    const int32_t* src_len;  // SIGNAL / FILTER: its length; SYNTH_POWER: the valid samples of the item's output
    const int32_t* blk_off;  // I + 1: the item's columns
    int I, R;                // items, columns
    const f32x4* table;      // [KB][NW][NU][64]
    float* out;              // SIGNAL / FILTER: R x PS spectra; SYNTH: R x BS samples
    double* part;            // SYNTH_POWER: R sums of squares
};

template <int MODE>
__global__ __launch_bounds__(NT, 2) void aug_dft_kernel(const DftArgs a) {
    constexpr int NU = MODE < SYNTH ? 8 : 4;  // 16-row blocks of the output per wave: 512 or 256 rows in all
    extern __shared__ f32x4 dyn4[];           // x[TM][LDX]
    __shared__ int valid[TM];                 // SYNTH_POWER: samples of the column that count
    __shared__ double wsum[NW][TM];
    float* const x = reinterpret_cast<float*>(dyn4);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int r0 = blockIdx.x * TM;

    // ---- 1. the tile's columns, a wave per column ---------------------------------------------------------------------------
    for (int q = 0; q < CPW; ++q) {
        const int c = wave * CPW + q, r = r0 + c;
        float* row = x + c * LDX;
        if (r >= a.R) {  // beyond the last column: zeros, never stored
#pragma unroll
            for (int t = 0; t < PS / 64; ++t) row[lane + 64 * t] = 0.f;
            if (MODE == SYNTH_POWER && lane == 0) valid[c] = 0;
            continue;
        }
        if (MODE == SIGNAL || MODE == FILTER) {
            const int it = item_of(a.blk_off, a.I, r);
            const int64_t b = r - a.blk_off[it], n = a.src_len[it], off = a.src_off[it];
#pragma unroll
            for (int t = 0; t < PS / 64; ++t) {
                const int i = lane + 64 * t;
                float v = 0.f;
                if (MODE == SIGNAL) {  // samples [(b - 1) BS, (b + 1) BS) of the zero-extended utterance
                    const int64_t p = (b - 1) * BS + i;
                    if (p >= 0 && p < n) v = (float)static_cast<const int16_t*>(a.src)[off + p];
                } else {               // taps [b BS, (b + 1) BS), then BS zeros
                    const int64_t p = b * BS + i;
                    if (i < BS && p < n) v = static_cast<const float*>(a.src)[off + p];
                }
                row[i] = v;
            }
        } else {
            const float* y = static_cast<const float*>(a.src) + (size_t)r * PS;
#pragma unroll
            for (int t = 0; t < PS / 64; ++t) row[lane + 64 * t] = y[lane + 64 * t];
            if (MODE == SYNTH_POWER && lane == 0) {
                const int it = item_of(a.blk_off, a.I, r);
                const int64_t left = (int64_t)a.src_len[it] - (int64_t)(r - a.blk_off[it]) * BS;
                valid[c] = left <= 0 ? 0 : left >= BS ? BS : (int)left;
            }
        }
    }
    __syncthreads();

    // ---- 2. out[row][column] = sum_k table[row][k] x[column][k] ----------------------------------------------------------------
    constexpr int KSTRIDE = NW * NU * 64;  // f32x4 per k16-step of the image
    const f32x4* dw = a.table + (size_t)wave * NU * 64 + lane;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][NU], odd[2][NU];          // the even k16-steps, the odd ones
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[0][u] = acc[1][u] = odd[0][u] = odd[1][u] = zero4;
    f32x4 cur[NU], nxt[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) cur[u] = dw[u * 64];
    const float* xb0 = x + j * LDX + 4 * g;
    const float* xb1 = xb0 + 16 * LDX;
    for (int kb = 0; kb < KB; kb += 2) {
        const int k1 = kb + 1, k2 = kb + 2 < KB ? kb + 2 : KB - 1;
#pragma unroll
        for (int u = 0; u < NU; ++u) nxt[u] = dw[(size_t)k1 * KSTRIDE + u * 64];
        {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(xb0 + 16 * kb);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(xb1 + 16 * kb);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    acc[0][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][r], b0[r], acc[0][u], 0, 0, 0);
                    acc[1][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][r], b1[r], acc[1][u], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) cur[u] = dw[(size_t)k2 * KSTRIDE + u * 64];
        {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(xb0 + 16 * k1);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(xb1 + 16 * k1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    odd[0][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(nxt[u][r], b0[r], odd[0][u], 0, 0, 0);
                    odd[1][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(nxt[u][r], b1[r], odd[1][u], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        acc[0][u] += odd[0][u];
        acc[1][u] += odd[1][u];
    }

    // ---- 3. lane 16 g + j holds rows 16 (wave NU + u) + 4 g .. + 3 of column 16 rg + j ---------------------------------------
    if (MODE != SYNTH_POWER) {
        constexpr int LDO = MODE == SYNTH ? BS : PS;
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
            const int r = r0 + 16 * rg + j;
            if (r < a.R) {
                float* o = a.out + (size_t)r * LDO + 16 * (wave * NU) + 4 * g;
#pragma unroll
                for (int u = 0; u < NU; ++u) *reinterpret_cast<f32x4*>(o + 16 * u) = acc[rg][u];
            }
        }
    } else {
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
            const int v = valid[16 * rg + j];
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double d = 16 * (wave * NU + u) + 4 * g + i < v ? (double)acc[rg][u][i] : 0.0;
                    s += d * d;  // the product of two floats is exact in double
                }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (g == 0) wsum[wave][16 * rg + j] = s;
        }
        __syncthreads();
        if (tid < TM && r0 + tid < a.R) a.part[r0 + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
    }
}

template <int MODE>
int launch_dft(const DftArgs& a, hipStream_t st) {
    const size_t lds = (size_t)TM * LDX * sizeof(float);
    // 66 KB of dynamic LDS want the attribute: set once per process, instance and device (bit d of `set`), so that a warmed
    // call issues no attribute call inside a stream capture
    static std::atomic<uint64_t> set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const uint64_t bit = dev >= 0 && dev < 64 ? (uint64_t)1 << dev : 0;
    if (!(set.load(std::memory_order_acquire) & bit)) {
        e = hipFuncSetAttribute((const void*)aug_dft_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        set.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL((aug_dft_kernel<MODE>), dim3((unsigned)((a.R + TM - 1) / TM)), dim3(NT), lds, st, a);
    return nplda_launch_status();
}

// ---- Y_b = sum_p X_{b-p} . H_p on the VALU -----------------------------------------------------------------------------------

struct MacArgs {
    const float* X;          // the batch's spectra
    const float* H;          // the filters' spectra
    const int32_t* blk_off;  // U + 1
    const int32_t* grp_off;  // U + 1
    const int32_t* rir_of;   // U
    const int32_t* parts;    // [rir][4]
    int U, early;
    float* Y;
};

// A thread block takes GRP consecutive blocks of one utterance, thread t bin t (thread 0: the DC and the Nyquist bin, both
// real).  The GRP spectra X_{b0 + j - p} slide through registers: a step of p loads one H_p and one X.
__global__ __launch_bounds__(NT) void aug_mac_kernel(const MacArgs a) {
    const int t = threadIdx.x;
    const int u = item_of(a.grp_off, a.U, (int)blockIdx.x);
    const int b0 = ((int)blockIdx.x - a.grp_off[u]) * GRP;
    const int base = a.blk_off[u], nb = a.blk_off[u + 1] - base;
    const int32_t* pr = a.parts + 4 * a.rir_of[u] + (a.early ? 2 : 0);
    const float* X = a.X + (size_t)base * PS + t;
    const float* H = a.H + (size_t)pr[0] * PS + t;
    const int np = pr[1], pmax = np < b0 + GRP ? np : b0 + GRP;
    float xr[GRP], xi[GRP], yr[GRP], yi[GRP];
#pragma unroll
    for (int j = 0; j < GRP; ++j) {
        const bool ok = b0 + j < nb;
        xr[j] = ok ? X[(size_t)(b0 + j) * PS] : 0.f;
        xi[j] = ok ? X[(size_t)(b0 + j) * PS + BS] : 0.f;
        yr[j] = yi[j] = 0.f;
    }
    for (int p = 0; p < pmax; ++p) {
        const float hr = H[(size_t)p * PS], hi = H[(size_t)p * PS + BS];
        if (t == 0) {
#pragma unroll
            for (int j = 0; j < GRP; ++j) {
                yr[j] += xr[j] * hr;
                yi[j] += xi[j] * hi;
            }
        } else {
#pragma unroll
            for (int j = 0; j < GRP; ++j) {
                yr[j] += xr[j] * hr - xi[j] * hi;
                yi[j] += xr[j] * hi + xi[j] * hr;
            }
        }
#pragma unroll
        for (int j = GRP - 1; j > 0; --j) {
            xr[j] = xr[j - 1];
            xi[j] = xi[j - 1];
        }
        const int idx = b0 - p - 1;
        xr[0] = idx >= 0 ? X[(size_t)idx * PS] : 0.f;
        xi[0] = idx >= 0 ? X[(size_t)idx * PS + BS] : 0.f;
    }
    float* Y = a.Y + (size_t)base * PS + t;
#pragma unroll
    for (int j = 0; j < GRP; ++j)
        if (b0 + j < nb) {
            Y[(size_t)(b0 + j) * PS] = yr[j];
            Y[(size_t)(b0 + j) * PS + BS] = yi[j];
        }
}

// ---- exact sums of squares of int16 items ------------------------------------------------------------------------------------

// The integer sums and counts start from zero.  A kernel, not hipMemsetAsync: replayed from a captured graph the memset node of
// the 96-byte `clipped` array left a 16-byte pattern in it instead of zeros (tests/test_augment_gpu.py, the graph test).
__global__ void aug_clear_kernel(unsigned long long* sums, int32_t* counts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        sums[i] = 0;
        if (counts) counts[i] = 0;
    }
}

__global__ __launch_bounds__(NT) void aug_power_kernel(const int16_t* __restrict__ s, const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ coff, int I, unsigned long long* sums) {
    __shared__ unsigned long long ws[NW];
    const int tid = threadIdx.x, c = (int)blockIdx.x;
    const int it = item_of(coff, I, c);
    const int64_t base = off[it], n = off[it + 1] - base, t0 = (int64_t)(c - coff[it]) * CH;
    unsigned long long acc = 0;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int64_t t = t0 + i * NT + tid;
        if (t < n) {
            const int v = s[base + t];
            acc += (unsigned long long)(v * v);
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) ws[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) atomicAdd(sums + it, ws[0] + ws[1] + ws[2] + ws[3]);  // integers: any order, the same sum
}

// ---- the element-wise path: mix, scalars, store -------------------------------------------------------------------------------

struct MixArgs {
    const int16_t* samples;
    const nplda_augment_utt* utts;
    const nplda_augment_entry* entries;
    const int32_t* chunk_off;  // U + 1, over n_out
    const int32_t* blk_off;    // U + 1
    int U;
    const float* y;            // x * h, block-aligned per utterance
    const int16_t* noise;
    const long long* noise_sums;
    const long long* isum;     // U: sum of x^2
    const double* epart;       // per block: sums of squares of x * h[a:b]
    double* mpart;             // per output chunk: sums of squares of the mix
    float* pin;                // U
    float* gain;               // U
    float* scale;              // E
    void* out;
    int32_t* clipped;
};

// Sample t of the mix of utterance q: separate float32 multiplies and adds in list order.  The pragma is what keeps them
// separate: hipcc contracts a * b + c to an fma by default, through __fmul_rn / __fadd_rn too (they are plain operators).
__device__ __forceinline__ float mixed(const MixArgs& a, const nplda_augment_utt& q, int t) {
#pragma clang fp contract(off)
    float v = q.rir >= 0 ? a.y[q.y_off + q.shift + t] : (float)a.samples[q.in_off + t];
    for (int e = 0; e < q.ent_count; ++e) {
        const nplda_augment_entry& en = a.entries[q.ent_begin + e];
        const float s = a.scale[q.ent_begin + e];
        const int d = t - en.start;
        if (s != 0.f && d >= 0 && (en.repeat || d < en.len)) v = v + s * (float)a.noise[en.noise_off + d % en.len];
    }
    return v;
}

// STAGE 0, before the mix: P_in, P_sig and the entries' scales; STAGE 1, after it: the gain.  A thread per utterance; every
// scalar is a float64 expression of float32-rounded powers, rounded once.
template <int STAGE>
__global__ void aug_scalars_kernel(const MixArgs a) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    const nplda_augment_utt q = a.utts[u];
    if (STAGE == 0) {
        const float pin = q.n > 0 ? (float)((double)a.isum[u] / (double)q.n) : 0.f;
        float psig = pin;
        if (q.rir >= 0) {
            double s = 0.0;
            for (int b = a.blk_off[u]; b < a.blk_off[u + 1]; ++b) s += a.epart[b];
            psig = q.n_early > 0 ? (float)(s / (double)q.n_early) : 0.f;
        }
        a.pin[u] = pin;
        for (int e = q.ent_begin; e < q.ent_begin + q.ent_count; ++e) {
            const nplda_augment_entry en = a.entries[e];
            const float pn = en.len > 0 ? (float)((double)a.noise_sums[en.item] / (double)en.len) : 0.f;
            a.scale[e] = pn > 0.f ? (float)sqrt(en.ratio * (double)psig / (double)pn) : 0.f;
        }
    } else {
        float gn = 1.f;
        if (q.volume > 0.f) {
            gn = q.volume;
        } else if (q.normalize) {
            double s = 0.0;
            for (int c = a.chunk_off[u]; c < a.chunk_off[u + 1]; ++c) s += a.mpart[c];
            const float pmix = q.n_out > 0 ? (float)(s / (double)q.n_out) : 0.f;
            if (pmix > 0.f) gn = (float)sqrt((double)a.pin[u] / (double)pmix);
        }
        a.gain[u] = gn;
    }
}

__global__ __launch_bounds__(NT) void aug_mix_sum_kernel(const MixArgs a) {
    __shared__ double ws[NW];
    const int tid = threadIdx.x, c = (int)blockIdx.x;
    const int u = item_of(a.chunk_off, a.U, c);
    const nplda_augment_utt q = a.utts[u];
    const int64_t t0 = (int64_t)(c - a.chunk_off[u]) * CH;
    double acc = 0.0;
    if (q.volume <= 0.f && q.normalize) {  // otherwise the gain does not need P_mix
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int64_t t = t0 + i * NT + tid;
            if (t < q.n_out) {
                const double m = (double)mixed(a, q, (int)t);
                acc += m * m;
            }
        }
    }
    acc = wave_sum(acc);  // (the xor butterfly: the same pairs at every level on every call)
    if ((tid & 63) == 0) ws[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.mpart[c] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

template <bool I16>
__global__ __launch_bounds__(NT) void aug_store_kernel(const MixArgs a) {
    const int tid = threadIdx.x, c = (int)blockIdx.x;
    const int u = item_of(a.chunk_off, a.U, c);
    const nplda_augment_utt q = a.utts[u];
    const int64_t t0 = (int64_t)(c - a.chunk_off[u]) * CH;
    const float gn = a.gain[u];
    int nclip = 0;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
#pragma clang fp contract(off)
        const int64_t t = t0 + i * NT + tid;
        if (t < q.n_out) {
            const float v = gn * mixed(a, q, (int)t);
            if (I16) {
                float r = rintf(v);  // round half to even
                if (r > 32767.f) { r = 32767.f; ++nclip; }
                else if (r < -32768.f) { r = -32768.f; ++nclip; }
                static_cast<int16_t*>(a.out)[q.out_off + t] = (int16_t)(int)r;
            } else {
                static_cast<float*>(a.out)[q.out_off + t] = v;
            }
        }
    }
    if (I16) {
        nclip = wave_sum(nclip);
        if ((tid & 63) == 0 && nclip) atomicAdd(a.clipped + u, nclip);  // integers
    }
}

struct Workspace {
    size_t X, Y, y, epart, mpart, isum, pin, gain, scale, total;
};

inline Workspace workspace(int64_t U, int64_t E, int64_t blocks, int64_t out_chunks) {
    Workspace w;
    size_t o = 0;
    w.X = o; o += up256((size_t)blocks * PS * sizeof(float));
    w.Y = o; o += up256((size_t)blocks * PS * sizeof(float));
    w.y = o; o += up256((size_t)blocks * BS * sizeof(float));
    w.epart = o; o += up256((size_t)blocks * sizeof(double));
    w.mpart = o; o += up256((size_t)out_chunks * sizeof(double));
    w.isum = o; o += up256((size_t)U * sizeof(long long));
    w.pin = o; o += up256((size_t)U * sizeof(float));
    w.gain = o; o += up256((size_t)U * sizeof(float));
    w.scale = o; o += up256((size_t)E * sizeof(float));
    w.total = o;
    return w;
}

inline bool counts_ok(int64_t v) { return v >= 0 && v <= INT_MAX / 2; }

// sums[i] <- sum of squares of item i; counts (if given): n_items zeros
int power(const int16_t* samples, const int64_t* item_off, const int32_t* chunk_off, int64_t n_items, int64_t total_chunks,
          int64_t* sums, int32_t* counts, hipStream_t st) {
    unsigned long long* const acc = reinterpret_cast<unsigned long long*>(sums);
    hipLaunchKernelGGL(aug_clear_kernel, dim3((unsigned)((n_items + NT - 1) / NT)), dim3(NT), 0, st, acc, counts, (int)n_items);
    int rc = nplda_launch_status();
    if (rc != NPLDA_OK || total_chunks == 0) return rc;
    hipLaunchKernelGGL(aug_power_kernel, dim3((unsigned)total_chunks), dim3(NT), 0, st, samples, item_off, chunk_off, (int)n_items,
                       acc);
    return nplda_launch_status();
}

}  // namespace

extern "C" {

size_t nplda_augment_table_bytes(int which) {
    return which == 0 ? (size_t)PS * PS * sizeof(float) : which == 1 ? (size_t)BS * PS * sizeof(float) : 0;
}

int nplda_augment_spectra_f32(const float* src, const int64_t* src_off, const int32_t* src_len, const int32_t* blk_off,
                              int64_t n_filters, int64_t total_blocks, int32_t min_len, int32_t max_len,
                              const void* forward_table, float* spectra, nplda_stream_t stream) {
    if (n_filters < 0 || total_blocks < 0) return NPLDA_EINVAL;
    if (n_filters == 0) return NPLDA_OK;
    if (min_len < 1 || max_len < min_len) return NPLDA_EINVAL;
    if (max_len > NPLDA_AUGMENT_MAX_RIR || !counts_ok(n_filters) || !counts_ok(total_blocks)) return NPLDA_EUNSUPPORTED;
    if (!src || !src_off || !src_len || !blk_off || !forward_table || !spectra || total_blocks < n_filters ||
        !nplda_aligned16(forward_table) || !nplda_aligned16(spectra))
        return NPLDA_EINVAL;
    DftArgs a;
    a.src = src; a.src_off = src_off; a.src_len = src_len; a.blk_off = blk_off; a.I = (int)n_filters; a.R = (int)total_blocks;
    a.table = (const f32x4*)forward_table; a.out = spectra; a.part = nullptr;
    return launch_dft<FILTER>(a, (hipStream_t)stream);
}

int nplda_augment_power_i64(const int16_t* samples, const int64_t* item_off, const int32_t* chunk_off, int64_t n_items,
                            int64_t total_chunks, int64_t* sums, nplda_stream_t stream) {
    if (n_items < 0 || total_chunks < 0) return NPLDA_EINVAL;
    if (n_items == 0) return NPLDA_OK;
    if (!counts_ok(n_items) || !counts_ok(total_chunks)) return NPLDA_EUNSUPPORTED;
    if (!item_off || !chunk_off || !sums || (total_chunks > 0 && !samples)) return NPLDA_EINVAL;
    return power(samples, item_off, chunk_off, n_items, total_chunks, sums, nullptr, (hipStream_t)stream);
}

size_t nplda_augment_workspace_bytes(int64_t n_utts, int64_t n_entries, int64_t total_blocks, int64_t total_out_chunks) {
    if (n_utts < 0 || n_entries < 0 || total_blocks < 0 || total_out_chunks < 0) return 0;
    return workspace(n_utts, n_entries, total_blocks, total_out_chunks).total;
}

int nplda_augment_batch(const nplda_augment_call* c, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    if (!c || c->n_utts < 0 || c->n_entries < 0 || c->total_blocks < 0 || c->total_groups < 0 || c->total_in_chunks < 0 ||
        c->total_out_chunks < 0 || c->max_conv_len < 0 || c->max_rir_len < 0)
        return NPLDA_EINVAL;
    if (c->n_utts == 0) return NPLDA_OK;
    if (c->max_rir_len > NPLDA_AUGMENT_MAX_RIR || c->max_conv_len > (int64_t)INT_MAX - PS || !counts_ok(c->n_utts) ||
        !counts_ok(c->n_entries) || !counts_ok(c->total_blocks) || !counts_ok(c->total_in_chunks) ||
        !counts_ok(c->total_out_chunks))
        return NPLDA_EUNSUPPORTED;
    const bool conv = c->total_blocks > 0;
    if (!c->utts || !c->in_off || !c->in_len || !c->in_chunk_off || !c->out_chunk_off || !c->blk_off || !c->grp_off ||
        !c->rir_of || !c->early_len || !c->clipped || !ws || (c->total_in_chunks > 0 && !c->samples) ||
        (c->total_out_chunks > 0 && !c->out) || (c->n_entries > 0 && (!c->entries || !c->noise || !c->noise_sums)) ||
        (conv && (!c->rir_spectra || !c->rir_parts || !c->forward_table || !c->inverse_table || c->total_groups <= 0 ||
                  !nplda_aligned16(c->forward_table) || !nplda_aligned16(c->inverse_table))) ||
        (((uintptr_t)ws) & 255u))
        return NPLDA_EINVAL;
    const Workspace w = workspace(c->n_utts, c->n_entries, c->total_blocks, c->total_out_chunks);
    if (ws_bytes < w.total) return NPLDA_ENOSPC;
    char* const base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)stream;
    const int U = (int)c->n_utts;
    int rc;

    MixArgs m;
    m.samples = c->samples; m.utts = c->utts; m.entries = c->entries; m.chunk_off = c->out_chunk_off; m.blk_off = c->blk_off;
    m.U = U; m.y = reinterpret_cast<const float*>(base + w.y); m.noise = c->noise;
    m.noise_sums = reinterpret_cast<const long long*>(c->noise_sums);
    m.isum = reinterpret_cast<const long long*>(base + w.isum);
    m.epart = reinterpret_cast<const double*>(base + w.epart); m.mpart = reinterpret_cast<double*>(base + w.mpart);
    m.pin = reinterpret_cast<float*>(base + w.pin); m.gain = reinterpret_cast<float*>(base + w.gain);
    m.scale = reinterpret_cast<float*>(base + w.scale); m.out = c->out; m.clipped = c->clipped;

    rc = power(c->samples, c->in_off, c->in_chunk_off, c->n_utts, c->total_in_chunks, reinterpret_cast<int64_t*>(base + w.isum),
               c->clipped, st);
    if (rc != NPLDA_OK) return rc;

    if (conv) {
        DftArgs d;
        d.src = c->samples; d.src_off = c->in_off; d.src_len = c->in_len; d.blk_off = c->blk_off; d.I = U;
        d.R = (int)c->total_blocks; d.table = (const f32x4*)c->forward_table; d.out = reinterpret_cast<float*>(base + w.X);
        d.part = nullptr;
        if ((rc = launch_dft<SIGNAL>(d, st)) != NPLDA_OK) return rc;
        MacArgs q;
        q.X = reinterpret_cast<const float*>(base + w.X); q.H = c->rir_spectra; q.blk_off = c->blk_off; q.grp_off = c->grp_off;
        q.rir_of = c->rir_of; q.parts = c->rir_parts; q.U = U; q.Y = reinterpret_cast<float*>(base + w.Y);
        d.src = base + w.Y; d.src_off = nullptr; d.table = (const f32x4*)c->inverse_table;
        for (int early = 0; early < 2; ++early) {
            q.early = early;
            hipLaunchKernelGGL(aug_mac_kernel, dim3((unsigned)c->total_groups), dim3(NT), 0, st, q);
            if ((rc = nplda_launch_status()) != NPLDA_OK) return rc;
            if (!early) {
                d.src_len = nullptr; d.out = reinterpret_cast<float*>(base + w.y);
                rc = launch_dft<SYNTH>(d, st);
            } else {
                d.src_len = c->early_len; d.out = nullptr; d.part = reinterpret_cast<double*>(base + w.epart);
                rc = launch_dft<SYNTH_POWER>(d, st);
            }
            if (rc != NPLDA_OK) return rc;
        }
    }

    const unsigned ub = (unsigned)((U + NT - 1) / NT), chunks = (unsigned)c->total_out_chunks;
    hipLaunchKernelGGL(aug_scalars_kernel<0>, dim3(ub), dim3(NT), 0, st, m);
    if ((rc = nplda_launch_status()) != NPLDA_OK) return rc;
    if (chunks) {
        hipLaunchKernelGGL(aug_mix_sum_kernel, dim3(chunks), dim3(NT), 0, st, m);
        if ((rc = nplda_launch_status()) != NPLDA_OK) return rc;
    }
    hipLaunchKernelGGL(aug_scalars_kernel<1>, dim3(ub), dim3(NT), 0, st, m);
    if ((rc = nplda_launch_status()) != NPLDA_OK) return rc;
    if (chunks) {
        if (c->out_i16) hipLaunchKernelGGL(aug_store_kernel<true>, dim3(chunks), dim3(NT), 0, st, m);
        else hipLaunchKernelGGL(aug_store_kernel<false>, dim3(chunks), dim3(NT), 0, st, m);
        if ((rc = nplda_launch_status()) != NPLDA_OK) return rc;
    }
    return NPLDA_OK;
}

}  // extern "C"
