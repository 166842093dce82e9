// nplda_mfcc.hip — Kaldi-compatible MFCCs (compute-mfcc-feats with --dither=0) from 16-bit audio on gfx950: the first stage
// of the speaker-verification pipeline, in front of nplda_feat.hip.  design/k14_mfcc.md.
//
// One frame is a chain of three matrix products, N samples -> P/2 cosine and P/2 sine sums -> B mel bins -> C cepstra, with
// two pointwise steps between them (re^2 + im^2, log).  One kernel; a block of four waves takes TM = 32 consecutive OUTPUT
// frames, which may belong to several utterances:
//
//   1. pre-processing, a wave per frame (eight frames each), plain fp32 on the VALU: the N samples with reflected indices
//      at the utterance's edges (never outside [offset_u, offset_u+1)), the frame mean from an exact integer sum, the raw
//      energy, pre-emphasis and the window; the result is a row of the LDS tile x[frame][sample].  DC removal and
//      pre-emphasis are NOT folded into the DFT matrix: with a recording offset of a few thousand counts the folded form
//      cancels in fp32.
//   2. GEMM 1 on v_mfma_f32_16x16x4_f32, transposed as everywhere in this library: the DFT table is the A operand, streamed
//      from its fragment image in L2 a k16-step ahead (800 KB at 16 kHz: L2-resident, not LDS-resident), the frames are the
//      B operand, one ds_read_b128 per lane, row group and k16-step.  Wave w owns bins [w P/8, (w + 1) P/8): their cosine
//      AND sine blocks, so that re^2 + im^2 is formed on the accumulators.  The even and the odd k16-steps go to two sets
//      of accumulators that are added at the end: two chains of N / 8 terms round less than one of N / 4.
//   3. GEMM 2 (P/2 -> B): an accumulator fragment holds, for frame j, bins 4 g .. 4 g + 3 of its block — with the
//      k-permutation of the fragment images that IS the B operand of the next product, no shuffle.  Every wave sums over
//      its own bins; the four partial sums meet in LDS and are added in the order of the waves, then the floor, and logf
//      of the energy scaled by the power of two 2^-k next below the frame's windowed energy: log mel energies near 25 (the
//      samples are int16 counts) would round to 2e-6 each and the lifter multiplies that by up to 12; near 0 they keep
//      their bits.  The shift -k ln 2 is common to a frame's bins, and the rows c >= 1 of the DCT sum to zero.
//   4. GEMM 3 (B -> C, the DCT with the lifter folded in) from LDS; c0 <- log energy or, without use_energy, c0 + k ln 2
//      times the sum of the DCT's row 0; one coalesced store of TM x C floats.
//
// Every sum has a fixed order and there are no atomics: two calls give the same bits, and a frame's row does not depend on
// the batch it is in (a frame's column of every product is independent of the other columns).
#include "nplda_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int TM = NPLDA_MFCC_TILE;  // frames per block: two 16-column groups of the MFMA
constexpr int NT = 256, NW = 4;      // threads, waves per block
constexpr int FPW = TM / NW;         // frames a wave pre-processes
constexpr int LP = TM + 4;           // row stride of the partial mel sums: 4 LP = 16 (mod 64), the four k-groups on other banks

struct MfccArgs {
    const int16_t* samples;
    const int64_t* soff;  // U + 1 sample offsets
    const int64_t* foff;  // U + 1 frame offsets
    int U;
    int64_t R;
    int N, S, snip, B, C, KB, lda;
    int remove_dc, use_energy, raw_energy, has_floor;
    float preemph, log_floor;
    double row0_ln2;  // ln 2 times the sum of the DCT image's row 0: what a shift of the log mel energies by ln 2 adds to c0
    const float* window;
    const f32x4* dft;   // [KB][NW][2 NBW][64]
    const f32x4* bank;  // [P/32][MB][64]
    const f32x4* dct;   // [MB][MB][64]
    float* out;
};

// The utterance that holds global frame r: the last u with foff[u] <= r (utterances of no frames are stepped over).
__device__ inline int utt_of(const int64_t* __restrict__ offsets, int U, int64_t r) {
    int lo = 0, hi = U;  // invariant: offsets[lo] <= r < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// NBW: 16-bin blocks per wave (P / 128), MB: 16-blocks of the mel bins and of the cepstra (2: B <= 32, 4: B <= 64)
template <int NBW, int MB>
__global__ __launch_bounds__(NT, 2) void mfcc_kernel(const MfccArgs a) {
    constexpr int LDM = 16 * MB + 4;  // row stride of the log mel energies: LDM / 4 odd, ds_read_b128 without conflicts
    constexpr int LDT = 16 * MB + 1;  // row stride of the output tile
    extern __shared__ f32x4 dyn4[];   // x[TM][lda], then the partial mel sums [NW][16 MB][LP]
    __shared__ f32x4 me4[TM * LDM / 4];
    __shared__ float tile[TM * LDT];
    __shared__ float loge[TM];
    __shared__ float mscale[TM];  // 2^-k of the frame, k the binary exponent of its windowed energy
    __shared__ int mexp[TM];      // k
    float* const dyn = reinterpret_cast<float*>(dyn4);
    float* const me = reinterpret_cast<float*>(me4);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * TM;
    const int lda = a.lda, N = a.N, K16 = 16 * a.KB;

    // ---- 1. the frames of this tile, a wave per frame ---------------------------------------------------------------------
    for (int q = 0; q < FPW; ++q) {
        const int fi = wave * FPW + q;
        const int64_t r = r0 + fi;
        float* row = dyn + fi * lda;
        if (r >= a.R) {  // beyond the last frame: a row of zeros, never stored
            for (int i = lane; i < K16; i += 64) row[i] = 0.f;
            if (lane == 0) { loge[fi] = 0.f; mscale[fi] = 1.f; mexp[fi] = 0; }
            continue;
        }
        const int u = utt_of(a.foff, a.U, r);
        const int64_t so = a.soff[u], n = a.soff[u + 1] - so;
        int64_t start = (r - a.foff[u]) * a.S;
        if (!a.snip) start += a.S / 2 - N / 2;
        const int16_t* src = a.samples + so;
        float v[8];
        int isum = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int i = lane + 64 * t;
            int s = 0;
            if (i < N && n > 0) {
                int64_t p = start + i;
                if (p < 0 || p >= n) {  // reflected until inside: i < 0 -> -i - 1, i >= n -> 2 n - 1 - i, period 2 n
                    int64_t m = p % (2 * n);
                    if (m < 0) m += 2 * n;
                    p = m < n ? m : 2 * n - 1 - m;
                }
                s = src[p];
            }
            isum += s;
            v[t] = (float)s;
        }
        isum = wave_sum(isum);  // |sum| <= 512 * 32768: exact
        const float mean = a.remove_dc ? (float)isum / (float)N : 0.f;
        float e = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (lane + 64 * t < N) v[t] -= mean;
            e = fmaf(v[t], v[t], e);
        }
        const float c = a.preemph;
        float y[8], ew = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float prev = __shfl_up(v[t], 1, 64);  // lane 0 keeps its own value: x[0] -= c x[0]
            if (t > 0) {
                const float last = __shfl(v[t - 1], 63, 64);
                if (lane == 0) prev = last;
            }
            const int i = lane + 64 * t;
            y[t] = i < N ? (v[t] - c * prev) * a.window[i] : 0.f;
            ew = fmaf(y[t], y[t], ew);
            if (i < K16) row[i] = y[t];
        }
        const float ews = wave_sum(ew);
        if (a.use_energy) {
            float le = logf(fmaxf(a.raw_energy ? wave_sum(e) : ews, FLT_EPSILON));
            if (a.has_floor) le = fmaxf(le, a.log_floor);
            if (lane == 0) loge[fi] = le;
        }
        int kx;
        (void)frexpf(fmaxf(ews, FLT_EPSILON), &kx);  // ews <= 512 (2^17)^2: |kx| <= 44, 2^-kx and floor * 2^-kx are normal
        if (lane == 0) { mscale[fi] = ldexpf(1.f, -kx); mexp[fi] = kx; }
    }
    __syncthreads();

    // ---- 2. GEMM 1: (cos | sin)[bin][frame] = sum_n table[n][bin] x[frame][n] ------------------------------------------------
    constexpr int NU = 2 * NBW;              // this wave's blocks: NBW of cosines, then the same bins' sines
    constexpr int KSTRIDE = NW * NU * 64;    // f32x4 per k16-step of the image
    const f32x4* dw = a.dft + (size_t)wave * NU * 64 + lane;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][NU], odd[2][NU];            // the even k16-steps, the odd ones
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[0][u] = acc[1][u] = odd[0][u] = odd[1][u] = zero4;
    f32x4 cur[NU], nxt[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) cur[u] = dw[u * 64];
    const float* xb0 = dyn + j * lda + 4 * g;
    const float* xb1 = xb0 + 16 * lda;
    const int KB = a.KB;
    for (int kb = 0; kb < KB; kb += 2) {
        const int k1 = kb + 1 < KB ? kb + 1 : KB - 1, k2 = kb + 2 < KB ? kb + 2 : KB - 1;
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
        if (kb + 1 < KB) {
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

    // ---- 3. power on the accumulators, GEMM 2 over this wave's bins ---------------------------------------------------------
    f32x4 acc2[2][MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc2[0][mb] = acc2[1][mb] = zero4;
#pragma unroll
    for (int u = 0; u < NBW; ++u) {
        const f32x4 p0 = acc[0][u] * acc[0][u] + acc[0][u + NBW] * acc[0][u + NBW];
        const f32x4 p1 = acc[1][u] * acc[1][u] + acc[1][u + NBW] * acc[1][u + NBW];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const f32x4 av = a.bank[((size_t)(wave * NBW + u) * MB + mb) * 64 + lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc2[0][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], p0[r], acc2[0][mb], 0, 0, 0);
                acc2[1][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], p1[r], acc2[1][mb], 0, 0, 0);
            }
        }
    }
    __syncthreads();  // every wave is done with x: its LDS takes the partial sums
    float* part = dyn + wave * (16 * MB * LP);
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i) part[(16 * mb + 4 * g + i) * LP + 16 * rg + j] = acc2[rg][mb][i];
    __syncthreads();
    for (int k = tid; k < TM * 16 * MB; k += NT) {
        const int f = k % TM, b = k / TM;
        const float* p = dyn + b * LP + f;
        const float s = ((p[0] + p[16 * MB * LP]) + p[2 * 16 * MB * LP]) + p[3 * 16 * MB * LP];
        me[f * LDM + b] = b < a.B ? logf(fmaxf(s, FLT_EPSILON) * mscale[f]) : 0.f;
    }
    __syncthreads();

    // ---- 4. GEMM 3: the DCT (lifter folded in), a (16 cepstra x 16 frames) block per wave and pass ---------------------------
    for (int t = wave; t < 2 * MB; t += NW) {
        const int rg = t & 1, cb = t >> 1;
        f32x4 acc3 = zero4;
#pragma unroll
        for (int kb = 0; kb < MB; ++kb) {
            const f32x4 av = a.dct[(kb * MB + cb) * 64 + lane];
            const f32x4 bv = *reinterpret_cast<const f32x4*>(me + (16 * rg + j) * LDM + 16 * kb + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv[r], acc3, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(16 * rg + j) * LDT + 16 * cb + 4 * g + i] = acc3[i];
    }
    __syncthreads();
    const int64_t left = a.R - r0;
    const int C = a.C, nout = (int)(left < TM ? left : TM) * C;
    float* o = a.out + r0 * C;
    for (int k = tid; k < nout; k += NT) {
        const int f = k / C, c = k - f * C;
        float v = tile[f * LDT + c];
        if (c == 0) v = a.use_energy ? loge[f] : (float)((double)v + (double)mexp[f] * a.row0_ln2);
        o[k] = v;
    }
}

inline int kb_of(int N) { return (N + 15) / 16; }

inline bool geometry_ok(const nplda_mfcc_geometry* q) {
    return q->N > 0 && (q->N % 4) == 0 && q->N <= 512 && (q->P == 256 || q->P == 512) && q->N <= q->P && q->B > 0 &&
           q->B <= 64 && q->C > 0 && q->C <= q->B;
}

template <int NBW, int MB>
int launch(const MfccArgs& a, size_t lds, unsigned tiles, hipStream_t st) {
    const hipError_t e = hipFuncSetAttribute((const void*)mfcc_kernel<NBW, MB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((mfcc_kernel<NBW, MB>), dim3(tiles), dim3(NT), lds, st, a);
    return nplda_launch_status();
}

}  // namespace

extern "C" {

size_t nplda_mfcc_image_bytes(const nplda_mfcc_geometry* geometry, int which) {
    if (!geometry || !geometry_ok(geometry)) return 0;
    const size_t MB = geometry->B <= 32 ? 2 : 4;
    switch (which) {
        case 0: return (size_t)kb_of(geometry->N) * (size_t)(geometry->P / 16) * 1024;
        case 1: return (size_t)(geometry->P / 32) * MB * 1024;
        case 2: return MB * MB * 1024;
        default: return 0;
    }
}

int nplda_mfcc_frames_f32(const int16_t* samples, const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts,
                          int64_t total_frames, const nplda_mfcc_geometry* geometry, const float* window, const void* dft_image,
                          const void* bank_image, const void* dct_image, float* out, nplda_stream_t stream) {
    if (!geometry || n_utts < 0 || total_frames < 0 || n_utts > INT32_MAX) return NPLDA_EINVAL;
    if (!geometry_ok(geometry)) return NPLDA_EUNSUPPORTED;
    if (geometry->S <= 0 || geometry->energy_floor < 0.f) return NPLDA_EINVAL;
    if (n_utts == 0 || total_frames == 0) return NPLDA_OK;
    if (!samples || !sample_offsets || !frame_offsets || !window || !dft_image || !bank_image || !dct_image || !out ||
        !nplda_aligned16(dft_image) || !nplda_aligned16(bank_image) || !nplda_aligned16(dct_image))
        return NPLDA_EINVAL;
    const int64_t tiles = (total_frames + TM - 1) / TM;
    if (tiles > INT32_MAX) return NPLDA_EUNSUPPORTED;
    MfccArgs a;
    a.samples = samples; a.soff = sample_offsets; a.foff = frame_offsets; a.U = (int)n_utts; a.R = total_frames;
    a.N = geometry->N; a.S = geometry->S; a.snip = geometry->snip_edges != 0; a.B = geometry->B; a.C = geometry->C;
    a.KB = kb_of(a.N); a.lda = 16 * a.KB + 4;
    a.remove_dc = (geometry->flags & NPLDA_MFCC_REMOVE_DC) != 0;
    a.use_energy = (geometry->flags & NPLDA_MFCC_USE_ENERGY) != 0;
    a.raw_energy = (geometry->flags & NPLDA_MFCC_RAW_ENERGY) != 0;
    a.has_floor = geometry->energy_floor > 0.f;
    a.preemph = geometry->preemph;
    a.log_floor = a.has_floor ? logf(geometry->energy_floor) : 0.f;
    a.row0_ln2 = M_LN2 * (double)a.B * (double)(float)sqrt(1.0 / (double)a.B);  // row 0 of the image: B times float(sqrt(1 / B))
    a.window = window;
    a.dft = (const f32x4*)dft_image; a.bank = (const f32x4*)bank_image; a.dct = (const f32x4*)dct_image;
    a.out = out;
    const int MB = a.B <= 32 ? 2 : 4;
    size_t lds = (size_t)TM * a.lda * sizeof(float);
    const size_t part = (size_t)NW * 16 * MB * LP * sizeof(float);
    if (part > lds) lds = part;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nt = (unsigned)tiles;
    if (geometry->P == 512) return MB == 2 ? launch<4, 2>(a, lds, nt, st) : launch<4, 4>(a, lds, nt, st);
    return MB == 2 ? launch<2, 2>(a, lds, nt, st) : launch<2, 4>(a, lds, nt, st);
}

}  // extern "C"
