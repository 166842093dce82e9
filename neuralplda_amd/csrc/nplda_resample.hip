// nplda_resample.hip — K29: rational-ratio resampling and speed perturbation of 16-bit audio on gfx950, the step in front of
// nplda_augment.hip and nplda_mfcc.hip.  design/k29_resample.md.
//
// With g = gcd(rin, rout), iu = rin / g, ou = rout / g, output sample k of an utterance is
//     y[k] = gain * sum_t w[k mod ou][t] * x[(k div ou) iu + first[k mod ou] + t],   t = 0 .. taps - 1, x = 0 outside [0, n):
// ou phases of a windowed-sinc filter, built by the caller in float64 from the integer tick distance i ou - k iu and rounded
// once (neuralplda_amd/resample.py).  A phase with fewer weights than `taps` is padded with zeros at its end; first[] does not
// decrease with the phase and first[ou - 1] <= first[0] + iu, so the first input of an output does not decrease with k.
//
// A thread block takes CHUNK consecutive outputs of ONE utterance (the chunk table names the utterance and the chunk's number
// in it): it stages the input span of the chunk in LDS as float32 — 16-byte loads of 8 samples where the vector lies inside
// the utterance, single samples at its two ends, zeros outside — and a thread then forms four outputs of ONE phase (a
// quarter of the chunk apart), each one chain of fused multiply-adds over the taps in increasing input index: a weight (the table, [tap][phase], so
// that consecutive threads read consecutive weights; it stays in L1 / L2) is read once for the four, so a multiply-add costs
// one LDS read and a quarter of a weight read.  `taps` is a multiple of 4 (the caller pads with zero rows): four weights are
// in flight at a time and the loop has no remainder.  The sum of an output does not depend on the chunking, the batch or the
// order.  A ratio index of -1 is a copy times the gain.
//
// Launches of a call: rs_clear_kernel (the saturation counts), rs_kernel.  The only atomics add integers.
#include "nplda_common.h"
#include "nplda_ragged.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int CH = NPLDA_RESAMPLE_CHUNK;  // outputs per thread block
constexpr int NT = 256;                   // threads per thread block
constexpr int OPT = CH / NT;              // outputs per thread
constexpr long long kMaxUtts = INT_MAX / 2;

static_assert(CH % NT == 0 && OPT == 4, "the kernel is written for four outputs per item, an item per thread and pass");

typedef short i16x8 __attribute__((ext_vector_type(8)));

// what an utterance of m output samples takes (csrc/nplda_ragged.h): its chunks
struct ChunkTerms {
    __host__ __device__ void operator()(long long m, long long, long long* terms) const { terms[0] = (m + CH - 1) / CH; }
};

// LDS floats of a chunk: the inputs between the first one of its first output and the last one of its last output, at most
// floor((CH - 1) iu / ou) + 1 + taps, in front of them up to 7 samples down to the 16-byte boundary, whole vectors
__host__ __device__ inline long long span_floats(long long iu, long long ou, long long taps) {
    return ((CH - 1) * iu / ou + 2 + taps + 7 + 7) / 8 * 8;
}

struct Args {
    const int16_t* samples;
    const nplda_resample_utt* utts;
    const nplda_resample_ratio* ratios;
    const int32_t* first;
    const float* weights;
    const int32_t* chunks;  // [total_chunks][2]: utterance, chunk of the utterance
    void* out;
    int32_t* clipped;
    int n_utts, n_ratios, lds_floats;
};

__global__ void rs_clear_kernel(int32_t* counts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// v -> the output: float32 as it is, or int16 by round-half-to-even with saturation (returns 1 if it saturated)
template <bool I16>
__device__ __forceinline__ int store(void* out, int64_t at, float v) {
    if (I16) {
        int clip = 0;
        float r = rintf(v);
        if (r > 32767.f) { r = 32767.f; clip = 1; }
        else if (r < -32768.f) { r = -32768.f; clip = 1; }
        static_cast<int16_t*>(out)[at] = (int16_t)(int)r;
        return clip;
    }
    static_cast<float*>(out)[at] = v;
    return 0;
}

template <bool I16>
__global__ __launch_bounds__(NT, 8) void rs_kernel(const Args a) {
    extern __shared__ float xs[];
    const int tid = threadIdx.x;
    const int u = a.chunks[2 * blockIdx.x], ci = a.chunks[2 * blockIdx.x + 1];
    if (u < 0 || u >= a.n_utts) return;
    const nplda_resample_utt q = a.utts[u];
    const int k0 = ci * CH;
    const int cnt = q.m - k0 < CH ? q.m - k0 : CH;  // uniform over the block
    if (ci < 0 || cnt <= 0 || q.ratio >= a.n_ratios) return;
    const float gain = q.gain;
    int nclip = 0;

    if (q.ratio < 0) {  // equal rates: the sample times the gain
#pragma unroll
        for (int r = 0; r < OPT; ++r) {
            const int j = tid + NT * r;
            if (j < cnt && k0 + j < q.n) nclip += store<I16>(a.out, q.out_off + k0 + j, gain * (float)a.samples[q.in_off + k0 + j]);
        }
    } else {
        const nplda_resample_ratio R = a.ratios[q.ratio];
        const int iu = R.iu, ou = R.ou, taps = R.taps;
        const int32_t* const first = a.first + R.first_off;
        const float* const w = a.weights + R.weight_off;
        const int b0 = k0 / ou, p0 = k0 - b0 * ou;
        const int k1 = k0 + cnt - 1, b1 = k1 / ou, p1 = k1 - b1 * ou;
        const long long lo = (long long)b0 * iu + first[p0];             // the chunk's first input (may lie before 0)
        const long long hi = (long long)b1 * iu + first[p1] + taps;      // one past its last
        const long long g0 = q.in_off + lo, a0 = g0 & ~7LL;              // ... in `samples`; the 16-byte boundary at or below
        const int lead = (int)(g0 - a0);
        const long long need = lead + (hi - lo);
        if (iu <= 0 || ou <= 0 || taps <= 0 || (taps & 3) || hi < lo || need > a.lds_floats) return;  // a table the host did not size for

        // ---- 1. the span, 8 samples per lane ---------------------------------------------------------------------------
        const long long ub = q.in_off, ue = q.in_off + q.n;
        const int nv = (int)((need + 7) >> 3);
        for (int v = tid; v < nv; v += NT) {
            const long long g = a0 + 8LL * v;
            float f[8];
            if (g >= ub && g + 8 <= ue) {
                const i16x8 s = *reinterpret_cast<const i16x8*>(a.samples + g);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (float)s[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (g + e >= ub && g + e < ue) ? (float)a.samples[g + e] : 0.f;
            }
            f32x4* d = reinterpret_cast<f32x4*>(xs + 8 * v);
            d[0] = f32x4{f[0], f[1], f[2], f[3]};
            d[1] = f32x4{f[4], f[5], f[6], f[7]};
        }
        __syncthreads();

        // ---- 2. a thread forms four outputs of ONE phase: a weight is loaded once for the four -------------------------------
        // The chunk is cut into four quarters of Q outputs, Q a multiple of ou: thread j0 < Q takes the outputs j0 + r Q, r < 4,
        // which share the phase (p0 + j0) mod ou.  Consecutive threads take consecutive outputs (consecutive weights and
        // outputs, inputs iu / ou apart: the LDS reads of a wave are as free of bank conflicts as the ratio allows); thread
        // tid takes j0 = tid, tid + NT, ...
        const int nbq = ((cnt + ou - 1) / ou + OPT - 1) / OPT, Q = nbq * ou, qstep = nbq * iu;
        const int fp0 = first[p0];
        const int db = NT / ou, dp = NT - db * ou;
        int b = (p0 + tid) / ou, p = p0 + tid - b * ou;  // output k0 + j0 is phase p of block b0 + b
        for (int j0 = tid; j0 < Q; j0 += NT) {
            if (j0 < cnt) {
                const int x0 = lead + b * iu + first[p] - fp0;
                int xo[OPT];
                float acc[OPT];
#pragma unroll
                for (int r = 0; r < OPT; ++r) {
                    xo[r] = j0 + r * Q < cnt ? x0 + r * qstep : x0;  // past the end: the first output again, not stored
                    acc[r] = 0.f;
                }
                const float* wt = w + p;
                for (int t = 0; t < taps; t += 4, wt += 4 * (size_t)ou) {  // taps is a multiple of 4
                    float wv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) wv[i] = wt[(size_t)i * ou];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int r = 0; r < OPT; ++r) acc[r] = fmaf(wv[i], xs[xo[r] + t + i], acc[r]);
                }
#pragma unroll
                for (int r = 0; r < OPT; ++r) {
#pragma clang fp contract(off)
                    const int j = j0 + r * Q;
                    if (j < cnt) nclip += store<I16>(a.out, q.out_off + k0 + j, gain * acc[r]);
                }
            }
            b += db;
            p += dp;
            if (p >= ou) { p -= ou; ++b; }
        }
    }
    if (I16) {
        nclip = wave_sum(nclip);
        if ((tid & 63) == 0 && nclip) atomicAdd(a.clipped + u, nclip);  // integers
    }
}

}  // namespace

extern "C" {

int nplda_resample_chunk(void) { return CH; }

size_t nplda_resample_span_floats(int32_t iu, int32_t ou, int32_t taps) {
    if (iu < 1 || ou < 1 || taps < 1 || iu > NPLDA_RESAMPLE_MAX_UNITS || ou > NPLDA_RESAMPLE_MAX_UNITS ||
        taps > NPLDA_RESAMPLE_MAX_TAPS)
        return 0;
    return (size_t)span_floats(iu, ou, taps);
}

int64_t nplda_resample_chunk_table(const int64_t* out_off, int64_t n_utts, int32_t* table, int64_t capacity) {
    long long total = 0, u = 0;
    const int status = ragged_walk(out_off, out_off, n_utts, kMaxUtts, [&](long long m, long long) {
        if (m > INT_MAX - CH) return NPLDA_EUNSUPPORTED;
        long long c[1];
        ChunkTerms()(m, m, c);
        if (table) {
            if (total + c[0] > capacity) return NPLDA_ENOSPC;
            for (long long i = 0; i < c[0]; ++i) {
                table[2 * (total + i)] = (int32_t)u;
                table[2 * (total + i) + 1] = (int32_t)i;
            }
        }
        total += c[0];
        ++u;
        return total > INT_MAX / 2 ? NPLDA_EUNSUPPORTED : NPLDA_OK;
    });
    return status != NPLDA_OK ? (int64_t)status : (int64_t)total;
}

int nplda_resample_batch(const nplda_resample_call* c, nplda_stream_t stream) {
    if (!c || c->n_utts < 0 || c->n_ratios < 0 || c->total_chunks < 0) return NPLDA_EINVAL;
    if (c->n_utts == 0) return NPLDA_OK;
    if (c->n_utts > kMaxUtts || c->n_ratios > kMaxUtts || c->total_chunks > INT_MAX / 2) return NPLDA_EUNSUPPORTED;
    size_t lds = 0;
    if (c->n_ratios > 0) {
        if (c->max_iu < 1 || c->max_ou < 1 || c->max_taps < 1) return NPLDA_EINVAL;
        if (c->max_iu > NPLDA_RESAMPLE_MAX_UNITS || c->max_ou > NPLDA_RESAMPLE_MAX_UNITS || c->max_taps > NPLDA_RESAMPLE_MAX_TAPS)
            return NPLDA_EUNSUPPORTED;
        if (c->max_span < 1) return NPLDA_EINVAL;
        if ((size_t)c->max_span * sizeof(float) > NPLDA_RESAMPLE_MAX_LDS_BYTES) return NPLDA_EUNSUPPORTED;
        lds = (size_t)c->max_span * sizeof(float);
    }
    if (!c->utts || !c->clipped || (c->total_chunks > 0 && (!c->samples || !c->out || !c->chunks)) ||
        (c->n_ratios > 0 && (!c->ratios || !c->first || !c->weights)) || !nplda_aligned16(c->samples))
        return NPLDA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rs_clear_kernel, dim3((unsigned)((c->n_utts + NT - 1) / NT)), dim3(NT), 0, st, c->clipped, (int)c->n_utts);
    int rc = nplda_launch_status();
    if (rc != NPLDA_OK || c->total_chunks == 0) return rc;
    Args a;
    a.samples = c->samples; a.utts = c->utts; a.ratios = c->ratios; a.first = c->first; a.weights = c->weights;
    a.chunks = c->chunks; a.out = c->out; a.clipped = c->clipped;
    a.n_utts = (int)c->n_utts; a.n_ratios = (int)c->n_ratios; a.lds_floats = (int)(lds / sizeof(float));
    if (c->out_i16) hipLaunchKernelGGL(rs_kernel<true>, dim3((unsigned)c->total_chunks), dim3(NT), lds, st, a);
    else hipLaunchKernelGGL(rs_kernel<false>, dim3((unsigned)c->total_chunks), dim3(NT), lds, st, a);
    return nplda_launch_status();
}

}  // extern "C"
