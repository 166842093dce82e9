// nplda_vbhmm.hip — VB-HMM resegmentation of clustered embeddings (VBx), P ragged problems per call (gfx950).
// design/k22_vbhmm.md has the semantics, the phases and the budget.
//
// vbhmm_kernel: ONE workgroup per problem (a recording: T rows in time order, S speaker slots, D features), every iteration
// inside the one launch.  All arithmetic is float64.  An iteration is a chain of block-wide phases over the problem's slice
// of the workspace: speaker counts, the speaker models (gamma^T x, four speakers per thread), the emissions (x alpha^T, a row
// and eight speakers per thread), a row maximum with exp, the forward recursion on wave 0 and the backward recursion on
// wave 1 at the same time (a lane per speaker, normalised per step), the posteriors, and the entry counts for pi.
// __syncthreads() only: no cross-block hand-off, no atomics, no memset, nothing read back; every sum has one fixed order.
#include <cmath>

#include "nplda_ragged.h"

namespace {

constexpr int kVbBlock = 512;  // threads of the workgroup: eight waves, two per SIMD, one block per CU (at most 256 registers)
constexpr int kVbWaves = kVbBlock / 64;
constexpr int kVbMaxS = 64;    // a speaker per lane in the recursions
constexpr int kVbMaxIters = 256;
constexpr int kVbMaxT = 16384;                // nplda_ahc_max_n()
constexpr long long kMaxP = (1ll << 22) - 1;  // as nplda_ahc_f32
constexpr int kSQ = 4;  // speakers per thread in the model phase
constexpr int kTile = 32;  // rows per LDS tile of the model phase (even: the two chains keep their parity)
constexpr int kRec = 16;  // steps of a recursion whose emissions are in registers
constexpr int kSC = 8;  // speakers per thread in the emission phase; alpha^T rows are padded to a multiple of it

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- the layout of a problem's workspace slice, in doubles (host and device agree through this one function) -----------------

struct Slice {
    long long aT, ksd, esd, G, m, c, w, p, f, b, total;
};

__host__ __device__ inline Slice slice_of(long long T, long long S, long long D) {
    const long long Sp = (S + kSC - 1) / kSC * kSC;
    Slice s;
    s.aT = 0;                // [D][Sp] alpha_sd sqrt(psi_d), zero in the pad columns
    s.ksd = s.aT + D * Sp;   // [S][D] (invL_sd + alpha_sd^2) psi_d
    s.esd = s.ksd + S * D;   // [S][D] ln invL_sd - invL_sd + 1 - alpha_sd^2
    s.G = s.esd + S * D;     // [T]
    s.m = s.G + T;           // [T] row maximum of the emissions
    s.c = s.m + T;           // [T] forward normaliser
    s.w = s.c + T;           // [T] 1 / (c_t sum_s f_ts b_ts)
    s.p = s.w + T;           // [T][S] emissions, then exp(emission - m_t)
    s.f = s.p + T * S;       // [T][S] normalised forward variable
    s.b = s.f + T * S;       // [T][S] normalised backward variable
    s.total = (s.b + T * S + 1) & ~1ll;  // slices stay 16-byte aligned
    return s;
}

// what a problem of T rows and S speaker slots takes (csrc/nplda_ragged.h): T S posteriors and its slice of the workspace
enum { kGamma, kWsDoubles, kTerms };
struct VbTerms {
    long long D;
    __host__ __device__ void operator()(long long T, long long S, long long* t) const {
        t[kGamma] = T * S;
        t[kWsDoubles] = slice_of(T, S, D).total;
    }
};

// ---- host: the ragged layout ---------------------------------------------------------------------------------------------------

struct VbPlan {
    int status;
    long long rows, slots, gamma_elems;
    size_t ws_bytes;
};

VbPlan vb_plan(const int64_t* offs, const int64_t* spk, int64_t P, int D2) {
    VbPlan r = {NPLDA_OK, 0, 0, 0, 0};
    if (P < 0 || D2 <= 0 || (P > 0 && (!offs || !spk))) {
        r.status = NPLDA_EINVAL;
        return r;
    }
    if (D2 > NPLDA_MAX_DIM) {  // (after the invalid arguments, before the tables' contents: where the walk has P > kMaxP)
        r.status = NPLDA_EUNSUPPORTED;
        return r;
    }
    long long ws = 0;
    int unsupported = 0;
    r.status = ragged_walk(offs, spk, P, kMaxP, [&](long long T, long long S) {
        if (S == 0 && T > 0) return NPLDA_EINVAL;
        if (T > kVbMaxT || S > kVbMaxS) {
            unsupported = 1;  // (an invalid problem further on still wins)
            return NPLDA_OK;
        }
        long long t[kTerms];
        VbTerms{D2}(T, S, t);
        r.gamma_elems += t[kGamma];
        ws += t[kWsDoubles];
        return NPLDA_OK;
    });
    if (r.status == NPLDA_OK && unsupported) r.status = NPLDA_EUNSUPPORTED;
    if (r.status == NPLDA_OK && P > 0) {
        r.rows = offs[P];
        r.slots = spk[P];
    }
    r.ws_bytes = up256((size_t)ws * 8) + 256;
    return r;
}

// ---- device --------------------------------------------------------------------------------------------------------------------

struct VbArgs {
    const float* z;
    long long ldz;
    const long long *offs, *spk;
    int D;
    const double* psi;
    const int* labels_init;
    const double *gamma_init, *pi_init;
    double Fa, Fb, loop, eps, smooth;
    int max_iters;
    double *gamma, *pi, *elbo;
    int *n_iters, *labels, *n_speakers;
    double* ws;
};

struct VbShared {
    long long red[2 * kVbWaves];
    double sum[2][kVbWaves];
    double psi[NPLDA_MAX_DIM], sqpsi[NPLDA_MAX_DIM];
    double pi[kVbMaxS], pinew[kVbMaxS], N[kVbMaxS], K[kVbMaxS], E[kVbMaxS];
    int owns[kVbMaxS];
    float xs[kTile * NPLDA_MAX_DIM];  // a tile of rows for the model phase
    double gs[kTile * kVbMaxS];       // and its posteriors
};

__device__ __forceinline__ long long uniform(long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the sum of v over the block, the same bits on every thread: lanes by butterfly, then the waves in order.  ONE barrier:
// consecutive calls alternate between two sets of slots, so the slots a call writes were last read two calls ago.
__device__ __forceinline__ double block_sum(VbShared& sh, int& slot, double v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh.sum[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh.sum[slot][0];
#pragma unroll
    for (int w = 1; w < kVbWaves; ++w) t += sh.sum[slot][w];
    slot ^= 1;
    return t;
}

__global__ __launch_bounds__(kVbBlock) void vbhmm_kernel(const VbArgs a) {
    __shared__ VbShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long prob = blockIdx.x;
    const int D = a.D;

    // where this problem's rows, speaker slots, posteriors and workspace slice start: integer sums over the problems before it
    // (two tables and this kernel's eight slots per term: nplda_ragged.h's ragged_starts takes one table and sixteen)
    long long ge = 0, we = 0;
    for (long long q = tid; q < prob; q += kVbBlock) {
        long long t[kTerms];
        VbTerms{D}(a.offs[q + 1] - a.offs[q], a.spk[q + 1] - a.spk[q], t);
        ge += t[kGamma];
        we += t[kWsDoubles];
    }
    ge = wave_sum(ge);
    we = wave_sum(we);
    if (lane == 0) {
        sh.red[wave] = ge;
        sh.red[kVbWaves + wave] = we;
    }
    __syncthreads();
    ge = we = 0;
#pragma unroll
    for (int w = 0; w < kVbWaves; ++w) {
        ge += sh.red[w];
        we += sh.red[kVbWaves + w];
    }
    ge = uniform(ge);  // (the same on every thread: in scalar registers, with every pointer formed from them)
    we = uniform(we);
    const long long row0 = uniform(a.offs[prob]), s0 = uniform(a.spk[prob]);
    const int T = __builtin_amdgcn_readfirstlane((int)(a.offs[prob + 1] - row0));
    const int S = __builtin_amdgcn_readfirstlane((int)(a.spk[prob + 1] - s0));
    const int max_iters = a.max_iters;
    double* elbo = a.elbo + prob * max_iters;
    if (T == 0) {  // block-uniform
        for (int i = tid; i < max_iters; i += kVbBlock) elbo[i] = __builtin_nan("");
        if (tid == 0) {
            a.n_iters[prob] = 0;
            a.n_speakers[prob] = 0;
        }
        return;
    }
    const int Sp = (S + kSC - 1) / kSC * kSC;
    int S2 = 1;
    while (S2 < S) S2 <<= 1;  // (at most six steps)
    const float* z = a.z + row0 * a.ldz;
    const long long ldz = a.ldz;
    double* gamma = a.gamma + ge;
    const Slice L = slice_of(T, S, D);
    double* ws = a.ws + we;
    double *aT = ws + L.aT, *ksd = ws + L.ksd, *esd = ws + L.esd, *G = ws + L.G, *mt = ws + L.m, *ct = ws + L.c, *wt = ws + L.w;
    double *pe = ws + L.p, *fw = ws + L.f, *bw = ws + L.b;
    const double Fa = a.Fa, Fb = a.Fb, r = a.Fa / a.Fb, loop = a.loop, enter = 1.0 - a.loop;

    // ---- the constants of the call: G_t, the initial posteriors and pi, zeros in the pad columns of alpha^T
    for (int d = tid; d < D; d += kVbBlock) {
        const double v = a.psi[d];
        sh.psi[d] = v;
        sh.sqpsi[d] = sqrt(v);
    }
    // G_t = -(sum_d x_td^2 + D ln 2 pi) / 2 enters every emission of row t and so the ELBO T times over: the squares of
    // float32 values are exact in float64, their sum is compensated (TwoSum), and D ln 2 pi carries its low part
    for (int t = tid; t < T; t += kVbBlock) {
        const float* x = z + (long long)t * ldz;
        double q = 0.0, comp = 0.0;
        for (int d = 0; d < D; ++d) {
            const double v = (double)x[d] * (double)x[d];
            const double u = q + v, bp = u - q;
            comp += (q - (u - bp)) + (v - bp);
            q = u;
        }
        const double ln2pi_hi = 0x1.d67f1c864beb5p+0, ln2pi_lo = -0x1.65b5a1b7ff5dfp-54;
        const double c_hi = (double)D * ln2pi_hi, c_lo = fma((double)D, ln2pi_hi, -c_hi) + (double)D * ln2pi_lo;
        const double u = q + c_hi, bp = u - q;
        comp += (q - (u - bp)) + (c_hi - bp) + c_lo;
        G[t] = -0.5 * (u + comp);
    }
    if (a.gamma_init) {
        const double* gi = a.gamma_init + ge;
        for (long long i = tid; i < (long long)T * S; i += kVbBlock) gamma[i] = gi[i];
    } else {
        const int* lab = a.labels_init + row0;
        const double e = exp(-a.smooth), den = 1.0 + (double)(S - 1) * e, hi = 1.0 / den, lo = e / den, uni = 1.0 / (double)S;
        for (long long i = tid; i < (long long)T * S; i += kVbBlock) {
            const int t = (int)(i / S), s = (int)(i - (long long)t * S), l = lab[t];
            gamma[i] = (l < 0 || l >= S) ? uni : (l == s ? hi : lo);
        }
    }
    if (tid < S) sh.pi[tid] = a.pi_init ? a.pi_init[s0 + tid] : 1.0 / (double)S;
    for (int i = tid; i < D * Sp; i += kVbBlock) aT[i] = 0.0;

    int slot = 0, done = 0;
    double prev = 0.0;
    const int nquad = (S + kSQ - 1) / kSQ, nchunk = Sp / kSC;
    for (int it = 0; it < max_iters; ++it) {  // (`done`, `prev` and the stop are block-uniform)
        __syncthreads();  // gamma and pi of the last iteration (or the initial ones) are in place

        // ---- N_s = sum_t gamma_ts: a wave per speaker, a lane per residue of t
        for (int s = wave; s < S; s += kVbWaves) {
            double n0 = 0.0;
            for (int t = lane; t < T; t += 64) n0 += gamma[(long long)t * S + s];
            n0 = wave_sum(n0);
            if (lane == 0) sh.N[s] = n0;
        }
        __syncthreads();

        // ---- the speaker models: a thread per (four speakers, d); sums over t on two chains each (even and odd t).  The
        // rows come through LDS, kTile at a time, fetched by the whole block: a thread that read gamma and x from memory
        // row by row spent the phase waiting for the L2, one round trip per pair of rows.
        for (int item0 = 0; item0 < nquad * D; item0 += kVbBlock) {  // (block-uniform, as is the tile loop: barriers inside)
            const int item = item0 + tid;
            const bool active = item < nquad * D;
            const int sq = active ? item / D : 0, d = active ? item - sq * D : 0;
            int si[kSQ];
#pragma unroll
            for (int k = 0; k < kSQ; ++k) si[k] = kSQ * sq + k < S ? kSQ * sq + k : S - 1;  // (clamped: read, not stored)
            double acc0[kSQ] = {0.0, 0.0, 0.0, 0.0}, acc1[kSQ] = {0.0, 0.0, 0.0, 0.0};
            for (int t0 = 0; t0 < T; t0 += kTile) {
                const int rows = T - t0 < kTile ? T - t0 : kTile;
                __syncthreads();  // the last tile has been used
                for (int i = tid; i < rows * D; i += kVbBlock) {
                    const int rr = i / D, dd = i - rr * D;
                    sh.xs[rr * NPLDA_MAX_DIM + dd] = z[(long long)(t0 + rr) * ldz + dd];
                }
                for (int i = tid; i < rows * S; i += kVbBlock) {
                    const int rr = i / S, ss = i - rr * S;
                    sh.gs[rr * kVbMaxS + ss] = gamma[(long long)t0 * S + i];
                }
                __syncthreads();
                if (active) {
                    int rr = 0;
                    for (; rr + 1 < rows; rr += 2) {
                        const double x0 = (double)sh.xs[rr * NPLDA_MAX_DIM + d], x1 = (double)sh.xs[(rr + 1) * NPLDA_MAX_DIM + d];
#pragma unroll
                        for (int k = 0; k < kSQ; ++k) {
                            acc0[k] = fma(sh.gs[rr * kVbMaxS + si[k]], x0, acc0[k]);
                            acc1[k] = fma(sh.gs[(rr + 1) * kVbMaxS + si[k]], x1, acc1[k]);
                        }
                    }
                    if (rr < rows) {  // (the last row of an odd T: an even t)
                        const double x0 = (double)sh.xs[rr * NPLDA_MAX_DIM + d];
#pragma unroll
                        for (int k = 0; k < kSQ; ++k) acc0[k] = fma(sh.gs[rr * kVbMaxS + si[k]], x0, acc0[k]);
                    }
                }
            }
            if (!active) continue;
            const double psd = sh.psi[d], sqd = sh.sqpsi[d];
#pragma unroll
            for (int k = 0; k < kSQ; ++k) {
                const int s = kSQ * sq + k;
                if (s < S) {
                    // with u = (Fa / Fb) N_s psi_d: ln invL - invL + 1 = u / (1 + u) - log1p(u), two terms of the size of u
                    // that leave u^2 / 2, where ln invL, invL and 1 are three of the size of 1
                    const double u = r * sh.N[s] * psd, invL = 1.0 / (1.0 + u);
                    const double al = r * invL * ((acc0[k] + acc1[k]) * sqd);
                    aT[(long long)d * Sp + s] = al * sqd;
                    ksd[(long long)s * D + d] = (invL + al * al) * psd;
                    esd[(long long)s * D + d] = (u * invL - log1p(u)) - al * al;
                }
            }
        }
        __syncthreads();

        // ---- K_s = 1/2 sum_d (invL + alpha^2) psi, E_s = sum_d (ln invL - invL - alpha^2 + 1): a wave per speaker
        for (int s = wave; s < S; s += kVbWaves) {
            double k0 = 0.0, e0 = 0.0;
            for (int d = lane; d < D; d += 64) {
                k0 += ksd[(long long)s * D + d];
                e0 += esd[(long long)s * D + d];
            }
            k0 = wave_sum(k0);
            e0 = wave_sum(e0);
            if (lane == 0) {
                sh.K[s] = 0.5 * k0;
                sh.E[s] = e0;
            }
        }
        __syncthreads();

        // ---- the emissions: a thread per (row t, eight speakers); the row is read two features at a time
        for (int item = tid; item < nchunk * T; item += kVbBlock) {
            const int ch = item / T, t = item - ch * T;
            const float* x = z + (long long)t * ldz;
            const double* ac = aT + kSC * ch;
            double acc[kSC];
#pragma unroll
            for (int k = 0; k < kSC; ++k) acc[k] = 0.0;
            int d = 0;
            for (; d + 1 < D; d += 2) {
                const f32x2 xv = *(const f32x2*)(x + d);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const double xu = (double)xv[u];
                    const f64x2* av = (const f64x2*)(ac + (long long)(d + u) * Sp);
#pragma unroll
                    for (int k = 0; k < kSC / 2; ++k) {
                        const f64x2 v = av[k];
                        acc[2 * k] = fma(xu, v[0], acc[2 * k]);
                        acc[2 * k + 1] = fma(xu, v[1], acc[2 * k + 1]);
                    }
                }
            }
            for (; d < D; ++d) {  // (the pad columns D .. ldz are never read)
                const double xu = (double)x[d];
                const f64x2* av = (const f64x2*)(ac + (long long)d * Sp);
#pragma unroll
                for (int k = 0; k < kSC / 2; ++k) {
                    const f64x2 v = av[k];
                    acc[2 * k] = fma(xu, v[0], acc[2 * k]);
                    acc[2 * k + 1] = fma(xu, v[1], acc[2 * k + 1]);
                }
            }
            const double g = G[t];
#pragma unroll
            for (int k = 0; k < kSC; ++k) {
                const int s = kSC * ch + k;
                if (s < S) pe[(long long)t * S + s] = Fa * ((acc[k] - sh.K[s]) + g);
            }
        }
        __syncthreads();

        // ---- m_t over the speakers that can be entered (pi_s > 0) and p_ts = exp(l_ts - m_t), 0 for the dead ones
        for (int t = tid; t < T; t += kVbBlock) {
            double* row = pe + (long long)t * S;
            double m = -__builtin_inf();
            for (int s = 0; s < S; ++s)
                if (sh.pi[s] > 0.0 && row[s] > m) m = row[s];
            for (int s = 0; s < S; ++s) row[s] = sh.pi[s] > 0.0 ? exp(row[s] - m) : 0.0;
            mt[t] = m;
        }
        __syncthreads();

        // ---- the recursions: forward on wave 0, backward on wave 1, a lane per speaker, normalised at every step
        // A step waits for nothing but its own arithmetic: the emissions of the next kRec steps are fetched while the
        // current kRec run from registers (one step of look-ahead left each step waiting for a load from the L2).
        if (wave == 0) {
            const bool on = lane < S;
            const double pis = on ? sh.pi[lane] : 0.0, ent = enter * pis;
            const double* pcol = pe + lane;
            double f = 0.0, pb[kRec], pnx[kRec];
#pragma unroll
            for (int k = 0; k < kRec; ++k) pb[k] = (on && k < T) ? pcol[(long long)k * S] : 0.0;
            for (int t0 = 0; t0 < T; t0 += kRec) {
#pragma unroll
                for (int k = 0; k < kRec; ++k) {
                    const int tn = t0 + kRec + k;
                    pnx[k] = (on && tn < T) ? pcol[(long long)tn * S] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < kRec; ++k) {
                    const int t = t0 + k;
                    if (t < T) {  // (wave-uniform)
                        const double av = (t == 0 ? pis : fma(loop, f, ent)) * pb[k];
                        const double c = wave_sum(av, S2);
                        f = av / c;
                        if (on) fw[(long long)t * S + lane] = f;
                        if (lane == 0) ct[t] = c;
                    }
                }
#pragma unroll
                for (int k = 0; k < kRec; ++k) pb[k] = pnx[k];
            }
        } else if (wave == 1) {
            const bool on = lane < S;
            const double pis = on ? sh.pi[lane] : 0.0;
            const double* pcol = pe + lane;
            double b = 1.0, pb[kRec], pnx[kRec];
            if (on) bw[(long long)(T - 1) * S + lane] = b;
            const int steps = T - 1;  // step j forms row T - 2 - j from row T - 1 - j
#pragma unroll
            for (int k = 0; k < kRec; ++k) pb[k] = (on && k < steps) ? pcol[(long long)(T - 1 - k) * S] : 0.0;
            for (int j0 = 0; j0 < steps; j0 += kRec) {
#pragma unroll
                for (int k = 0; k < kRec; ++k) {
                    const int jn = j0 + kRec + k;
                    pnx[k] = (on && jn < steps) ? pcol[(long long)(T - 1 - jn) * S] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < kRec; ++k) {
                    const int j = j0 + k;
                    if (j < steps) {  // (wave-uniform)
                        const double q = pb[k] * b;  // (0 on the lanes without a speaker)
                        const double u = wave_sum(pis * q, S2), v = wave_sum(q, S2);
                        b = fma(loop, q, enter * u) / fma(loop, v, (double)S * enter * u);
                        if (on) bw[(long long)(T - 2 - j) * S + lane] = b;
                    }
                }
#pragma unroll
                for (int k = 0; k < kRec; ++k) pb[k] = pnx[k];
            }
        }
        __syncthreads();

        // ---- the posteriors, and L = sum_t (ln c_t + m_t)
        double lc = 0.0;
        for (int t = tid; t < T; t += kVbBlock) {
            const double *fr = fw + (long long)t * S, *br = bw + (long long)t * S;
            double* gr = gamma + (long long)t * S;
            double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;  // (four chains: its rounding is common to the row's posteriors)
            int s4 = 0;
            for (; s4 + 3 < S; s4 += 4) {
                g0 = fma(fr[s4], br[s4], g0);
                g1 = fma(fr[s4 + 1], br[s4 + 1], g1);
                g2 = fma(fr[s4 + 2], br[s4 + 2], g2);
                g3 = fma(fr[s4 + 3], br[s4 + 3], g3);
            }
            for (; s4 < S; ++s4) g0 = fma(fr[s4], br[s4], g0);
            const double g = (g0 + g1) + (g2 + g3);
            for (int s = 0; s < S; ++s) gr[s] = fr[s] * br[s] / g;
            const double c = ct[t];
            wt[t] = 1.0 / (c * g);
            lc += log(c) + mt[t];
        }
        const double Lev = block_sum(sh, slot, lc);  // (its barrier also ends the pass above)

        // ---- pi_s <- gamma_0s + (1 - loop) pi_s sum_{t >= 1} p_ts b_ts / (c_t g_t): a wave per speaker
        for (int s = wave; s < S; s += kVbWaves) {
            double e0 = 0.0;
            for (int t = 1 + lane; t < T; t += 64) e0 = fma(pe[(long long)t * S + s] * bw[(long long)t * S + s], wt[t], e0);
            e0 = wave_sum(e0);
            if (lane == 0) sh.pinew[s] = gamma[s] + enter * sh.pi[s] * e0;
        }
        __syncthreads();
        // (every wave: the same butterfly over the same LDS words, so the same bits on every thread; a tree, because the
        // rounding of `tot` is an error common to every pi_s)
        const double tot = wave_sum(lane < S ? sh.pinew[lane] : 0.0), esum = wave_sum(lane < S ? sh.E[lane] : 0.0);
        const double el = Lev + 0.5 * Fb * esum;
        __syncthreads();  // everyone has read pinew and E; pi may change
        if (tid < S) sh.pi[tid] = sh.pinew[tid] / tot;
        if (tid == 0) elbo[it] = el;
        done = it + 1;
        if (it >= 1 && el - prev < a.eps) break;  // block-uniform: every thread formed `el` from the same LDS words
        prev = el;
    }
    __syncthreads();

    // ---- the outputs of the last iteration executed
    for (int i = done + tid; i < max_iters; i += kVbBlock) elbo[i] = __builtin_nan("");
    if (tid < S) {
        a.pi[s0 + tid] = sh.pi[tid];
        sh.owns[tid] = 0;
    }
    __syncthreads();
    int* labels = a.labels + row0;
    for (int t0 = 0; t0 < T; t0 += kVbBlock) {  // argmax with the lowest s among equal values
        const int t = t0 + tid;
        if (t < T) {
            const double* gr = gamma + (long long)t * S;
            int best = 0;
            double bv = gr[0];
            for (int s = 1; s < S; ++s)
                if (gr[s] > bv) {
                    bv = gr[s];
                    best = s;
                }
            labels[t] = best;
            sh.owns[best] = 1;  // (every writer stores the same word)
        }
    }
    __syncthreads();
    if (wave == 0) {  // the dense rank of the speakers that own a row
        const bool own = lane < S && sh.owns[lane] != 0;
        const unsigned long long bal = __ballot(own);
        sh.owns[lane] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) {
            a.n_iters[prob] = done;
            a.n_speakers[prob] = __popcll(bal);
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += kVbBlock) labels[t] = sh.owns[labels[t]];
}

}  // namespace

extern "C" {

int nplda_vbhmm_max_speakers(void) { return kVbMaxS; }
int nplda_vbhmm_max_iters(void) { return kVbMaxIters; }
int nplda_vbhmm_block(void) { return kVbBlock; }

size_t nplda_vbhmm_workspace_bytes(const int64_t* offsets_host, const int64_t* spk_offsets_host, int64_t P, int D2) {
    const VbPlan r = vb_plan(offsets_host, spk_offsets_host, P, D2);
    return r.status == NPLDA_OK ? r.ws_bytes : 0;
}

int nplda_vbhmm_f64(const float* z, int64_t ldz, const int64_t* offsets_host, const int64_t* offsets, const int64_t* spk_offsets_host,
                    const int64_t* spk_offsets, int64_t P, int D2, const double* psi, const int32_t* labels_init,
                    const double* gamma_init, const double* pi_init, double Fa, double Fb, double loop_prob, double epsilon,
                    double init_smoothing, int max_iters, double* gamma, double* pi, double* elbo, int32_t* n_iters, int32_t* labels,
                    int32_t* n_speakers, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    if (std::isnan(epsilon) || !(Fa > 0.0) || !(Fb > 0.0) || !std::isfinite(Fa) || !std::isfinite(Fb)) return NPLDA_EINVAL;
    if (!(loop_prob >= 0.0 && loop_prob < 1.0) || !(init_smoothing >= 0.0) || max_iters < 1) return NPLDA_EINVAL;
    const VbPlan r = vb_plan(offsets_host, spk_offsets_host, P, D2);
    if (r.status != NPLDA_OK) return r.status;
    if (max_iters > kVbMaxIters) return NPLDA_EUNSUPPORTED;
    if (P == 0) return NPLDA_OK;
    if ((labels_init != nullptr) == (gamma_init != nullptr)) return NPLDA_EINVAL;
    if (!offsets || !spk_offsets || !elbo || !n_iters || !n_speakers) return NPLDA_EINVAL;
    auto a8 = [](const void* p) { return (((uintptr_t)p) & 7u) == 0; };
    auto a4 = [](const void* p) { return (((uintptr_t)p) & 3u) == 0; };
    if (!a8(offsets) || !a8(spk_offsets) || !a8(elbo) || !a4(n_iters) || !a4(n_speakers)) return NPLDA_EINVAL;
    if (r.rows > 0) {
        if (!z || !psi || !gamma || !pi || !labels || !ws) return NPLDA_EINVAL;
        if (ldz < D2 || (ldz & 3) || !nplda_aligned16(z) || !nplda_aligned16(ws)) return NPLDA_EINVAL;
        if (!a8(psi) || !a8(gamma) || !a8(pi) || !a4(labels) || !a8(gamma_init) || !a8(pi_init) || !a4(labels_init))
            return NPLDA_EINVAL;
        if (ws_bytes < r.ws_bytes) return NPLDA_ENOSPC;
    }
    VbArgs a = {z, (long long)ldz, (const long long*)offsets, (const long long*)spk_offsets, D2, psi, (const int*)labels_init,
                gamma_init, pi_init, Fa, Fb, loop_prob, epsilon, init_smoothing, max_iters, gamma, pi, elbo,
                (int*)n_iters, (int*)labels, (int*)n_speakers, (double*)ws};
    hipLaunchKernelGGL(vbhmm_kernel, dim3((unsigned)P), dim3(kVbBlock), 0, (hipStream_t)stream, a);
    return nplda_launch_status();
}

}  // extern "C"
