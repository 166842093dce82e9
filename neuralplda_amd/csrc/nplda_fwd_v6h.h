// nplda_fwd_v6h.h — nplda_fwd_v6.h (L2S = 1) with a HYBRID layer 1: the last S1 of the NB feature blocks run in split form
// (three bf16 pieces per fp32 operand, six v_mfma_f32_16x16x32_bf16 passes, nplda_fwd_bf16x3.h), the other NB - S1 stay on
// fp32-input 16 x 16 x 4 MFMAs.
//
// Why a few blocks and not all: v6 is bound by the matrix pipe and layer 1 is nine tenths of its matrix time, but the
// headline line is priced against the fp32-input MFMA peak — a whole-layer split form runs past that peak and its roofline
// fraction reads above 1 (design/k01_forward_streaming.md, "Hybrid layer 1").  Per k32-step a feature block costs
// 2 x 8 x 32 = 512 matrix cycles in fp32 form and 12 x 16 = 192 in split form, both sides together; splitting x and y
// (two split3x8 per wave and k32-step, ~44 VALU instructions) is paid once however many blocks use the pieces.
//
// The split set always holds the tail block NB - 1 (the six left-over features of D = 150): as a split block it is an
// ordinary padded 16-feature block again — its rows are zero in the image and in b1 — so v6's 4 x 4 x 1 quads, their
// k-group sums and the re-layout into an accumulator block are gone.
//
// One layer-1 chunk is two k16-steps = one k32-step (KS1 must be even: the dispatch sends other layouts to v6):
//  * the x loads are v6's.  The fp32 image's fragments W1p[2 c][nb][lane] and W1p[2 c + 1][nb][lane] are the eight A values
//    of one 16 x 16 x 32 lane (k = 32 c + 4 g + e for e < 4, 32 c + 16 + 4 g + e - 4 above) and xc[0], xc[1] the matching B
//    values — the argument nplda_fwd_v6.h makes for W2p in layer 2;
//  * the block splits the W1 pieces of the S1 blocks ONCE per chunk (no derived image in the packed buffer, which training
//    rewrites in place): unit u (block NB - S1 + u, 64 lanes x 8 values) of chunk c + 1 belongs to wave (S1 (c + 1) + u) mod
//    WAVES — the owner rotates with the chunk, so the ~22 extra VALU instructions do not sit on the same waves every chunk
//    (the fence waits for the slowest).  The owner loads the unit into registers during chunk c - 1, and at the head of
//    chunk c — the fence has drained every load — splits it and stores the pieces into the LDS piece buffer
//    [u][piece][lane] of the other parity; the chunk fence publishes them;
//  * the LDS-DMA of a chunk skips the split blocks' segments (the LDS layout keeps the image's stride).
// Normalise, layer 2 and the epilogue are v6's; the last layer-2 step also prepares chunk 0's W1 pieces of the next tile.
#pragma once
#include "nplda_fwd_kernel.h"
#include "nplda_fwd_bf16x3.h"

namespace nplda {

// six-pass product accumulate (small terms first, the order of mfma6x4) for N feature blocks x two row groups: 2 N
// independent accumulator chains, interleaved
template <int N>
__device__ __forceinline__ void mfma6_blocks(const WFrag (&w)[N], const bf16x8 ah, const bf16x8 am, const bf16x8 al,
                                             const bf16x8 bh, const bf16x8 bm, const bf16x8 bl, f32x4* accA, f32x4* accB) {
#define NPLDA_PASS(P, XA, XB)                                  \
    _Pragma("unroll") for (int u = 0; u < N; ++u) {            \
        accA[u] = NPLDA_MFMA_BF16(w[u].P, XA, accA[u]);        \
        accB[u] = NPLDA_MFMA_BF16(w[u].P, XB, accB[u]);        \
    }
    NPLDA_PASS(m, am, bm)
    NPLDA_PASS(h, al, bl)
    NPLDA_PASS(l, ah, bh)
    NPLDA_PASS(h, am, bm)
    NPLDA_PASS(m, ah, bh)
    NPLDA_PASS(h, ah, bh)
#undef NPLDA_PASS
}

template <int NB, int WAVES, int S1, int G1, int XM = 0>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void nplda_fwd_v6h_kernel(const FwdArgs a, int ntiles) {
    constexpr int KPB = 2;                           // one chunk = one k32-step
    constexpr int NF = NB - S1;                      // feature blocks on fp32-input MFMAs: [0, NF); split form: [NF, NB)
    constexpr int STEP4 = NB * 64;                   // float4 per k16-step of weights (the image's stride: all NB blocks)
    constexpr int CH1 = STEP4 * KPB;                 // layer-1 chunk
    constexpr int NSEG1 = NF * KPB;                  // its live segments
    constexpr int NGR = (NF + G1 - 1) / G1;          // MFMA groups of a k16-step
    constexpr int KC2 = NB / 2;                      // k32-steps of layer 2
    constexpr int SG = S1 % 2 ? 3 : 2;               // split blocks per mfma6_blocks call: pairs, an odd count starts with three
    static_assert(S1 >= 1 && S1 <= WAVES && S1 < NB && (S1 % 2 == 0 || S1 >= 3), "one W1 unit per wave at the most");
    static_assert((WAVES & (WAVES - 1)) == 0, "the owner of a W1 unit is computed mod WAVES");
    static_assert(NB % 2 == 0 && WAVES <= NB && NB <= 2 * WAVES, "split layer 2: k32-steps of two whole accumulator blocks, one "
                                                                 "or two W2 units per wave");
    __shared__ f32x4 wbuf[2][CH1];
    __shared__ bf16x8 wsp1[2][S1 * 3 * 64];          // W1 pieces of one chunk, [u][piece][lane]
    __shared__ bf16x8 wsp[2][NB * 3 * 64];           // W2 pieces of one k32-step, [nb][piece][lane]
    __shared__ f32x4 cvec[4][NB * 4];
    __shared__ f32x4 sink[64];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15;
    const int g = lane >> 4;

    const f32x4* Wall = reinterpret_cast<const f32x4*>(a.packed);
    const long long w2base4 = (long long)(a.oW2 / 4);
    for (int i = tid; i < 4 * NB * 4; i += WAVES * 64) {
        const int v = i / (NB * 4), e = i % (NB * 4);
        const size_t o = v == 0 ? a.ob1 : (v == 1 ? a.ob2 : (v == 2 ? a.oQ : a.oP));
        cvec[v][e] = reinterpret_cast<const f32x4*>(a.packed + o)[e];
    }
    const f32x4* b1p = cvec[0];
    const f32x4* b2p = cvec[1];
    const f32x4* Qp = cvec[2];
    const f32x4* Pp = cvec[3];
    const int D0 = a.D0;
    const int NC1 = a.KS1 / KPB;  // (KS1 is even)

    auto seg_dma = [&](const f32x4* src, f32x4* dst) {  // see nplda_fwd_v5.h
        unsigned lo = (unsigned)lane * 16u;
        asm volatile("" : "+v"(lo));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(src) + lo),
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    };
    // the NF fp32 blocks of both k16-steps of chunk c, at their offsets in the image
    auto dma_l1 = [&](int c, f32x4* dst) {
        const f32x4* src = Wall + (long long)c * CH1;
#pragma unroll
        for (int i = 0; i < (NSEG1 + WAVES - 1) / WAVES; ++i) {
            const int sgm = wave + WAVES * i;
            const bool live = sgm < NSEG1;
            const int sg = live ? sgm : 0;
            const int off = (sg / NF) * STEP4 + (sg % NF) * 64;
            seg_dma(src + off, live ? dst + off : sink);
        }
    };
    auto chunk_fence = [&]() {
        __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    // W1 unit of chunk cn that this wave owns (if any): loaded unconditionally (a wave without a unit re-reads unit 0), split
    // and stored under a scalar branch.  A wave-uniform base and an opaque 32-bit lane offset: see w2_load
    f32x4 w1lo, w1hi;
    auto w1_unit = [&](int cn) { return (wave - cn * S1) & (WAVES - 1); };
    auto w1_load = [&](int cn) {
        const int u = w1_unit(cn);
        const char* base = reinterpret_cast<const char*>(Wall + (long long)(2 * cn) * STEP4 + (NF + (u < S1 ? u : 0)) * 64);
        unsigned lo = (unsigned)lane * 16u;
        asm volatile("" : "+v"(lo));
        w1lo = *reinterpret_cast<const f32x4*>(base + lo);
        w1hi = *reinterpret_cast<const f32x4*>(base + STEP4 * 16 + lo);
    };
    auto w1_store = [&](int cn, bf16x8* dst) {
        const int u = w1_unit(cn);
        if (u < S1) {
            bf16x8 h, m, l;
            split3x8(w1lo, w1hi, h, m, l);
            dst[(u * 3 + 0) * 64 + lane] = h;
            dst[(u * 3 + 1) * 64 + lane] = m;
            dst[(u * 3 + 2) * 64 + lane] = l;
        }
    };
    // W2 units of k32-step c: as in nplda_fwd_v6.h
    f32x4 w2lo[2], w2hi[2];
    const bool two = wave + WAVES < NB;
    auto w2_load = [&](int c, int i, int r) {
        const int nb = wave + WAVES * i;
        const char* base = reinterpret_cast<const char*>(Wall + w2base4 + (long long)(2 * c) * STEP4 + (nb < NB ? nb : 0) * 64);
        unsigned lo = (unsigned)lane * 16u;
        asm volatile("" : "+v"(lo));
        w2lo[r] = *reinterpret_cast<const f32x4*>(base + lo);
        w2hi[r] = *reinterpret_cast<const f32x4*>(base + STEP4 * 16 + lo);
    };
    auto w2_store = [&](int i, int r, bf16x8* dst) {
        const int nb = wave + WAVES * i;
        bf16x8 h, m, l;
        split3x8(w2lo[r], w2hi[r], h, m, l);
        dst[(nb * 3 + 0) * 64 + lane] = h;
        dst[(nb * 3 + 1) * 64 + lane] = m;
        dst[(nb * 3 + 2) * 64 + lane] = l;
    };

    auto tile_ptrs = [&](long long t, long long& t0, bool& ok, const float*& pa, const float*& pb) {
        t0 = (t * WAVES + wave) * 16;
        long long r = t0 + j;
        ok = r < a.n;
        if (!ok) r = a.n - 1;
        pa = x_row<XM>(a.xa, r, a.ldx);
        pb = x_row<XM>(a.xb, r, a.ldx);
    };
    long long tile = blockIdx.x;
    long long t0;
    bool ok;
    const float *sa, *sb;
    tile_ptrs(tile, t0, ok, sa, sb);

    const int cn1 = NC1 > 1 ? 1 : 0;  // the chunk whose unit rides into chunk 0 in registers (one chunk: re-read, never stored)
    dma_l1(0, wbuf[0]);
    w1_load(0);
    f32x4 xa[KPB], xb[KPB];
#pragma unroll
    for (int s = 0; s < KPB; ++s) {
        xa[s] = load_xrow<XM>(sa, 16 * s + 4 * g, D0);
        xb[s] = load_xrow<XM>(sb, 16 * s + 4 * g, D0);
    }
    w1_store(0, wsp1[0]);
    w1_load(cn1);
    __syncthreads();  // cvec
    chunk_fence();
    int par = 0;

    for (;;) {
        const long long tile_n = tile + gridDim.x;

        f32x4 accA[NB], accB[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            accA[nb] = b1p[4 * nb + g];
            accB[nb] = accA[nb];
        }

        // ---- layer 1 ---------------------------------------------------------------------------------------
        // one chunk: the MFMAs read (xc, yc) while (xn, yn) receive the next chunk's rows (two register sets, as in v6)
        auto chunk = [&](int c, f32x4 (&xc)[KPB], f32x4 (&yc)[KPB], f32x4 (&xn)[KPB], f32x4 (&yn)[KPB]) {
            const bool more = (c + 1 < NC1);
            // the unit of chunk c + 1 arrived in registers a chunk ago: split and stored FIRST, while no vector-memory
            // operation is in flight (behind the x loads hipcc puts s_waitcnt vmcnt(0) in front of this branch's stores: the
            // owner then waits out the HBM latency of the rows it has just asked for, in the middle of the chunk)
            if (more) {
                w1_store(c + 1, wsp1[par ^ 1]);
                dma_l1(c + 1, wbuf[par ^ 1]);
                if (c + 2 < NC1) w1_load(c + 2);
            } else {
                w2_load(0, 0, 0);
                w2_load(0, 1, 1);
            }
#pragma unroll
            for (int s = 0; s < KPB; ++s) {
                const int ks = more ? KPB * (c + 1) + s : KPB * c + s;  // (after the last chunk: a harmless re-read, see v5)
                xn[s] = load_xrow<XM>(sa, 16 * ks + 4 * g, D0);
                yn[s] = load_xrow<XM>(sb, 16 * ks + 4 * g, D0);
            }
            // (the rows are asked for HERE: with the splits' VALU work in the chunk hipcc otherwise sinks these loads, which
            // nothing in the chunk uses, to its end — in front of the fence's vmcnt(0), the whole HBM latency exposed)
            __builtin_amdgcn_sched_barrier(0);
            const f32x4* w = wbuf[par];
            const bf16x8* wp = wsp1[par];
            bf16x8 ah, am, al, bh, bm, bl;
            split3x8(xc[0], xc[1], ah, am, al);
            split3x8(yc[0], yc[1], bh, bm, bl);
            auto fp32_step = [&](int s) {
#pragma unroll
                for (int gr = 0; gr < NGR; ++gr) {
                    const int nb0 = gr * G1;
                    f32x4 av[G1];
#pragma unroll
                    for (int u = 0; u < G1; ++u)
                        if (nb0 + u < NF) av[u] = w[s * STEP4 + (nb0 + u) * 64 + lane];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
#pragma unroll
                        for (int u = 0; u < G1; ++u) {
                            if (nb0 + u < NF) {
                                accA[nb0 + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][r], xc[s][r], accA[nb0 + u], 0, 0, 0);
                                accB[nb0 + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][r], yc[s][r], accB[nb0 + u], 0, 0, 0);
                            }
                        }
                    }
                }
            };
            fp32_step(0);
            // the split blocks: the first SG of them together, pairs after that
            {
                WFrag wf[SG];
#pragma unroll
                for (int u = 0; u < SG; ++u) {
                    wf[u].h = wp[(u * 3 + 0) * 64 + lane];
                    wf[u].m = wp[(u * 3 + 1) * 64 + lane];
                    wf[u].l = wp[(u * 3 + 2) * 64 + lane];
                }
                mfma6_blocks<SG>(wf, ah, am, al, bh, bm, bl, &accA[NF], &accB[NF]);
            }
#pragma unroll
            for (int u0 = SG; u0 < S1; u0 += 2) {
                WFrag wf[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    wf[u].h = wp[((u0 + u) * 3 + 0) * 64 + lane];
                    wf[u].m = wp[((u0 + u) * 3 + 1) * 64 + lane];
                    wf[u].l = wp[((u0 + u) * 3 + 2) * 64 + lane];
                }
                mfma6_blocks<2>(wf, ah, am, al, bh, bm, bl, &accA[NF + u0], &accB[NF + u0]);
            }
            fp32_step(1);
            if (!more) {
                w2_store(0, 0, wsp[0]);
                if (two) w2_store(1, 1, wsp[0]);
            }
            chunk_fence();
            par ^= 1;
        };
        f32x4 xan[KPB], xbn[KPB];
        int c = 0;
        for (; c + 1 < NC1; c += 2) {
            chunk(c, xa, xb, xan, xbn);
            chunk(c + 1, xan, xbn, xa, xb);
        }
        if (c < NC1) {  // an odd chunk count (never at 512-d x-vectors): one more, and the sets change places by copy
            chunk(c, xa, xb, xan, xbn);
#pragma unroll
            for (int s = 0; s < KPB; ++s) {
                xa[s] = xan[s];
                xb[s] = xbn[s];
            }
        }

        // ---- F.normalize (utils/models.py:368) ---------------------------------------------------------------
        {
            float ssA = 0.f, ssB = 0.f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ssA = fmaf(accA[nb][r], accA[nb][r], ssA);
                    ssB = fmaf(accB[nb][r], accB[nb][r], ssB);
                }
            }
            ssA = wave_xor_add(ssA, 16); ssA = wave_xor_add(ssA, 32);
            ssB = wave_xor_add(ssB, 16); ssB = wave_xor_add(ssB, 32);
            const float invA = 1.0f / fmaxf(sqrtf(ssA), 1e-12f);
            const float invB = 1.0f / fmaxf(sqrtf(ssB), 1e-12f);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                accA[nb] *= invA;
                accB[nb] *= invB;
            }
        }

        // ---- layer 2 in split form (nplda_fwd_v6.h): k32-step c takes accumulator blocks 2 c and 2 c + 1 -------------
        float part = 0.f;
        f32x4 zA[NB], zB[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            zA[nb] = b2p[4 * nb + g];
            zB[nb] = zA[nb];
        }
#pragma unroll
        for (int c2 = 0; c2 < KC2; ++c2) {
            const bool more = c2 + 1 < KC2;
            if (more) {
                w2_load(c2 + 1, 0, 0);
            } else {
                dma_l1(0, wbuf[par]);  // chunk 0 of the next tile (both layer-1 buffers are free here), its W1 unit and x rows
                w1_load(0);
                long long t0_x;
                bool ok_x;
                const float *pa, *pb;
                tile_ptrs(tile_n, t0_x, ok_x, pa, pb);
#pragma unroll
                for (int s = 0; s < KPB; ++s) {
                    xa[s] = load_xrow<XM>(pa, 16 * s + 4 * g, D0);
                    xb[s] = load_xrow<XM>(pb, 16 * s + 4 * g, D0);
                }
            }
            bf16x8 ah, am, al, bh, bm, bl;
            split3x8(accA[2 * c2], accA[2 * c2 + 1], ah, am, al);
            split3x8(accB[2 * c2], accB[2 * c2 + 1], bh, bm, bl);
            const bf16x8* w = wsp[c2 & 1];
#pragma unroll
            for (int nb = 0; nb < NB; nb += 2) {
                WFrag w0, w1;
                w0.h = w[(nb * 3 + 0) * 64 + lane];
                w0.m = w[(nb * 3 + 1) * 64 + lane];
                w0.l = w[(nb * 3 + 2) * 64 + lane];
                w1.h = w[(nb * 3 + 3) * 64 + lane];
                w1.m = w[(nb * 3 + 4) * 64 + lane];
                w1.l = w[(nb * 3 + 5) * 64 + lane];
                mfma6x4(w0, w1, ah, am, al, bh, bm, bl, zA[nb], zB[nb], zA[nb + 1], zB[nb + 1]);
                if (nb == 2 * ((NB / 2) / 2)) {  // past the middle: unit 0 has landed; unit 1 reuses its registers
                    if (more) {
                        w2_store(0, 0, wsp[(c2 + 1) & 1]);
                        w2_load(c2 + 1, 1, 0);
                    } else {
                        w1_store(0, wsp1[par]);
                        w1_load(cn1);
                    }
                }
            }
            if (more && two) w2_store(1, 0, wsp[(c2 + 1) & 1]);
            chunk_fence();
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const f32x4 q = Qp[4 * nb + g];
            const f32x4 p = Pp[4 * nb + g];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z1 = zA[nb][r], z2 = zB[nb][r];
                part = fmaf(q[r], fmaf(z1, z1, z2 * z2), part);
                part = fmaf(2.0f * p[r], z1 * z2, part);
            }
        }
        part = wave_xor_add(part, 16);
        part = wave_xor_add(part, 32);
        if (g == 0 && ok) a.out_s[t0 + j] = part;

        tile = tile_n;
        if (tile >= ntiles) break;
        tile_ptrs(tile, t0, ok, sa, sb);
    }
}

}  // namespace nplda
