// nplda_allpairs.hip — SoftCdet / BCE over ALL pairs of a batch of embeddings, with every gradient, in one pass (gfx950).
//
// The per-utterance counterpart of forward_from_plda_embeddings + loss + backward (utils/models.py:372-376, :384-399) on
// the trials a batch of N utterances implies (what TrialSampler, utils/sv_trials_loaders.py:22-75, enumerates pair by
// pair): T = {(i, j): i < j, grp[i] == grp[j]}, target iff spk[i] == spk[j],
//   s_ij = q_i + q_j + 2 sum_d P_d z_id z_jd,   q_i = sum_d Q_d z_id^2,   g_ij = dL/ds_ij (nplda_loss_math.h)
//   G symmetric with G_ij = G_ji = g_ij on T, 0 elsewhere;   r_i = sum_j G_ij,   A_i = sum_j G_ij z_j
//   dz_i = 2 r_i (Q o z_i) + 2 P o A_i,   dQ_d = sum_i r_i z_id^2,   dP_sqrt_d = 2 P_sqrt_d sum_i z_id A_id
// The N x N score and gradient matrices are never written: a block owns 64 rows i (four waves of 16), walks the column
// tiles j, forms a 16 x 16 piece of S^T on fp32-input MFMAs (A operand z_j, B operand P o z_i), turns it into G in the
// accumulator registers and hands those registers to a second MFMA chain as its B operand (Y^T += z_j^T G: the second
// product sums over the accumulator's ROW index j, so no transpose is needed).  design/k17_allpairs.md has the derivation,
// the tile shape and the budget.  Four launches, nothing else: counts (labels only), pad (z image, q), main, finish.
// Every sum is combined in a fixed order; there are no floating-point atomics and nothing is zeroed by a memset.
#include "nplda_loss_math.h"
#include "nplda_loss_single.h"

namespace {

using namespace nplda_loss;

constexpr int kRowTile = 64;     // rows i per block (NPLDA_ALLPAIRS_TILE)
constexpr int kColTile = 16;     // columns j per LDS stage: one 16 x 16 piece of S^T
constexpr int kCountTile = 256;  // rows per block of the label pre-pass
constexpr int kSumStride = 2 + 4 * kMaxK;
constexpr int64_t kMaxN = (int64_t)1 << 20;

static_assert(kRowTile == NPLDA_ALLPAIRS_TILE, "the header states the row tile");

struct WsLayout {
    size_t oZ, oq, ospk, ogrp, oP, oQ, ocnt, osums, odq, total;
    int64_t Np;
    int nblk, ncnt;
};

WsLayout ws_layout(int64_t N, int Dp) {
    WsLayout L;
    L.Np = (N + kRowTile - 1) / kRowTile * kRowTile;
    L.nblk = (int)(L.Np / kRowTile);
    L.ncnt = (int)((N + kCountTile - 1) / kCountTile);
    L.oZ = 0;
    L.oq = L.oZ + up256((size_t)L.Np * Dp * sizeof(float));
    L.ospk = L.oq + up256((size_t)L.Np * sizeof(float));
    L.ogrp = L.ospk + up256((size_t)L.Np * sizeof(int));
    L.oP = L.ogrp + up256((size_t)L.Np * sizeof(int));
    L.oQ = L.oP + up256((size_t)Dp * sizeof(float));
    L.ocnt = L.oQ + up256((size_t)Dp * sizeof(float));
    L.osums = L.ocnt + up256((size_t)L.ncnt * 2 * sizeof(long long));
    L.odq = L.osums + up256((size_t)L.nblk * kSumStride * sizeof(double));
    L.total = L.odq + up256((size_t)L.nblk * 2 * Dp * sizeof(float));
    return L;
}

// ---- N_t, N_n from the labels alone: block b counts the trials (i, j > i) of its 256 rows i ---------------------------------
__global__ __launch_bounds__(kCountTile) void ap_count(const int* __restrict__ spk, const int* __restrict__ grp, int N,
                                                       long long* __restrict__ cnt) {
    __shared__ int s_spk[kCountTile], s_grp[kCountTile];
    __shared__ long long red[kCountTile / 64][2];
    const int i = blockIdx.x * kCountTile + threadIdx.x;
    const int si = i < N ? spk[i] : 0;
    const int gi = (i < N && grp) ? grp[i] : 0;
    int nt = 0, nall = 0;
    for (int j0 = blockIdx.x * kCountTile; j0 < N; j0 += kCountTile) {
        __syncthreads();
        const int j = j0 + threadIdx.x;
        s_spk[threadIdx.x] = j < N ? spk[j] : 0;
        s_grp[threadIdx.x] = (j < N && grp) ? grp[j] : 0;
        __syncthreads();
        const int lim = N - j0 < kCountTile ? N - j0 : kCountTile;
        if (i < N) {
            for (int jj = 0; jj < lim; ++jj) {
                const int trial = (j0 + jj > i) & (s_grp[jj] == gi);
                nall += trial;
                nt += trial & (s_spk[jj] == si);
            }
        }
    }
    const long long wt = wave_sum(nt), wa = wave_sum(nall);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = wt;
        red[threadIdx.x >> 6][1] = wa - wt;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        long long v = 0;
        for (int w = 0; w < kCountTile / 64; ++w) v += red[w][threadIdx.x];
        cnt[2 * blockIdx.x + threadIdx.x] = v;
    }
}

// ---- zero-padded image of z (Np x Dp), q, the labels and P = P_sqrt^2, Q padded to Dp: 16 rows per block --------------------
__global__ __launch_bounds__(256) void ap_pad(const float* __restrict__ z, long long ldz, int N, int D2, int Dp,
                                              const int* __restrict__ spk, const int* __restrict__ grp,
                                              const float* __restrict__ P_sqrt, const float* __restrict__ Q,
                                              float* __restrict__ Zp, float* __restrict__ q, int* __restrict__ spk_p,
                                              int* __restrict__ grp_p, float* __restrict__ Pp, float* __restrict__ Qp) {
    const int c = threadIdx.x & 15;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
    float qa = 0.f;
    for (int d = c; d < Dp; d += 16) {
        const bool in = i < N && d < D2;
        const float v = in ? z[(long long)i * ldz + d] : 0.f;
        Zp[(size_t)i * Dp + d] = v;
        qa = fmaf((in ? Q[d] : 0.f) * v, v, qa);
    }
    qa = row16_sum(qa);
    if (c == 0) {
        q[i] = qa;
        spk_p[i] = i < N ? spk[i] : 0;
        grp_p[i] = (i < N && grp) ? grp[i] : 0;
    }
    if (blockIdx.x == 0) {
        for (int d = threadIdx.x; d < Dp; d += 256) {
            const float ps = d < D2 ? P_sqrt[d] : 0.f;
            Pp[d] = ps * ps;
            Qp[d] = d < D2 ? Q[d] : 0.f;
        }
    }
}

// ---- the main kernel.  LM: 0 = BCE, 1 .. 4 = SoftCdet with K = LM thresholds -------------------------------------------------
template <int NB, int LM>
__global__ __launch_bounds__(256, 2) void ap_main(const float* __restrict__ Zp, const float* __restrict__ q,
                                                  const int* __restrict__ spk, const int* __restrict__ grp,
                                                  const float* __restrict__ Pp, const float* __restrict__ Qp,
                                                  const long long* __restrict__ cnt, int ncnt, int N, int D2, ThetaPtrs th,
                                                  BetaVals beta, float alpha, int grad, float* __restrict__ dz,
                                                  long long lddz, double* __restrict__ psums, float* __restrict__ pdq) {
    constexpr int Dp = 16 * NB;
    constexpr int LD = Dp + 4;  // LDS row stride: the b128 reads of 16 rows and the b32 reads of rows 4 apart are conflict-free
    constexpr int K = LM == 0 ? 1 : LM;
    constexpr int NS = LM == 0 ? 4 : 2 + 4 * K;
    constexpr int NST = (kColTile * Dp / 4 + 255) / 256;  // float4 per thread of one stage
    __shared__ __attribute__((aligned(16))) float zs[kColTile * LD];
    __shared__ __attribute__((aligned(16))) float qs[kColTile];
    __shared__ __attribute__((aligned(16))) int ss[kColTile], gs[kColTile];
    __shared__ double red[4][NS];
    __shared__ long long cred[4][2];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int Np = gridDim.x * kRowTile;

    // N_t, N_n: integer sums, exact in any order
    long long ct_l = 0, cn_l = 0;
    for (int b = threadIdx.x; b < ncnt; b += 256) {
        ct_l += cnt[2 * b];
        cn_l += cnt[2 * b + 1];
    }
    ct_l = wave_sum(ct_l);
    cn_l = wave_sum(cn_l);
    if (lane == 0) {
        cred[wave][0] = ct_l;
        cred[wave][1] = cn_l;
    }
    __syncthreads();
    const double Nt = (double)(cred[0][0] + cred[1][0] + cred[2][0] + cred[3][0]);
    const double Nn = (double)(cred[0][1] + cred[1][1] + cred[2][1] + cred[3][1]);

    float theta[K], cn[K], ctc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) theta[k] = th.p[k][0];
    if constexpr (LM == 0) cn[0] = (float)(1.0 / (Nt + Nn));
    else softcdet_consts<K>(Nt, Nn, beta, alpha, cn, ctc);

    // this wave's 16 rows i: B operand of the first product, P o z_i, feature 16 qb + 4 g + m in pz[qb][m]
    const int i = blockIdx.x * kRowTile + 16 * wave + c;
    const float* zi = Zp + (size_t)i * Dp + 4 * g;
    f32x4 pz[NB];
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) pz[qb] = *(const f32x4*)(zi + 16 * qb) * *(const f32x4*)(Pp + 16 * qb + 4 * g);
    const float qi = q[i];
    const int spi = spk[i], gpi = grp[i];

    f32x4 Y[NB];
#pragma unroll
    for (int db = 0; db < NB; ++db) Y[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float rs = 0.f;
    double acc[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = 0.0;

    // without gradients only the tiles that hold a pair i < j are walked
    const int jbeg = grad ? 0 : blockIdx.x * kRowTile;
    f32x4 st[NST];
    float pq = 0.f;
    int psp = 0, pgp = 0;
    auto fetch = [&](int j0) {
        const f32x4* src = (const f32x4*)(Zp + (size_t)j0 * Dp);
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kColTile * Dp / 4) st[u] = src[e];
        }
        if (threadIdx.x < kColTile) {
            pq = q[j0 + threadIdx.x];
            psp = spk[j0 + threadIdx.x];
            pgp = grp[j0 + threadIdx.x];
        }
    };
    fetch(jbeg);
    for (int j0 = jbeg; j0 < Np; j0 += kColTile) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kColTile * Dp / 4) *(f32x4*)(zs + (e / (4 * NB)) * LD + 4 * (e % (4 * NB))) = st[u];
        }
        if (threadIdx.x < kColTile) {
            qs[threadIdx.x] = pq;
            ss[threadIdx.x] = psp;
            gs[threadIdx.x] = pgp;
        }
        __syncthreads();
        if (j0 + kColTile < Np) fetch(j0 + kColTile);

        // S^T piece: rows j = 4 g + r in register r, column i = c on the lane.  The feature sum runs as TWO chains (even and
        // odd 16-blocks) that are added at the end: a single fp32 chain of 150+ terms carries twice the rounding error of
        // its halves (measured: 2.4 against 1.0 units of the score's last place), and two independent accumulators also keep
        // the MFMA pipe fed (40 cycles of dependent latency against 32 of issue).
        f32x4 S0 = f32x4{0.f, 0.f, 0.f, 0.f}, S1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            const f32x4 a = *(const f32x4*)(zs + c * LD + 16 * qb + 4 * g);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (qb & 1) S1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], pz[qb][m], S1, 0, 0, 0);
                else S0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], pz[qb][m], S0, 0, 0, 0);
            }
        }
        const f32x4 S = S0 + S1;
        const f32x4 qj = *(const f32x4*)(qs + 4 * g);
        const int4 spj = *(const int4*)(ss + 4 * g);
        const int4 gpj = *(const int4*)(gs + 4 * g);
        const int sp4[4] = {spj.x, spj.y, spj.z, spj.w}, gp4[4] = {gpj.x, gpj.y, gpj.z, gpj.w};
        f32x4 G;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const bool valid = (i < N) & (j < N) & (i != j) & (gp4[r] == gpi);
            const float t = sp4[r] == spi ? 1.0f : 0.0f;
            const float s = fmaf(2.0f, S[r], qi + qj[r]);
            float gv = 0.f;
            if (valid) {
                if constexpr (LM == 0) {
                    gv = bce_gi(s, t, theta[0], cn[0]);
                    if (i < j) bce_accumulate(s, t, theta[0], acc);
                } else {
                    gv = softcdet_gi<K>(s, t, theta, cn, ctc, alpha);
                    if (i < j) softcdet_accumulate<K, false>(s, t, theta, alpha, acc);
                }
            }
            G[r] = gv;
        }
        rs += (G[0] + G[1]) + (G[2] + G[3]);
        if (grad) {
            // Y^T (d, i) += sum_j z_jd G_ji: A operand z^T (row d = 16 db + c, k = g <-> j = 4 g + r), B operand G[r] as it lies
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* zr = zs + (4 * g + r) * LD + c;
#pragma unroll
                for (int db = 0; db < NB; ++db) Y[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(zr[16 * db], G[r], Y[db], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: r_i over the four row groups of the lanes, dz_i, this block's share of dQ and sum_i z_id A_id -------------
    const float ri = wave_xor_add(wave_xor_add(rs, 16), 32);
    __syncthreads();           // every wave has finished reading zs: reused for the block's column sums
    float* cq = zs;            // [wave][Dp]
    float* cp = zs + 4 * Dp;   // [wave][Dp]
    if (grad) {
#pragma unroll
        for (int db = 0; db < NB; ++db) {
            const f32x4 z4 = *(const f32x4*)(zi + 16 * db);
            const f32x4 Q4 = *(const f32x4*)(Qp + 16 * db + 4 * g), P4 = *(const f32x4*)(Pp + 16 * db + 4 * g);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int d = 16 * db + 4 * g + m;
                if (dz != nullptr && i < N && d < D2)
                    dz[(long long)i * lddz + d] = 2.0f * fmaf(ri * Q4[m], z4[m], P4[m] * Y[db][m]);
                const float sq = row16_sum(ri * z4[m] * z4[m]);
                const float sp = row16_sum(z4[m] * Y[db][m]);
                if (c == 0) {
                    cq[wave * Dp + d] = sq;
                    cp[wave * Dp + d] = sp;
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        const double v = wave_sum(acc[n]);
        if (lane == 0) red[wave][n] = v;
    }
    __syncthreads();
    if (grad) {
        for (int d = threadIdx.x; d < Dp; d += 256) {
            pdq[(size_t)blockIdx.x * 2 * Dp + d] = ((cq[d] + cq[Dp + d]) + cq[2 * Dp + d]) + cq[3 * Dp + d];
            pdq[(size_t)blockIdx.x * 2 * Dp + Dp + d] = ((cp[d] + cp[Dp + d]) + cp[2 * Dp + d]) + cp[3 * Dp + d];
        }
    }
    if (threadIdx.x < NS)
        psums[(size_t)blockIdx.x * kSumStride + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- one block: the blocks' partial sums in block order, loss and dL/dtheta, dQ and dP_sqrt ---------------------------------
template <int LM>
__global__ __launch_bounds__(256) void ap_finish(const double* __restrict__ psums, const float* __restrict__ pdq,
                                                 const long long* __restrict__ cnt, int ncnt, int nblk, int Dp, int D2,
                                                 const float* __restrict__ P_sqrt, BetaVals beta, float alpha,
                                                 double* __restrict__ sums, float* loss, float* dtheta,
                                                 float* __restrict__ dP_sqrt, float* __restrict__ dQ) {
    constexpr int K = LM == 0 ? 1 : LM;
    constexpr int NS = LM == 0 ? 4 : 2 + 4 * K;
    __shared__ double tot[NS];
    if (threadIdx.x < NS) {
        double v = 0.0;
        if (threadIdx.x < 2) {
            long long n = 0;
            for (int b = 0; b < ncnt; ++b) n += cnt[2 * b + threadIdx.x];
            v = (double)n;
        } else {
            for (int b = 0; b < nblk; ++b) v += psums[(size_t)b * kSumStride + threadIdx.x];
        }
        tot[threadIdx.x] = v;
        sums[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (LM == 0) bce_scalars(tot, loss, dtheta);
        else softcdet_scalars<K>(tot, beta, alpha, loss, dtheta);
    }
    if (dP_sqrt == nullptr && dQ == nullptr) return;
    for (int d = threadIdx.x; d < D2; d += 256) {
        float aq = 0.f, ap = 0.f;
        for (int b = 0; b < nblk; ++b) {
            aq += pdq[(size_t)b * 2 * Dp + d];
            ap += pdq[(size_t)b * 2 * Dp + Dp + d];
        }
        if (dQ) dQ[d] = aq;
        if (dP_sqrt) dP_sqrt[d] = 2.0f * P_sqrt[d] * ap;
    }
}

struct MainArgs {
    const float *Zp, *q;
    const int *spk, *grp;
    const float *Pp, *Qp;
    const long long* cnt;
    int ncnt, N, D2;
    ThetaPtrs th;
    BetaVals beta;
    float alpha;
    int grad;
    float* dz;
    long long lddz;
    double* psums;
    float* pdq;
};

template <int NB, int LM>
void launch_main(const MainArgs& a, int nblk, hipStream_t st) {
    hipLaunchKernelGGL((ap_main<NB, LM>), dim3(nblk), dim3(256), 0, st, a.Zp, a.q, a.spk, a.grp, a.Pp, a.Qp, a.cnt, a.ncnt,
                       a.N, a.D2, a.th, a.beta, a.alpha, a.grad, a.dz, a.lddz, a.psums, a.pdq);
}

template <int NB>
void launch_main_lm(int lm, const MainArgs& a, int nblk, hipStream_t st) {
    switch (lm) {
        case 0: launch_main<NB, 0>(a, nblk, st); break;
        case 1: launch_main<NB, 1>(a, nblk, st); break;
        case 2: launch_main<NB, 2>(a, nblk, st); break;
        case 3: launch_main<NB, 3>(a, nblk, st); break;
        default: launch_main<NB, 4>(a, nblk, st); break;
    }
}

}  // namespace

extern "C" {

size_t nplda_allpairs_workspace_bytes(int64_t N, int D2, int K) {
    if (N < 0 || N > kMaxN || D2 <= 0 || K < 1 || K > kMaxK) return 0;
    const int nb = nplda_kernel_nb(D2, D2);
    if (nb == 0) return 0;
    return ws_layout(N, 16 * nb).total;
}

int nplda_allpairs_loss_f32(const float* z, int64_t ldz, int64_t N, int D2, const int32_t* spk, const int32_t* grp,
                            const float* P_sqrt, const float* Q, const float* const* theta, const float* beta, int K,
                            float alpha, int kind, double* sums, float* loss, float* dtheta, float* dz, int64_t lddz,
                            float* dP_sqrt, float* dQ, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    if (kind != 0 && kind != 1) return NPLDA_EINVAL;
    if (K < 1 || K > kMaxK || N < 0 || D2 <= 0) return NPLDA_EINVAL;
    if (N == 0) return NPLDA_OK;  // (an empty batch has no pointers to check)
    if (!z || !spk || !P_sqrt || !Q || !theta || !sums || !loss || !ws) return NPLDA_EINVAL;
    if (kind == 0 && !beta) return NPLDA_EINVAL;
    if (ldz < D2 || (ldz & 3) || !nplda_aligned16(z) || !nplda_aligned16(ws)) return NPLDA_EINVAL;
    if (dz && (lddz < D2 || (lddz & 3) || !nplda_aligned16(dz))) return NPLDA_EINVAL;
    ThetaPtrs th = {};
    BetaVals bv = {};
    for (int k = 0; k < (kind == 1 ? 1 : K); ++k) {
        if (!theta[k]) return NPLDA_EINVAL;
        th.p[k] = theta[k];
        if (kind != 1) bv.b[k] = beta[k];
    }
    const int nb = nplda_kernel_nb(D2, D2);
    if (nb == 0 || N > kMaxN) return NPLDA_EUNSUPPORTED;
    const int Dp = 16 * nb;
    const WsLayout L = ws_layout(N, Dp);
    if (ws_bytes < L.total) return NPLDA_ENOSPC;

    char* w = (char*)ws;
    float* Zp = (float*)(w + L.oZ);
    float* q = (float*)(w + L.oq);
    int* spk_p = (int*)(w + L.ospk);
    int* grp_p = (int*)(w + L.ogrp);
    float* Pp = (float*)(w + L.oP);
    float* Qp = (float*)(w + L.oQ);
    long long* cnt = (long long*)(w + L.ocnt);
    double* psums = (double*)(w + L.osums);
    float* pdq = (float*)(w + L.odq);
    hipStream_t st = (hipStream_t)stream;

    hipLaunchKernelGGL(ap_count, dim3(L.ncnt), dim3(kCountTile), 0, st, (const int*)spk, (const int*)grp, (int)N, cnt);
    hipLaunchKernelGGL(ap_pad, dim3((unsigned)(L.Np / 16)), dim3(256), 0, st, z, (long long)ldz, (int)N, D2, Dp,
                       (const int*)spk, (const int*)grp, P_sqrt, Q, Zp, q, spk_p, grp_p, Pp, Qp);
    MainArgs a = {Zp, q, spk_p, grp_p, Pp, Qp, cnt, L.ncnt, (int)N, D2, th, bv, alpha,
                  (dz || dP_sqrt || dQ) ? 1 : 0, dz, (long long)lddz, psums, pdq};
    const int lm = kind == 1 ? 0 : K;
    switch (nb) {
        case 2: launch_main_lm<2>(lm, a, L.nblk, st); break;
        case 4: launch_main_lm<4>(lm, a, L.nblk, st); break;
        case 8: launch_main_lm<8>(lm, a, L.nblk, st); break;
        case 10: launch_main_lm<10>(lm, a, L.nblk, st); break;
        case 11: launch_main_lm<11>(lm, a, L.nblk, st); break;
        default: launch_main_lm<12>(lm, a, L.nblk, st); break;
    }
#define NPLDA_AP_FINISH(LM)                                                                                              \
    hipLaunchKernelGGL(ap_finish<LM>, dim3(1), dim3(256), 0, st, (const double*)psums, (const float*)pdq,                \
                       (const long long*)cnt, L.ncnt, L.nblk, Dp, D2, P_sqrt, bv, alpha, sums, loss, dtheta, dP_sqrt, dQ)
    switch (lm) {
        case 0: NPLDA_AP_FINISH(0); break;
        case 1: NPLDA_AP_FINISH(1); break;
        case 2: NPLDA_AP_FINISH(2); break;
        case 3: NPLDA_AP_FINISH(3); break;
        default: NPLDA_AP_FINISH(4); break;
    }
#undef NPLDA_AP_FINISH
    return nplda_launch_status();
}

}  // extern "C"
