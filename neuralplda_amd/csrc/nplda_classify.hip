// nplda_classify.hip — speaker-classification loss (softmax, AM-softmax, AAM-softmax) over a class table, with every
// gradient, without the N x C logits (gfx950).
//
// Embeddings X (N, D), class table W (C, D), optional bias b (C), labels y (N), kind, scale s, margin m:
//   kind 0: u_ic = <x_i, w_c>;  kinds 1, 2: u_ic = <x^_i, w^_c>,  x^ = x / max(||x||, 1e-12)  (F.normalize)
//   a_ic = s u_ic + b_c (inference logit);  l_ic = a_ic for c != y_i,  l_iy = s phi(u_iy) + b_y
//   phi(u) = u (kind 0), u - m (kind 1); kind 2: v = clamp(u, -1, 1), sn = sqrt(max(1 - v^2, 2^-24)),
//     v > -cos m: phi = v cos m - sn sin m, phi' = cos m + (v / sn) sin m;  else phi = v - m sin m, phi' = 1
//   V = {i: 0 <= y_i < C};  lse_i = log sum_c exp l_ic;  rowloss_i = lse_i - l_iy on V, 0 elsewhere;  loss = sum_V rowloss / |V|
//   pred_i = argmax_c a_ic (lowest index on ties);  g_ic = (exp(l_ic - lse_i) - [c = y_i]) / |V| on V, 0 elsewhere
//   db_c = sum_i g_ic;  h_ic = s g_ic (times phi'(u_iy) at c = y_i);  kind 0: dX = H W, dW = H^T X;
//   kinds 1, 2: A = H W^, dX_i = (A_i - <x^_i, A_i> x^_i) / max(||x_i||, 1e-12), dW likewise from H^T X^.
// One device body (cl_main) in two orientations, the MFMA arrangement of nplda_allpairs.hip: a block OWNS 64 rows of one
// padded image (B operand of the first product, in registers for the whole walk) and WALKS 16-row tiles of the other
// through LDS (A operand); the 16 x 16 piece of logits comes out with the owner on the lane and the walked index in the
// registers, is turned into h in those registers and handed to the second product as its B operand.  "Rows own" walks a
// chunk of the class tiles (LSE pass: running max / sum of exponentials, best inference logit, the target's u and l; GRAD
// pass: one partial of A per class chunk); "classes own" walks a chunk of the row tiles (one partial of H^T X^ and of db
// per row chunk).  Launches: pad, LSE, merge, scalars, then GRAD rows-own + finish and GRAD classes-own + finish (the two
// passes share one region for their partials) — nothing else.  Every sum is combined in a fixed order; no floating-point
// atomics, no memset.  design/k26_classify.md has the derivation.
#include <float.h>
#include <math.h>
#include "nplda_common.h"

namespace {

constexpr int kOwn = 64;             // rows of the owned image per block: four waves of 16
constexpr int kWalk = 16;            // rows of the walked image per LDS stage
constexpr int kMergeRows = 256;      // rows per block of the merge kernel
constexpr int kTargetBlocks = 512;   // the plan aims at two blocks for each of 256 CUs (a constant, not a device query)
constexpr int kPlanMaxChunks = 64;   // the plan's cap on chunks
constexpr int kMinChunkTiles = 16;   // the plan makes no chunk shorter than 16 walked tiles (256 classes or rows)
constexpr int kMaxChunks = 1024;     // cap on a caller's forced chunk count
constexpr int kLseFields = 6;        // max, sum, best a, best index, target u, target l
constexpr int64_t kMaxN = (int64_t)1 << 20;
constexpr int64_t kMaxC = (int64_t)1 << 20;

inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
inline int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

// Chunks of the walk for `own_tiles` owner blocks over `walk_tiles` tiles: a function of the shape alone.
int64_t want_chunks(int64_t own_tiles, int64_t walk_tiles, int forced) {
    own_tiles = imax(own_tiles, 1);  // (N == 0 or C == 0: a size is still reported, nothing is launched)
    if (forced > 0) return imax(1, imin(imin(forced, walk_tiles), kMaxChunks));
    const int64_t cap = imax(1, imin(kPlanMaxChunks, walk_tiles / kMinChunkTiles));
    return imax(1, imin(cap, (kTargetBlocks + own_tiles - 1) / own_tiles));
}

// chunks x owner tiles never exceeds this, and it never decreases with either tile count (the workspace is sized by it)
int64_t chunk_tiles_bound(int64_t own_tiles, int64_t walk_tiles, int forced) {
    if (forced > 0) return want_chunks(own_tiles, walk_tiles, forced) * own_tiles;
    const int64_t cap = imax(1, imin(kPlanMaxChunks, walk_tiles / kMinChunkTiles));
    return imin(cap * own_tiles, kTargetBlocks + own_tiles);
}

struct WsLayout {
    size_t oX, oW, onx, onw, oy, ob, olse, olp, obs, obc, ocnt, oA, oB, odb, total;
    int64_t Np, Cp;
    int cc, cper, rc, rper, nmb;  // class chunks and class tiles per chunk, row chunks and row tiles per chunk, merge blocks
};

WsLayout ws_layout(int64_t N, int64_t C, int Dp, int class_chunks, int row_chunks) {
    WsLayout L;
    L.Np = (N + kOwn - 1) / kOwn * kOwn;
    L.Cp = (C + kOwn - 1) / kOwn * kOwn;
    const int64_t rt = L.Np / kOwn, ct = L.Cp / kOwn;                          // owner tiles
    const int64_t rw = (N + kWalk - 1) / kWalk, cw = (C + kWalk - 1) / kWalk;  // walked tiles
    const int64_t cc = want_chunks(rt, cw, class_chunks), rc = want_chunks(ct, rw, row_chunks);
    L.cper = (int)imax(1, (cw + cc - 1) / cc);
    L.cc = (int)imax(1, (cw + L.cper - 1) / L.cper);
    L.rper = (int)imax(1, (rw + rc - 1) / rc);
    L.rc = (int)imax(1, (rw + L.rper - 1) / L.rper);
    L.nmb = (int)((L.Np + kMergeRows - 1) / kMergeRows);
    const size_t ctb = (size_t)chunk_tiles_bound(rt, cw, class_chunks) * kOwn;  // >= cc * Np
    const size_t rtb = (size_t)chunk_tiles_bound(ct, rw, row_chunks) * kOwn;    // >= rc * Cp
    L.oX = 0;
    L.oW = L.oX + up256((size_t)L.Np * Dp * sizeof(float));
    L.onx = L.oW + up256((size_t)L.Cp * Dp * sizeof(float));
    L.onw = L.onx + up256((size_t)L.Np * sizeof(float));
    L.oy = L.onw + up256((size_t)L.Cp * sizeof(float));
    L.ob = L.oy + up256((size_t)L.Np * sizeof(int));
    L.olse = L.ob + up256((size_t)L.Cp * sizeof(float));
    L.olp = L.olse + up256((size_t)L.Np * sizeof(float));
    L.obs = L.olp + up256(ctb * kLseFields * sizeof(float));
    L.obc = L.obs + up256((size_t)L.nmb * sizeof(double));
    L.ocnt = L.obc + up256((size_t)L.nmb * 3 * sizeof(long long));
    L.oA = L.ocnt + up256(4 * sizeof(long long));
    L.oB = L.oA;  // one region for the partials of both gradient passes: each is finished before the next is launched
    L.odb = L.oA + up256((ctb > rtb ? ctb : rtb) * Dp * sizeof(float));
    L.total = L.odb + up256(rtb * sizeof(float));
    return L;
}

// ---- zero-padded images of X (Np x Dp) and W (Cp x Dp), divided by the row norms for kinds 1 and 2; the norms, the labels
// ---- padded with -1 and the bias padded with 0: 16 rows per block, 16 lanes per row -----------------------------------------
__global__ __launch_bounds__(256) void cl_pad(const float* __restrict__ X, long long ldx, int N, const float* __restrict__ W,
                                              long long ldw, int C, int D, int Dp, int normalise,
                                              const float* __restrict__ b, const int* __restrict__ y, int nxblk,
                                              float* __restrict__ Xp, float* __restrict__ Wp, float* __restrict__ nx,
                                              float* __restrict__ nw, int* __restrict__ yp, float* __restrict__ bp) {
    const int c = threadIdx.x & 15;
    const bool isx = (int)blockIdx.x < nxblk;
    const int i = ((int)blockIdx.x - (isx ? 0 : nxblk)) * 16 + (threadIdx.x >> 4);
    const float* src = isx ? X : W;
    const long long ld = isx ? ldx : ldw;
    const int n = isx ? N : C;
    float* dst = (isx ? Xp : Wp) + (size_t)i * Dp;
    float ss = 0.f;
    for (int d = c; d < Dp; d += 16) {
        const float v = (i < n && d < D) ? src[(long long)i * ld + d] : 0.f;
        ss = fmaf(v, v, ss);
    }
    ss = row16_sum(ss);
    const float nrm = normalise ? fmaxf(sqrtf(ss), 1e-12f) : 1.0f;
    for (int d = c; d < Dp; d += 16) {
        const float v = (i < n && d < D) ? src[(long long)i * ld + d] : 0.f;
        dst[d] = normalise ? v / nrm : v;
    }
    if (c == 0) {
        if (isx) {
            nx[i] = nrm;
            yp[i] = i < N ? y[i] : -1;
        } else {
            nw[i] = nrm;
            bp[i] = (i < C && b != nullptr) ? b[i] : 0.f;
        }
    }
}

struct Margin {
    int kind;
    float s, m, cosm, sinm, msinm;
};

// phi(u) and phi'(u) of the target's logit
__device__ __forceinline__ void margin_phi(const Margin& k, float u, float& phi, float& dphi) {
    phi = u;
    dphi = 1.0f;
    if (k.kind == 1) {
        phi = u - k.m;
    } else if (k.kind == 2) {
        const float v = fminf(fmaxf(u, -1.0f), 1.0f);
        const float sn = sqrtf(fmaxf(fmaf(-v, v, 1.0f), 0x1p-24f));
        if (v > -k.cosm) {
            phi = fmaf(v, k.cosm, -(sn * k.sinm));
            dphi = fmaf(v / sn, k.sinm, k.cosm);
        } else {
            phi = v - k.msinm;
        }
    }
}

struct MainArgs {
    const float* own;      // the owned image: Xp (rows own) or Wp (classes own)
    const float* walk;     // the walked image
    const int* yp;         // labels, Np
    const float* bp;       // bias, Cp
    const float* lse;      // lse_i, Np (GRAD)
    const long long* cnt;  // cnt[0] = |V| (GRAD)
    long long ownP;        // rows of the owned image
    int C, per, ntiles;    // classes; walked tiles per chunk and in all
    Margin k;
    float* out;            // LSE: kLseFields planes of [chunk][Np]; GRAD: [chunk][ownP][Dp]
    float* pdb;            // classes own: [chunk][Cp]
};

// ---- the main kernel: ROWS = rows own (walk classes) or classes own (walk rows); GRAD = gradient pass or LSE pass ----------
template <int NB, bool ROWS, bool GRAD>
__global__ __launch_bounds__(256, 2) void cl_main(const MainArgs a) {
    static_assert(ROWS || GRAD, "the LSE pass exists in the rows-own orientation only");
    constexpr int Dp = 16 * NB;
    constexpr int LD = Dp + 4;  // LDS row stride, as in nplda_allpairs.hip: both operand reads are conflict-free
    constexpr int NST = (kWalk * Dp / 4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float zs[kWalk * LD];
    __shared__ __attribute__((aligned(16))) float fs[kWalk];  // rows own: b_c of the walked classes; classes own: lse_i of the walked rows
    __shared__ __attribute__((aligned(16))) int is[kWalk];    // classes own: y_i of the walked rows

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int C = a.C;
    const float s = a.k.s;

    // this wave's 16 owners: B operand of the first product, feature 16 qb + 4 g + m in ob[qb][m]
    const int o = blockIdx.x * kOwn + 16 * wave + c;
    const float* op = a.own + (size_t)o * Dp + 4 * g;
    f32x4 ob[NB];
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) ob[qb] = *(const f32x4*)(op + 16 * qb);
    const int yo = ROWS ? a.yp[o] : 0;
    const float fo = ROWS ? (GRAD ? a.lse[o] : 0.f) : a.bp[o];
    float invV = 0.f;
    if constexpr (GRAD) invV = (float)(1.0 / (double)a.cnt[0]);

    f32x4 Y[NB];
#pragma unroll
    for (int db = 0; db < NB; ++db) Y[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float rs = 0.f;                                     // classes own: sum_i g_ic of this lane's rows
    float mrun = -FLT_MAX, srun = 0.f;                  // LSE: running max and sum of exp(l - max) of this lane's classes
    float ba = -INFINITY, tu = 0.f, tl = 0.f;           // best inference logit; the target's u and l
    int bi = 0x7fffffff;

    const int t0 = blockIdx.y * a.per;
    const int t1 = t0 + a.per < a.ntiles ? t0 + a.per : a.ntiles;
    f32x4 st[NST];
    float pf = 0.f;
    int pi = 0;
    auto fetch = [&](int j0) {
        const f32x4* src = (const f32x4*)(a.walk + (size_t)j0 * Dp);
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kWalk * Dp / 4) st[u] = src[e];
        }
        if (threadIdx.x < kWalk) {
            if constexpr (ROWS) {
                pf = a.bp[j0 + threadIdx.x];
            } else {
                pf = a.lse[j0 + threadIdx.x];
                pi = a.yp[j0 + threadIdx.x];
            }
        }
    };
    fetch(t0 * kWalk);
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * kWalk;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kWalk * Dp / 4) *(f32x4*)(zs + (e / (4 * NB)) * LD + 4 * (e % (4 * NB))) = st[u];
        }
        if (threadIdx.x < kWalk) {
            fs[threadIdx.x] = pf;
            is[threadIdx.x] = pi;
        }
        __syncthreads();
        if (t + 1 < t1) fetch(j0 + kWalk);

        // the piece of logits: walked index 4 g + r in register r, the owner c on the lane; two chains (even and odd
        // sixteen-feature blocks) added at the end, as design/k17_allpairs.md measures
        f32x4 S0 = f32x4{0.f, 0.f, 0.f, 0.f}, S1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            const f32x4 av = *(const f32x4*)(zs + c * LD + 16 * qb + 4 * g);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (qb & 1) S1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], ob[qb][m], S1, 0, 0, 0);
                else S0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], ob[qb][m], S0, 0, 0, 0);
            }
        }
        const f32x4 S = S0 + S1;
        const f32x4 f4 = *(const f32x4*)(fs + 4 * g);
        const int4 iv = *(const int4*)(is + 4 * g);
        const int i4[4] = {iv.x, iv.y, iv.z, iv.w};
        f32x4 H = f32x4{0.f, 0.f, 0.f, 0.f};
        float l4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int w = j0 + 4 * g + r;
            const int cls = ROWS ? w : o;
            const int yi = ROWS ? yo : i4[r];
            const float bc = ROWS ? f4[r] : fo;
            const float u = S[r];
            const float ai = fmaf(s, u, bc);
            const bool in = cls < C;
            const bool tgt = in && cls == yi;
            float l = ai, dphi = 1.0f;
            if (tgt) {
                float phi;
                margin_phi(a.k, u, phi, dphi);
                l = fmaf(s, phi, bc);
            }
            if constexpr (GRAD) {
                const float lsei = ROWS ? fo : f4[r];
                float gv = 0.f;
                if (in && yi >= 0 && yi < C) gv = (expf(l - lsei) - (tgt ? 1.0f : 0.0f)) * invV;
                rs += gv;
                H[r] = (s * gv) * dphi;
            } else {
                l4[r] = in ? l : -INFINITY;
                if (in && ai > ba) {  // classes come in increasing order: a strict compare keeps the lowest index
                    ba = ai;
                    bi = cls;
                }
                if (tgt) {
                    tu = u;
                    tl = l;
                }
            }
        }
        if constexpr (GRAD) {
            // Y^T (d, owner) += sum_w walked_wd H_w,owner: A operand the staged tile transposed, B operand H[r] as it lies
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* zr = zs + (4 * g + r) * LD + c;
#pragma unroll
                for (int db = 0; db < NB; ++db) Y[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(zr[16 * db], H[r], Y[db], 0, 0, 0);
            }
        } else {
            const float mn = fmaxf(mrun, fmaxf(fmaxf(l4[0], l4[1]), fmaxf(l4[2], l4[3])));
            srun = fmaf(srun, expf(mrun - mn), (expf(l4[0] - mn) + expf(l4[1] - mn)) + (expf(l4[2] - mn) + expf(l4[3] - mn)));
            mrun = mn;
        }
    }

    if constexpr (GRAD) {
        // the partial of this chunk: feature 16 db + 4 g + m of owner c in Y[db][m]
        float* dst = a.out + ((size_t)blockIdx.y * a.ownP + o) * Dp + 4 * g;
#pragma unroll
        for (int db = 0; db < NB; ++db) *(f32x4*)(dst + 16 * db) = Y[db];
        if constexpr (!ROWS) {
            const float r4 = wave_xor_add(wave_xor_add(rs, 16), 32);
            if (g == 0) a.pdb[(size_t)blockIdx.y * a.ownP + o] = r4;
        }
    } else {
        // the four lanes of a row (g = 0 .. 3), combined in that order by every one of them
        float mk[4], sk[4], bk[4];
        int ik[4];
        float tus = 0.f, tls = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mk[k] = __shfl(mrun, c + 16 * k, 64);
            sk[k] = __shfl(srun, c + 16 * k, 64);
            bk[k] = __shfl(ba, c + 16 * k, 64);
            ik[k] = __shfl(bi, c + 16 * k, 64);
            tus += __shfl(tu, c + 16 * k, 64);  // (one lane at the most holds the target: the others add 0)
            tls += __shfl(tl, c + 16 * k, 64);
        }
        const float M = fmaxf(fmaxf(mk[0], mk[1]), fmaxf(mk[2], mk[3]));
        const float Ssum = ((sk[0] * expf(mk[0] - M) + sk[1] * expf(mk[1] - M)) + sk[2] * expf(mk[2] - M)) + sk[3] * expf(mk[3] - M);
        float bb = bk[0];
        int bx = ik[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            if (bk[k] > bb || (bk[k] == bb && ik[k] < bx)) {
                bb = bk[k];
                bx = ik[k];
            }
        }
        if (g == 0) {
            const size_t plane = (size_t)gridDim.y * a.ownP;
            float* dst = a.out + (size_t)blockIdx.y * a.ownP + o;
            dst[0] = M;
            dst[plane] = Ssum;
            dst[2 * plane] = bb;
            dst[3 * plane] = __int_as_float(bx);
            dst[4 * plane] = tus;
            dst[5 * plane] = tls;
        }
    }
}

// ---- the class chunks of a row in chunk order: lse_i, rowloss_i, pred_i; per block of 256 rows the fp64 sum of rowloss in
// ---- row order and the three counts ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMergeRows) void cl_merge(const float* __restrict__ part, int nch, long long Np, int per,
                                                       const int* __restrict__ yp, int N, int C, float* __restrict__ lse,
                                                       float* __restrict__ rowloss, int* __restrict__ pred,
                                                       double* __restrict__ bsum, long long* __restrict__ bcnt) {
    __shared__ float s_loss[kMergeRows];
    __shared__ int s_flag[kMergeRows];
    const long long i = (long long)blockIdx.x * kMergeRows + threadIdx.x;
    float rl = 0.f;
    int flag = 0;
    if (i < Np) {
        const size_t plane = (size_t)nch * Np;
        float M = -FLT_MAX, Ssum = 0.f, bb = -INFINITY;
        int bx = 0x7fffffff;
        for (int ch = 0; ch < nch; ++ch) {
            const float* p = part + (size_t)ch * Np + i;
            const float m2 = p[0], s2 = p[plane], b2 = p[2 * plane];
            const int i2 = __float_as_int(p[3 * plane]);
            const float mn = fmaxf(M, m2);
            Ssum = Ssum * expf(M - mn) + s2 * expf(m2 - mn);
            M = mn;
            if (b2 > bb) {  // chunks hold increasing classes
                bb = b2;
                bx = i2;
            }
        }
        const float ls = M + logf(Ssum);
        lse[i] = ls;
        const int yi = yp[i];
        const int px = bx == 0x7fffffff ? 0 : bx;
        if (i < N) {
            if (yi >= 0 && yi < C) {
                const int ch = (yi / kWalk) / per;
                rl = ls - part[5 * plane + (size_t)ch * Np + i];
                flag = 1 | (px == yi ? 2 : 0);
            } else if (yi != -1) {
                flag = 4;
            }
            if (rowloss != nullptr) rowloss[i] = rl;
            if (pred != nullptr) pred[i] = px;
        }
    }
    s_loss[threadIdx.x] = rl;
    s_flag[threadIdx.x] = flag;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        long long nv = 0, nc = 0, nb = 0;
        for (int k = 0; k < kMergeRows; ++k) {
            const int f = s_flag[k];
            if (f & 1) acc += (double)s_loss[k];
            nv += f & 1;
            nc += (f >> 1) & 1;
            nb += (f >> 2) & 1;
        }
        bsum[blockIdx.x] = acc;
        bcnt[3 * blockIdx.x] = nv;
        bcnt[3 * blockIdx.x + 1] = nc;
        bcnt[3 * blockIdx.x + 2] = nb;
    }
}

// ---- one thread: the merge blocks in block order -> loss, counts, and |V| for the gradient passes ----------------------------
__global__ void cl_scalars(const double* __restrict__ bsum, const long long* __restrict__ bcnt, int nblk,
                           float* __restrict__ loss, long long* __restrict__ counts, long long* __restrict__ cnt) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double acc = 0.0;
    long long nv = 0, nc = 0, nb = 0;
    for (int b = 0; b < nblk; ++b) {
        acc += bsum[b];
        nv += bcnt[3 * b];
        nc += bcnt[3 * b + 1];
        nb += bcnt[3 * b + 2];
    }
    *loss = nv > 0 ? (float)(acc / (double)nv) : __int_as_float(0x7fc00000);
    counts[0] = nv;
    counts[1] = nc;
    counts[2] = nb;
    cnt[0] = nv;
}

struct FinishSide {
    const float* part;  // [chunk][P][Dp]
    const float* img;   // the normalised image, [P][Dp]
    const float* nrm;   // the row norms, [P]
    float* out;         // (n, ld), may be NULL on the class side when only db is wanted
    long long ld, P;
    int n, nch;
};

// ---- partials in chunk order, then the projection through the normalisation: 16 rows per block, 16 lanes per row -------------
__global__ __launch_bounds__(256) void cl_finish(FinishSide fx, FinishSide fw, int nxblk, const float* __restrict__ pdb,
                                                 float* __restrict__ db, int D, int Dp, int normalise) {
    const int c = threadIdx.x & 15;
    const bool isx = (int)blockIdx.x < nxblk;
    const FinishSide& f = isx ? fx : fw;
    const long long i = ((long long)blockIdx.x - (isx ? 0 : nxblk)) * 16 + (threadIdx.x >> 4);
    if (f.out != nullptr) {  // (the same for every thread of the block)
        float A[NPLDA_MAX_NB];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < NPLDA_MAX_NB; ++k) {
            A[k] = 0.f;
            const int d = c + 16 * k;
            if (d < Dp) {
                for (int ch = 0; ch < f.nch; ++ch) A[k] += f.part[((size_t)ch * f.P + i) * Dp + d];
                dot = fmaf(f.img[(size_t)i * Dp + d], A[k], dot);
            }
        }
        dot = row16_sum(dot);
        if (i < f.n) {
            const float nr = f.nrm[i];
#pragma unroll
            for (int k = 0; k < NPLDA_MAX_NB; ++k) {
                const int d = c + 16 * k;
                if (d < D) f.out[i * f.ld + d] = normalise ? fmaf(-dot, f.img[(size_t)i * Dp + d], A[k]) / nr : A[k];
            }
        }
    }
    if (!isx && db != nullptr && c == 0 && i < fw.n) {
        float acc = 0.f;
        for (int ch = 0; ch < fw.nch; ++ch) acc += pdb[(size_t)ch * fw.P + i];
        db[i] = acc;
    }
}

template <int NB>
void launch_all(const MainArgs& lse, const MainArgs* gx, const MainArgs* gw, dim3 grid_rows, dim3 grid_cls, hipStream_t st,
                int pass) {
    if (pass == 0) hipLaunchKernelGGL((cl_main<NB, true, false>), grid_rows, dim3(256), 0, st, lse);
    if (pass == 1 && gx) hipLaunchKernelGGL((cl_main<NB, true, true>), grid_rows, dim3(256), 0, st, *gx);
    if (pass == 1 && gw) hipLaunchKernelGGL((cl_main<NB, false, true>), grid_cls, dim3(256), 0, st, *gw);
}

void launch_nb(int nb, const MainArgs& lse, const MainArgs* gx, const MainArgs* gw, dim3 grid_rows, dim3 grid_cls,
               hipStream_t st, int pass) {
    switch (nb) {
        case 2: launch_all<2>(lse, gx, gw, grid_rows, grid_cls, st, pass); break;
        case 4: launch_all<4>(lse, gx, gw, grid_rows, grid_cls, st, pass); break;
        case 8: launch_all<8>(lse, gx, gw, grid_rows, grid_cls, st, pass); break;
        case 10: launch_all<10>(lse, gx, gw, grid_rows, grid_cls, st, pass); break;
        case 11: launch_all<11>(lse, gx, gw, grid_rows, grid_cls, st, pass); break;
        default: launch_all<12>(lse, gx, gw, grid_rows, grid_cls, st, pass); break;
    }
}

}  // namespace

extern "C" {

size_t nplda_classify_workspace_bytes(int64_t N, int64_t C, int D, int class_chunks, int row_chunks) {
    if (N < 0 || N > kMaxN || C < 0 || C > kMaxC || D <= 0 || class_chunks < 0 || row_chunks < 0) return 0;
    const int nb = nplda_kernel_nb(D, D);
    if (nb == 0) return 0;
    return ws_layout(N, C, 16 * nb, class_chunks, row_chunks).total;
}

int nplda_classify_loss_f32(const float* X, int64_t ldx, int64_t N, const float* W, int64_t ldw, int64_t C, int D,
                            const float* b, const int32_t* y, int kind, float s, float m, int class_chunks, int row_chunks,
                            float* loss, int64_t* counts, float* rowloss, int32_t* pred, float* dX, int64_t lddx, float* dW,
                            int64_t lddw, float* db, void* ws, size_t ws_bytes, nplda_stream_t stream) {
    if (kind < 0 || kind > 2 || !(s > 0.f) || !(m >= 0.f)) return NPLDA_EINVAL;
    if ((kind == 0 && m != 0.f) || (kind == 2 && !(m < 3.14159265358979323846f))) return NPLDA_EINVAL;
    if (N < 0 || C < 0 || D <= 0 || class_chunks < 0 || row_chunks < 0) return NPLDA_EINVAL;
    if (N == 0 || C == 0) return NPLDA_OK;  // (an empty problem has no pointers to check)
    if (!X || !W || !y || !loss || !counts || !ws) return NPLDA_EINVAL;
    if (ldx < D || (ldx & 3) || ldw < D || (ldw & 3)) return NPLDA_EINVAL;
    if (!nplda_aligned16(X) || !nplda_aligned16(W) || !nplda_aligned16(ws)) return NPLDA_EINVAL;
    if (dX && (lddx < D || (lddx & 3) || !nplda_aligned16(dX))) return NPLDA_EINVAL;
    if (dW && (lddw < D || (lddw & 3) || !nplda_aligned16(dW))) return NPLDA_EINVAL;
    const int nb = nplda_kernel_nb(D, D);
    if (nb == 0 || N > kMaxN || C > kMaxC) return NPLDA_EUNSUPPORTED;
    const int Dp = 16 * nb;
    const WsLayout L = ws_layout(N, C, Dp, class_chunks, row_chunks);
    if (ws_bytes < L.total) return NPLDA_ENOSPC;

    char* w = (char*)ws;
    float* Xp = (float*)(w + L.oX);
    float* Wp = (float*)(w + L.oW);
    float* nx = (float*)(w + L.onx);
    float* nw = (float*)(w + L.onw);
    int* yp = (int*)(w + L.oy);
    float* bp = (float*)(w + L.ob);
    float* lse = (float*)(w + L.olse);
    float* lpart = (float*)(w + L.olp);
    double* bsum = (double*)(w + L.obs);
    long long* bcnt = (long long*)(w + L.obc);
    long long* cnt = (long long*)(w + L.ocnt);
    float* pA = (float*)(w + L.oA);
    float* pB = (float*)(w + L.oB);
    float* pdb = (float*)(w + L.odb);
    hipStream_t st = (hipStream_t)stream;
    const int normalise = kind != 0;
    const int nxblk = (int)(L.Np / 16), nwblk = (int)(L.Cp / 16);
    const int cw = (int)((C + kWalk - 1) / kWalk), rw = (int)((N + kWalk - 1) / kWalk);
    const Margin mk = {kind, s, m, (float)cos((double)m), (float)sin((double)m), (float)((double)m * sin((double)m))};

    hipLaunchKernelGGL(cl_pad, dim3(nxblk + nwblk), dim3(256), 0, st, X, (long long)ldx, (int)N, W, (long long)ldw, (int)C, D,
                       Dp, normalise, b, (const int*)y, nxblk, Xp, Wp, nx, nw, yp, bp);
    const dim3 grid_rows((unsigned)(L.Np / kOwn), (unsigned)L.cc), grid_cls((unsigned)(L.Cp / kOwn), (unsigned)L.rc);
    const MainArgs a_lse = {Xp, Wp, yp, bp, lse, cnt, (long long)L.Np, (int)C, L.cper, cw, mk, lpart, nullptr};
    launch_nb(nb, a_lse, nullptr, nullptr, grid_rows, grid_cls, st, 0);
    hipLaunchKernelGGL(cl_merge, dim3(L.nmb), dim3(kMergeRows), 0, st, (const float*)lpart, L.cc, (long long)L.Np, L.cper,
                       (const int*)yp, (int)N, (int)C, lse, rowloss, (int*)pred, bsum, bcnt);
    hipLaunchKernelGGL(cl_scalars, dim3(1), dim3(64), 0, st, (const double*)bsum, (const long long*)bcnt, L.nmb, loss,
                       (long long*)counts, cnt);
    const bool want_x = dX != nullptr, want_w = dW != nullptr || db != nullptr;
    if (want_x || want_w) {
        const MainArgs a_gx = {Xp, Wp, yp, bp, lse, cnt, (long long)L.Np, (int)C, L.cper, cw, mk, pA, nullptr};
        const MainArgs a_gw = {Wp, Xp, yp, bp, lse, cnt, (long long)L.Cp, (int)C, L.rper, rw, mk, pB, pdb};
        const FinishSide fx = {pA, Xp, nx, dX, (long long)lddx, (long long)L.Np, (int)N, L.cc};
        const FinishSide fw = {pB, Wp, nw, dW, (long long)lddw, (long long)L.Cp, (int)C, L.rc};
        if (want_x) {
            launch_nb(nb, a_lse, &a_gx, nullptr, grid_rows, grid_cls, st, 1);
            hipLaunchKernelGGL(cl_finish, dim3(nxblk), dim3(256), 0, st, fx, fw, nxblk, (const float*)pdb, db, D, Dp, normalise);
        }
        if (want_w) {
            launch_nb(nb, a_lse, nullptr, &a_gw, grid_rows, grid_cls, st, 1);
            hipLaunchKernelGGL(cl_finish, dim3(nwblk), dim3(256), 0, st, fx, fw, 0, (const float*)pdb, db, D, Dp, normalise);
        }
    }
    return nplda_launch_status();
}

}  // extern "C"
