// nplda_topk.hip — the k best-scoring rows of an embedding table for every probe row, with their indices (gfx950).
//
// 1:N identification and hard-trial mining: s_rj = q_r + q_j + 2 sum_d P_d z_rd z_jd (utils/models.py:372-376) of R probe
// rows against the M rows of a table, under an eligibility mask given by labels, groups and "this row IS table row j",
// reduced to the k largest (or smallest) scores per row, sorted, ties by ascending column.  The R x M matrix is never
// written.  design/k19_topk_search.md has the semantics, the tile shape and the budget.
//
// Two launches.  topk_main: a block owns 64 rows (four waves of 16) and a CHUNK of the table's 16-column tiles; it forms
// 16 x 16 pieces of S^T on fp32-input MFMAs exactly as ap_main does (A operand z_j, B operand P o z_r, two accumulator
// chains over even and odd 16-blocks of features, so a score's bits depend on (row, column, model) only), turns every
// eligible score into a 64-bit COMPOSITE (order-preserving key of the score << 32 | ~column: larger is better, unique per
// column) and appends the composites that beat the row's current k-th best to the row's candidate list in LDS; a full list
// is sorted by its wave and cut to the best k, which raises the threshold.  The block leaves k composites per (row, chunk)
// in the workspace.  topk_merge: one block per row folds the row's chunk lists the same way and decodes (score, index).
// The composites are totally ordered, so the result is that of a stable sort of the row whatever the chunking.  No
// atomics, no memset, no hand-off inside a launch: every workspace word that is read was written by topk_main of this call.
#include <cstdlib>

#include "nplda_cohort_common.h"

namespace {

typedef unsigned long long u64;

constexpr int kRowTile = 64;           // rows per block
constexpr int kColTile = 16;           // table rows per LDS stage
constexpr int kMaxK = 128;             // NPLDA_TOPK_MAX_K
constexpr int kTargetBlocks = 768;     // three resident blocks on each of 256 CUs: what registers and LDS admit at k <= 16;
constexpr int kTargetBlocksBigK = 512; // above that the candidate lists leave room for two (k <= 64) or one
constexpr int kMinTilesPerChunk = 4;   // a chunk is at least 64 table rows
constexpr int kMergeCap = 256;         // candidate slots of the merge: k + one slab of 64
constexpr int kMergeLoads = 8;         // composites a lane of the merge fetches before it filters them
constexpr int kMaxDev = 64;
constexpr long long kMaxR = (1ll << 24) - 1;  // the merge is one block of 256 threads per row: a grid below 2^32 threads

static_assert(kMaxK == NPLDA_TOPK_MAX_K, "the header states the largest k");
static_assert(kMergeCap >= kMaxK + 64, "a slab of 64 must fit behind the kept k");

struct TopkPlan {
    long long nrt, ntiles, tiles_per_chunk;
    int chunks;
    size_t ws_bytes;
};

// The chunk count: as many as fill the chip once with this call's row tiles, at least kMinTilesPerChunk tiles each.
// NPLDA_TOPK_MAX_CHUNKS can only LOWER the cap (fewer, longer chunks) — for A/B runs and for tests that want one chunk and
// several at a few thousand columns.  Read per call by the sizing function and the launch alike, so the two always agree.
// ws_bytes is an upper bound of rows x chunks lists that never decreases with R, M or k (the exact product does, where the
// floor of kTargetBlocks / nrt steps down).
TopkPlan topk_plan(int64_t R, int64_t M, int k) {
    TopkPlan p;
    p.nrt = (R + kRowTile - 1) / kRowTile;
    p.ntiles = (M + kColTile - 1) / kColTile;
    const long long nrt = p.nrt < 1 ? 1 : p.nrt;
    long long cap = kTargetBlocks;
    if (const char* e = getenv("NPLDA_TOPK_MAX_CHUNKS")) {
        const long long want = atoll(e);
        if (want >= 1 && want < cap) cap = want;
    }
    long long maxc = (k <= 16 ? kTargetBlocks : kTargetBlocksBigK) / nrt;
    if (maxc > cap) maxc = cap;
    if (maxc < 1) maxc = 1;
    long long bylen = p.ntiles / kMinTilesPerChunk;
    if (bylen < 1) bylen = 1;
    long long chunks = maxc < bylen ? maxc : bylen;
    p.tiles_per_chunk = (p.ntiles + chunks - 1) / chunks;
    if (p.tiles_per_chunk < 1) p.tiles_per_chunk = 1;
    chunks = (p.ntiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;
    p.chunks = (int)(chunks < 1 ? 1 : chunks);
    // nrt * chunks <= max(nrt, min(kTargetBlocks, nrt * cap, nrt * bylen)), with the larger target whatever k: monotone in k
    long long blocks = kTargetBlocks;
    if (nrt * cap < blocks) blocks = nrt * cap;
    if (nrt * bylen < blocks) blocks = nrt * bylen;
    if (blocks < nrt) blocks = nrt;
    p.ws_bytes = up256((size_t)blocks * kRowTile * (size_t)k * sizeof(u64));
    return p;
}

// LDS traffic between the lanes of ONE wave: a wave's DS instructions execute in order, so a later read sees an earlier write
// of another lane once the compiler keeps the two apart.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Sort buf[0 .. CAP) (n live composites, the rest cleared to 0 = "no candidate") best first, by the calling wave; returns the
// number kept and sets thr to the k-th best (0 while fewer than k are known: everything eligible passes).
template <int CAP>
__device__ __forceinline__ int wave_compact(u64* buf, int n, int k, int lane, u64& thr) {
    wave_lds_sync();
    for (int t = lane; t < CAP; t += 64)
        if (t >= n) buf[t] = 0;
    wave_lds_sync();
    for (int size = 2; size <= CAP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < CAP / 2; t += 64) {
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const u64 a = buf[lo], b = buf[hi];
                if ((a < b) == desc) {
                    buf[lo] = b;
                    buf[hi] = a;
                }
            }
            wave_lds_sync();
        }
    }
    thr = n >= k ? buf[k - 1] : 0;
    return n < k ? n : k;
}

struct TopkArgs {
    const float *z_rows, *q_rows, *z_tab, *q_tab, *P;
    long long R, M, ldz, tiles_per_chunk, ntiles;
    int chunks, k, largest, mask_mode;
    const int *lab_rows, *lab_tab, *grp_rows, *grp_tab;
    const long long* self_rows;
    u64* lists;  // [R][chunks][k]
};

template <int NB, int KC>
__global__ __launch_bounds__(256, KC > 64 ? 1 : 2) void topk_main(const TopkArgs a) {
    constexpr int Dp = 16 * NB;
    constexpr int LD = Dp + 4;   // LDS row stride: conflict-free b128 reads of 16 rows (as ap_main)
    constexpr int CAP = 2 * KC;  // candidate slots per row: the kept k and at least 16 new ones
    constexpr int NST = (kColTile * Dp / 4 + 255) / 256;
    static_assert(KC >= kColTile, "a tile's 16 scores must fit behind the kept k");
    __shared__ __attribute__((aligned(16))) float zs[kColTile * LD];
    __shared__ __attribute__((aligned(16))) float qs[kColTile];
    __shared__ __attribute__((aligned(16))) int ls[kColTile], gs[kColTile];
    extern __shared__ __attribute__((aligned(16))) u64 cand[];  // [kRowTile][CAP]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int ch = (int)(blockIdx.x % (unsigned)a.chunks);
    const long long row0 = (long long)(blockIdx.x / (unsigned)a.chunks) * kRowTile + 16 * wave;
    const bool wave_on = row0 < a.R;  // a wave without a row stages and waits with the others, nothing else
    const long long i = row0 + c;
    const bool row_ok = i < a.R;
    const long long ic = row_ok ? i : a.R - 1;  // (clamped: rows beyond R are read nowhere and emit nothing)
    const bool has_grp = a.grp_rows != nullptr;

    f32x4 pz[NB];
    {
        const float* zi = a.z_rows + ic * a.ldz + 4 * g;
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) pz[qb] = *(const f32x4*)(zi + 16 * qb) * *(const f32x4*)(a.P + 16 * qb + 4 * g);
    }
    const float qi = a.q_rows[ic];
    const int li = a.mask_mode ? a.lab_rows[ic] : 0;
    const int gi = has_grp ? a.grp_rows[ic] : 0;
    const long long si = a.self_rows ? a.self_rows[ic] : -1;

    u64* mine = cand + (size_t)(16 * wave + c) * CAP;
    u64 thr = 0;
    int cnt = 0;
    const u64 rowmask = 0x0001000100010001ull << c;  // the four lanes that hold row c
    const u64 below = rowmask & ((1ull << (16 * g)) - 1ull);

    const long long tbeg = (long long)ch * a.tiles_per_chunk;
    const long long tend = tbeg + a.tiles_per_chunk < a.ntiles ? tbeg + a.tiles_per_chunk : a.ntiles;
    f32x4 st[NST];
    float pq = 0.f;
    int pl = 0, pg = 0;
    auto fetch = [&](long long j0) {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kColTile * Dp / 4) {
                long long jr = j0 + e / (4 * NB);
                jr = jr < a.M ? jr : a.M - 1;  // (clamped: buffer rows beyond M are never read)
                st[u] = *(const f32x4*)(a.z_tab + jr * a.ldz + 4 * (e % (4 * NB)));
            }
        }
        if (threadIdx.x < kColTile) {
            long long jr = j0 + threadIdx.x;
            jr = jr < a.M ? jr : a.M - 1;
            pq = a.q_tab[jr];
            pl = a.mask_mode ? a.lab_tab[jr] : 0;
            pg = has_grp ? a.grp_tab[jr] : 0;
        }
    };
    if (tbeg < tend) fetch(tbeg * kColTile);
    for (long long t = tbeg; t < tend; ++t) {
        const long long j0 = t * kColTile;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kColTile * Dp / 4) *(f32x4*)(zs + (e / (4 * NB)) * LD + 4 * (e % (4 * NB))) = st[u];
        }
        if (threadIdx.x < kColTile) {
            qs[threadIdx.x] = pq;
            ls[threadIdx.x] = pl;
            gs[threadIdx.x] = pg;
        }
        __syncthreads();
        if (t + 1 < tend) fetch(j0 + kColTile);
        if (!wave_on) continue;

        // S^T piece: table rows j = 4 g + r in register r, probe row c on the lane; the feature sum as ap_main's two chains
        f32x4 S0 = f32x4{0.f, 0.f, 0.f, 0.f}, S1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            const f32x4 av = *(const f32x4*)(zs + c * LD + 16 * qb + 4 * g);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (qb & 1) S1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], pz[qb][m], S1, 0, 0, 0);
                else S0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], pz[qb][m], S0, 0, 0, 0);
            }
        }
        const f32x4 S = S0 + S1;
        const f32x4 qj = *(const f32x4*)(qs + 4 * g);
        const int4 lj = *(const int4*)(ls + 4 * g);
        const int4 gj = *(const int4*)(gs + 4 * g);
        const int l4[4] = {lj.x, lj.y, lj.z, lj.w}, g4[4] = {gj.x, gj.y, gj.z, gj.w};
        u64 comp[4], m4[4];
        bool pass[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long j = j0 + 4 * g + r;
            bool ok = row_ok & (j < a.M) & (j != si) & (!has_grp | (g4[r] == gi));
            if (a.mask_mode == 1) ok &= l4[r] != li;
            if (a.mask_mode == 2) ok &= l4[r] == li;
            unsigned sb = __float_as_uint(fmaf(2.0f, S[r], qi + qj[r]));
            if ((sb << 1) == 0u) sb = 0u;  // -0.0f counts as +0.0f
            unsigned key = f2key(__uint_as_float(sb));
            if (!a.largest) key = ~key;
            comp[r] = ok ? ((u64)key << 32) | (u64)(~(unsigned)j) : 0ull;
            pass[r] = comp[r] > thr;
            m4[r] = __ballot(pass[r]);
        }
        if ((m4[0] | m4[1] | m4[2] | m4[3]) == 0ull) continue;
        int tot = 0, off = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            tot += __popcll(m4[r] & rowmask);
            off += __popcll(m4[r] & below);
        }
        u64 need = __ballot(g == 0 && cnt + tot > CAP);
        while (need) {  // wave-uniform: the rows whose list would overflow are cut to their best k first
            const int rr = __ffsll((long long)need) - 1;
            need &= need - 1;
            const int n = __shfl(cnt, rr, 64);
            u64 nthr;
            const int kept = wave_compact<CAP>(cand + (size_t)(16 * wave + rr) * CAP, n, a.k, lane, nthr);
            if (c == rr) {
                cnt = kept;
                thr = nthr;
            }
        }
        int pos = cnt + off;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (pass[r]) mine[pos++] = comp[r];
        cnt += tot;
    }

    if (!wave_on) return;
    for (int rr = 0; rr < 16; ++rr) {
        if (row0 + rr >= a.R) break;
        const int n = __shfl(cnt, rr, 64);
        u64* buf = cand + (size_t)(16 * wave + rr) * CAP;
        u64 nthr;
        wave_compact<CAP>(buf, n, a.k, lane, nthr);
        u64* dst = a.lists + ((size_t)(row0 + rr) * a.chunks + ch) * a.k;
        for (int t = lane; t < a.k; t += 64) dst[t] = buf[t];  // (slots past the kept ones sorted to 0)
    }
}

// One block of four waves per row: the row's chunk lists (k composites each, 0 where a chunk had fewer than k) -> the best k,
// decoded.  Each wave folds a quarter of the lists into a candidate list of its own, wave 0 then folds the other three in:
// a single probe against 1.2 M rows leaves several hundred lists to this one block.
__global__ __launch_bounds__(256) void topk_merge(const u64* __restrict__ lists, int nlists, int k, int largest,
                                                  float* __restrict__ vals, long long* __restrict__ idx) {
    __shared__ u64 bufs[4][kMergeCap];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* buf = bufs[wave];
    const u64 lower = (1ull << lane) - 1ull;
    u64 thr = 0;
    int cnt = 0;
    auto push = [&](u64 v) {  // one composite per lane, wave-uniform control flow
        const bool pass = v > thr;
        const u64 m = __ballot(pass);
        if (m == 0ull) return;
        const int tot = __popcll(m);
        if (cnt + tot > kMergeCap) cnt = wave_compact<kMergeCap>(buf, cnt, k, lane, thr);
        if (pass) buf[cnt + __popcll(m & lower)] = v;
        cnt += tot;
    };
    const int per = (nlists + 3) / 4;
    const long long e0 = (long long)(wave * per < nlists ? wave * per : nlists) * k;
    const long long e1 = (long long)((wave + 1) * per < nlists ? (wave + 1) * per : nlists) * k;
    const u64* src = lists + (size_t)blockIdx.x * nlists * k;
    for (long long base = e0; base < e1; base += 64 * kMergeLoads) {
        u64 v[kMergeLoads];
#pragma unroll
        for (int u = 0; u < kMergeLoads; ++u) {
            const long long e = base + 64 * u + lane;
            v[u] = e < e1 ? src[e] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kMergeLoads; ++u) push(v[u]);
    }
    cnt = wave_compact<kMergeCap>(buf, cnt, k, lane, thr);
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w)
        for (int t0 = 0; t0 < k; t0 += 64) push(t0 + lane < k ? bufs[w][t0 + lane] : 0ull);
    wave_compact<kMergeCap>(buf, cnt, k, lane, thr);
    for (int t = lane; t < k; t += 64) {
        const u64 w = buf[t];
        unsigned key = (unsigned)(w >> 32);
        if (!largest) key = ~key;
        const size_t o = (size_t)blockIdx.x * k + t;
        vals[o] = w ? key2f(key) : (largest ? -__builtin_inff() : __builtin_inff());
        idx[o] = w ? (long long)(~(unsigned)w) : -1ll;
    }
}

template <int NB, int KC>
int launch_main(const TopkArgs& a, unsigned grid, hipStream_t st) {
    constexpr size_t lds = (size_t)kRowTile * 2 * KC * sizeof(u64);
    // the candidate lists of KC = 64 and 128 go past the 64 KB a launch may take without asking; asked once per device
    static unsigned char asked[kMaxDev];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) dev = kMaxDev - 1;
    if (!asked[dev] || dev == kMaxDev - 1) {
        const hipError_t e =
            hipFuncSetAttribute((const void*)topk_main<NB, KC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        asked[dev] = 1;
    }
    hipLaunchKernelGGL((topk_main<NB, KC>), dim3(grid), dim3(256), lds, st, a);
    return NPLDA_OK;
}

template <int NB>
int launch_main_kc(int k, const TopkArgs& a, unsigned grid, hipStream_t st) {
    if (k <= 16) return launch_main<NB, 16>(a, grid, st);
    if (k <= 64) return launch_main<NB, 64>(a, grid, st);
    return launch_main<NB, 128>(a, grid, st);
}

}  // namespace

extern "C" {

size_t nplda_topk_workspace_bytes(int64_t R, int64_t M, int D2, int k) {
    if (R < 0 || M < 0 || R > kMaxR || M > 0x7fffffffLL || D2 <= 0 || k < 1 || k > kMaxK) return 0;
    if (nplda_kernel_nb(D2, D2) == 0) return 0;
    return topk_plan(R, M, k).ws_bytes;
}

int nplda_topk_scores_f32(const float* z_rows, const float* q_rows, int64_t R, const float* z_tab, const float* q_tab,
                          int64_t M, int64_t ldz, const void* packed, int D0, int D1, int D2, int k, int largest,
                          int mask_mode, const int32_t* lab_rows, const int32_t* lab_tab, const int32_t* grp_rows,
                          const int32_t* grp_tab, const int64_t* self_rows, float* vals, int64_t* idx, void* ws,
                          size_t ws_bytes, nplda_stream_t stream) {
    if (R < 0 || M < 0 || D0 <= 0 || D1 <= 0 || D2 <= 0 || k < 1 || k > kMaxK) return NPLDA_EINVAL;
    if (mask_mode < 0 || mask_mode > 2 || (largest != 0 && largest != 1)) return NPLDA_EINVAL;
    if (R == 0) return NPLDA_OK;  // (no row, no pointer to check)
    if (!vals || !idx || !ws || !nplda_aligned16(ws)) return NPLDA_EINVAL;
    if (mask_mode != 0 && (!lab_rows || !lab_tab)) return NPLDA_EINVAL;
    if ((grp_rows == nullptr) != (grp_tab == nullptr)) return NPLDA_EINVAL;
    if (M > 0 && (!z_rows || !q_rows || !z_tab || !q_tab || !packed)) return NPLDA_EINVAL;
    if (!nplda_dims_ok(D0, D1, D2)) return (D0 % 4) ? NPLDA_EINVAL : NPLDA_EUNSUPPORTED;
    const NpldaLayout L = nplda_layout(D0, D1, D2);
    const int Dp = 16 * L.NB;
    if (M > 0 && (ldz < Dp || (ldz & 3) || !nplda_aligned16(z_rows) || !nplda_aligned16(z_tab) || !nplda_aligned16(packed)))
        return NPLDA_EINVAL;
    if (R > kMaxR || M > 0x7fffffffLL) return NPLDA_EUNSUPPORTED;
    const TopkPlan p = topk_plan(R, M, k);
    if (ws_bytes < p.ws_bytes) return NPLDA_ENOSPC;
    if (p.nrt * p.chunks > kMaxR) return NPLDA_EUNSUPPORTED;  // (cannot happen: nrt <= 2^18, or chunks = 1)

    hipStream_t st = (hipStream_t)stream;
    u64* lists = (u64*)ws;
    if (M > 0) {
        TopkArgs a = {z_rows, q_rows, z_tab, q_tab, (const float*)packed + L.oP,
                      (long long)R, (long long)M, (long long)ldz, p.tiles_per_chunk, p.ntiles,
                      p.chunks, k, largest, mask_mode,
                      (const int*)lab_rows, (const int*)lab_tab, (const int*)grp_rows, (const int*)grp_tab,
                      (const long long*)self_rows, lists};
        const unsigned grid = (unsigned)(p.nrt * p.chunks);
        int rc;
        switch (L.NB) {
            case 2: rc = launch_main_kc<2>(k, a, grid, st); break;
            case 4: rc = launch_main_kc<4>(k, a, grid, st); break;
            case 8: rc = launch_main_kc<8>(k, a, grid, st); break;
            case 10: rc = launch_main_kc<10>(k, a, grid, st); break;
            case 11: rc = launch_main_kc<11>(k, a, grid, st); break;
            default: rc = launch_main_kc<12>(k, a, grid, st); break;
        }
        if (rc != NPLDA_OK) return rc;
    }
    hipLaunchKernelGGL(topk_merge, dim3((unsigned)R), dim3(256), 0, st, (const u64*)lists, M > 0 ? p.chunks : 0, k, largest,
                       vals, (long long*)idx);
    return nplda_launch_status();
}

}  // extern "C"
