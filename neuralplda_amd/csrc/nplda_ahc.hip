// nplda_ahc.hip — the dense score matrix of a set against itself and its agglomerative clustering, P ragged problems per
// call (gfx950).  design/k21_ahc.md has the semantics, the kernel shapes and the budget.
//
// score_matrix_kernel: the staging / MFMA loop of topk_main (csrc/nplda_topk.hip) with a store epilogue.  A block owns 64 rows
// of one problem (four waves of 16) and a chunk of 16 of its 16-column tiles; only 16 x 16 pieces that hold some i < j are
// formed, the lower index on the row operand, so a score's bits are those of ops.topk_scores for (row i, column j); the
// piece goes to (i, j) and, from the same registers, to (j, i); the diagonal is +0.0f.
//
// ahc_kernel: ONE workgroup per problem.  The upper triangle becomes a symmetric fp64 matrix of linkage numerators in the
// workspace (sums for average linkage, min / max otherwise) with a per-cluster cache of (best higher-indexed partner,
// value); a merge is a block-wide argmax over the cache, one pass that updates row and column a and patches the caches
// it can, a re-scan of the rows whose cached partner was a or b, and the record store.  __syncthreads() only: no
// cross-block hand-off, no atomics on floating-point data, no memset, nothing read back.
#include <cmath>

#include "nplda_cohort_common.h"
#include "nplda_ragged.h"

namespace {

constexpr int kRowTile = 64;        // rows per block of the score kernel
constexpr int kColTile = 16;        // columns per LDS stage
constexpr int kChunkTiles = 16;     // column tiles per block: 256 columns
constexpr int kAhcBlock = 1024;     // threads of the clustering block
constexpr int kAhcWaves = kAhcBlock / 64;
constexpr int kAhcMaxN = 16384;     // 8 n^2 bytes of fp64 numerators per problem: 2 GiB
constexpr long long kMaxP = (1ll << 22) - 1;  // a grid of P blocks of 1024 threads stays below 2^32 threads
constexpr int kBlockScanRows = 8;   // a merge of a problem above kSmallN rows with up to this many rows to scan again has
constexpr int kSmallN = 2048;       // the whole block scan each; any other merge gives every such row to one wave

// ---- the ragged layout (csrc/nplda_ragged.h) ------------------------------------------------------------------------------------

// what a problem of n rows takes: n^2 matrix elements, max(n - 1, 0) merge records, and in the workspace n^2 fp64 numerators
// with five words per row (cache value 8, partner, size, rep, todo 4 each)
enum { kElems, kRecords, kWsBytes, kTerms };
struct AhcTerms {
    __host__ __device__ void operator()(long long n, long long, long long* t) const {
        t[kElems] = n * n;
        t[kRecords] = n > 1 ? n - 1 : 0;
        t[kWsBytes] = 8 * n * n + 24 * n;
    }
};

struct RaggedPlan {
    int status;
    long long rows, max_n, elems, records;  // table rows, largest problem, sum n^2, sum max(n - 1, 0)
    size_t ws_bytes;
};

RaggedPlan ragged_plan(const int64_t* offs, int64_t P) {
    RaggedPlan r = {NPLDA_OK, 0, 0, 0, 0, 0};
    long long ws = 0;
    r.status = ragged_walk(offs, offs, P, kMaxP, [&](long long n, long long) {
        if (n > kAhcMaxN) return NPLDA_EUNSUPPORTED;
        long long t[kTerms];
        AhcTerms()(n, n, t);
        if (n > r.max_n) r.max_n = n;
        r.elems += t[kElems];
        r.records += t[kRecords];
        ws += t[kWsBytes];
        return NPLDA_OK;
    });
    if (r.status == NPLDA_OK && P > 0) r.rows = offs[P];
    r.ws_bytes = up256((size_t)ws) + 256;
    return r;
}

// blocks of the score kernel a problem of n rows needs: row tile I (64 rows) meets the 256-column chunks I / 4 .. C - 1
inline long long score_blocks(long long n) {
    const long long T = (n + kRowTile - 1) / kRowTile, C = (n + kColTile * kChunkTiles - 1) / (kColTile * kChunkTiles);
    long long b = 0;
    for (long long I = 0; I < T; ++I) b += C - I / 4;
    return b;
}

// ---- device: where problem p starts -----------------------------------------------------------------------------------------

struct Starts {
    long long row0, n, elem0, rec0, ws0;  // first table row, rows, first matrix element, first merge record, workspace byte
};

__device__ __forceinline__ Starts problem_starts(const long long* __restrict__ offs, long long p, long long* red /* [3 * 16] */) {
    long long sum[kTerms];
    ragged_starts(offs, p, AhcTerms(), red, sum);
    Starts s;
    s.elem0 = sum[kElems];
    s.rec0 = sum[kRecords];
    s.ws0 = sum[kWsBytes];
    s.row0 = offs[p];
    s.n = offs[p + 1] - s.row0;
    return s;
}

// ---- the score matrix ---------------------------------------------------------------------------------------------------------

struct ScoreArgs {
    const float *z, *q, *P;
    const long long* offs;
    long long ldz;
    float* out;
};

template <int NB>
__global__ __launch_bounds__(256, 2) void score_matrix_kernel(const ScoreArgs a) {
    constexpr int Dp = 16 * NB;
    constexpr int LD = Dp + 4;  // LDS row stride: conflict-free b128 reads of 16 rows (as topk_main)
    constexpr int NST = (kColTile * Dp / 4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float zs[kColTile * LD];
    __shared__ __attribute__((aligned(16))) float qs[kColTile];
    __shared__ long long red[48];

    // which (row tile, column chunk) of the problem this block is; a block past the problem's count has nothing to do
    const long long n = a.offs[blockIdx.x + 1] - a.offs[blockIdx.x];
    const int T = (int)((n + kRowTile - 1) / kRowTile), C = (int)((n + kColTile * kChunkTiles - 1) / (kColTile * kChunkTiles));
    int I = 0, rest = (int)blockIdx.y;
    while (I < T && rest >= C - I / 4) {  // (at most T <= 256 steps)
        rest -= C - I / 4;
        ++I;
    }
    if (I >= T) return;  // block-uniform
    const int ch = I / 4 + rest;
    const Starts s = problem_starts(a.offs, blockIdx.x, red);
    const float* zp = a.z + s.row0 * a.ldz;
    const float* qp = a.q + s.row0;
    float* out = a.out + s.elem0;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const long long row0 = (long long)I * kRowTile + 16 * wave;
    const bool wave_on = row0 < n;  // a wave without a row stages and waits with the others, nothing else
    const long long i = row0 + c;
    const long long ic = i < n ? i : n - 1;  // (clamped: rows of the next problem are never read)

    f32x4 pz[NB];
    {
        const float* zi = zp + ic * a.ldz + 4 * g;
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) pz[qb] = *(const f32x4*)(zi + 16 * qb) * *(const f32x4*)(a.P + 16 * qb + 4 * g);
    }
    const float qi = qp[ic];

    const long long ntiles = (n + kColTile - 1) / kColTile;
    long long tbeg = (long long)ch * kChunkTiles;
    if (tbeg < 4ll * I) tbeg = 4ll * I;  // tiles left of the block's first row hold no i < j
    const long long tend = (long long)(ch + 1) * kChunkTiles < ntiles ? (long long)(ch + 1) * kChunkTiles : ntiles;
    f32x4 st[NST];
    float pq = 0.f;
    auto fetch = [&](long long j0) {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < kColTile * Dp / 4) {
                long long jr = j0 + e / (4 * NB);
                jr = jr < n ? jr : n - 1;
                st[u] = *(const f32x4*)(zp + jr * a.ldz + 4 * (e % (4 * NB)));
            }
        }
        if (threadIdx.x < kColTile) {
            long long jr = j0 + threadIdx.x;
            jr = jr < n ? jr : n - 1;
            pq = qp[jr];
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
        if (threadIdx.x < kColTile) qs[threadIdx.x] = pq;
        __syncthreads();
        if (t + 1 < tend) fetch(j0 + kColTile);
        if (!wave_on || j0 < row0) continue;  // (wave-uniform) a piece strictly below the diagonal is the mirror of another

        // S^T piece: columns j = j0 + 4 g + r in register r, row c on the lane; the feature sum as topk_main's two chains
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
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long j = j0 + 4 * g + r;
            if (i >= n || j >= n || j < i) continue;
            unsigned sb = __float_as_uint(fmaf(2.0f, S[r], qi + qj[r]));
            if ((sb << 1) == 0u || j == i) sb = 0u;  // -0.0f counts as +0.0f (as topk_main); the diagonal is +0.0f
            const float v = __uint_as_float(sb);
            out[i * n + j] = v;
            if (j != i) out[j * n + i] = v;
        }
    }
}

template <int NB>
void launch_score(const ScoreArgs& a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((score_matrix_kernel<NB>), grid, dim3(256), 0, st, a);
}

// ---- clustering ------------------------------------------------------------------------------------------------------------

struct Merge {  // nplda_ahc_merge
    int a, b;
    double value;
    int size_after, reserved;
};
static_assert(sizeof(Merge) == sizeof(nplda_ahc_merge), "the header states the record");

struct AhcArgs {
    const float* S;
    const long long* offs;
    int linkage, min_clusters;
    double threshold;
    Merge* merges;
    int *n_merges, *n_clusters, *labels;
    char* ws;
};

// the linkage value of two clusters from their numerator: a division for average linkage (an integer product converted
// exactly, a correctly rounded quotient), the numerator itself otherwise
__device__ __forceinline__ double link_value(int linkage, double num, int sa, int sb) {
    return linkage == 0 ? num / (double)((long long)sa * (long long)sb) : num;
}

// The best (value, index) over the whole block, with a payload x that travels with the winner; the same result on every
// thread.  ONE barrier: consecutive calls alternate between two sets of LDS slots (`slot`, block-uniform), so the slots a
// call writes were last read two calls ago, with the barrier of the call in between behind those reads.
struct BlockBest {
    double v[2][kAhcWaves];
    int j[2][kAhcWaves], x[2][kAhcWaves];
};
__device__ __forceinline__ void block_best(BlockBest& sh, int& slot, int lane, int wave, double& v, int& j, int& x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ov = __shfl_xor(v, s, 64);
        const int oj = __shfl_xor(j, s, 64), ox = __shfl_xor(x, s, 64);
        if (before(ov, oj, v, j)) {
            v = ov;
            j = oj;
            x = ox;
        }
    }
    if (lane == 0) {
        sh.v[slot][wave] = v;
        sh.j[slot][wave] = j;
        sh.x[slot][wave] = x;
    }
    __syncthreads();
    v = sh.v[slot][0];
    j = sh.j[slot][0];
    x = sh.x[slot][0];
#pragma unroll
    for (int w = 1; w < kAhcWaves; ++w)
        if (before(sh.v[slot][w], sh.j[slot][w], v, j)) {
            v = sh.v[slot][w];
            j = sh.j[slot][w];
            x = sh.x[slot][w];
        }
    slot ^= 1;
}

// The best partner j > k of live cluster k, by the calling wave: (value, j) into the cache.
__device__ __forceinline__ void scan_row(int linkage, const double* __restrict__ D, const int* __restrict__ size, int n, int k,
                                         int lane, double* bv, int* nb) {
    const int sk = size[k];
    double v = 0.0;
    int bj = kNone;
    const double* row = D + (size_t)k * n;
    for (int j = k + 1 + lane; j < n; j += 64) {
        const int sj = size[j];
        if (sj > 0) {
            const double L = link_value(linkage, row[j], sk, sj);
            if (bj == kNone || L > v) {  // (ascending j on a lane: the first of equal values stays)
                v = L;
                bj = j;
            }
        }
    }
    wave_best(v, bj);
    if (lane == 0) {
        bv[k] = v;
        nb[k] = bj;
    }
}

__global__ __launch_bounds__(kAhcBlock) void ahc_kernel(const AhcArgs a) {
    __shared__ long long red[48];
    __shared__ BlockBest sh;
    __shared__ int todo_n;
    __shared__ int wcount[kAhcWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Starts s = problem_starts(a.offs, blockIdx.x, red);
    const int n = (int)s.n;
    const int linkage = a.linkage;
    int* labels = a.labels + s.row0;
    Merge* rec = a.merges + s.rec0;
    if (n <= 1) {  // nothing to merge, nothing of the workspace is touched
        if (tid == 0) {
            a.n_merges[blockIdx.x] = 0;
            a.n_clusters[blockIdx.x] = n;
            if (n == 1) labels[0] = 0;
        }
        return;
    }
    const float* S = a.S + s.elem0;
    double* D = (double*)(a.ws + s.ws0);  // [n][n] symmetric numerators
    double* bv = D + (size_t)n * n;       // [n] cached best value of row k over partners j > k
    int* nb = (int*)(bv + n);             // [n] that partner (kNone: none, or k is dead)
    int* size = nb + n;                   // [n] members; 0 = absorbed
    int* rep = size + n;                  // [n] the cluster that absorbed k (k itself while it lives)
    int* todo = rep + n;                  // [n] rows to re-scan in this merge; at the end the rank of every root

    // phase 1: the strict upper triangle -> symmetric fp64, and the cache of every row (all sizes are 1)
    for (int k = wave; k < n; k += kAhcWaves) {
        double v = 0.0;
        int bj = kNone;
        for (int j = k + 1 + lane; j < n; j += 64) {
            const double d = (double)S[(size_t)k * n + j];
            D[(size_t)k * n + j] = d;
            D[(size_t)j * n + k] = d;
            if (bj == kNone || d > v) {
                v = d;
                bj = j;
            }
        }
        wave_best(v, bj);
        if (lane == 0) {
            bv[k] = v;
            nb[k] = bj;
            size[k] = 1;
            rep[k] = k;
        }
    }

    // phase 2: merges.  `live`, `done` and `slot` are block-uniform; the loop runs at most n - 1 times by construction.
    int live = n, done = 0, slot = 0;
    const int floor_live = a.min_clusters;
    for (int step = 0; step < n - 1 && live > floor_live; ++step) {
        __syncthreads();  // the caches and numerators of the last merge (or of phase 1) are in place
        double V = 0.0;
        int ca = kNone, cb = kNone;
        for (int k = tid; k < n; k += kAhcBlock) {  // rows ascending on a thread, so the first of equal values stays
            const int j = nb[k];
            if (j != kNone) {
                const double L = bv[k];
                if (ca == kNone || L > V) {
                    V = L;
                    ca = k;
                    cb = j;
                }
            }
        }
        block_best(sh, slot, lane, wave, V, ca, cb);
        if (ca == kNone || V < a.threshold) break;  // block-uniform: every thread reduced the same sixteen entries
        const int sa = size[ca], sb = size[cb], sn = sa + sb;
        if (tid == 0) todo_n = 0;
        __syncthreads();  // everyone holds the sizes of a and b
        if (tid == 0) {
            size[ca] = sn;
            size[cb] = 0;
            nb[cb] = kNone;
            rep[cb] = ca;
            Merge m;
            m.a = ca;
            m.b = cb;
            m.value = V;
            m.size_after = sn;
            m.reserved = 0;
            rec[done] = m;
        }
        // Row and column a take the merged numerators.  Row a's own cache comes out of the same pass (its partners k > a);
        // the cache of a lower row is patched where one comparison suffices, and listed for a scan where its partner is gone.
        const double* Da = D + (size_t)ca * n;
        const double* Db = D + (size_t)cb * n;
        double av = 0.0;
        int aj = kNone, unused = 0;
        for (int k = tid; k < n; k += kAhcBlock) {
            if (k == ca || k == cb) continue;
            const int sk = size[k];
            if (sk == 0) continue;
            const double da = Da[k], db = Db[k];
            const double nw = linkage == 0 ? da + db : linkage == 1 ? (db < da ? db : da) : (db > da ? db : da);
            D[(size_t)ca * n + k] = nw;
            D[(size_t)k * n + ca] = nw;
            const double L = link_value(linkage, nw, sn, sk);
            if (k < ca) {
                const int j = nb[k];
                if (j == ca || j == cb) {
                    todo[atomicAdd(&todo_n, 1)] = k;
                } else if (before(L, ca, bv[k], j)) {
                    bv[k] = L;
                    nb[k] = ca;
                }
            } else {
                if (aj == kNone || L > av) {
                    av = L;
                    aj = k;
                }
                if (k < cb && nb[k] == cb) todo[atomicAdd(&todo_n, 1)] = k;
            }
        }
        block_best(sh, slot, lane, wave, av, aj, unused);  // (its barrier also ends the pass above)
        if (tid == 0) {
            bv[ca] = av;
            nb[ca] = aj;
        }
        const int nt = todo_n;  // at most n - 2: the live rows below b other than a
        if (n > kSmallN && nt <= kBlockScanRows) {
            // few long rows (the usual case of a large problem): the whole block scans each, a thread per partner
            for (int t = 0; t < nt; ++t) {
                const int k = todo[t], sk = size[k];
                const double* row = D + (size_t)k * n;
                double v = 0.0;
                int bj = kNone;
                for (int j = k + 1 + tid; j < n; j += kAhcBlock) {
                    const int sj = size[j];
                    if (sj > 0) {
                        const double L = link_value(linkage, row[j], sk, sj);
                        if (bj == kNone || L > v) {
                            v = L;
                            bj = j;
                        }
                    }
                }
                block_best(sh, slot, lane, wave, v, bj, unused);
                if (tid == 0) {
                    bv[k] = v;
                    nb[k] = bj;
                }
            }
        } else {
            for (int t = wave; t < nt; t += kAhcWaves) scan_row(linkage, D, size, n, todo[t], lane, bv, nb);
        }
        --live;
        ++done;
    }
    __syncthreads();

    // phase 3: records that were not executed, then the dense rank of every row's cluster in order of smallest members
    for (int m = done + tid; m < n - 1; m += kAhcBlock) {
        Merge e;
        e.a = e.b = -1;
        e.value = __builtin_nan("");
        e.size_after = 0;
        e.reserved = 0;
        rec[m] = e;
    }
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += kAhcBlock) {
        const int k = k0 + tid;
        const bool root = k < n && size[k] > 0;
        const unsigned long long bal = __ballot(root);
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int before_me = base, total = 0;
#pragma unroll
        for (int w = 0; w < kAhcWaves; ++w) {
            if (w < wave) before_me += wcount[w];
            total += wcount[w];
        }
        if (root) todo[k] = before_me + __popcll(bal & ((1ull << lane) - 1ull));
        base += total;
        __syncthreads();
    }
    for (int k = tid; k < n; k += kAhcBlock) {
        int r = k;
        for (int hop = 0; hop < n && rep[r] != r; ++hop) r = rep[r];  // rep[r] < r: at most n - 1 hops
        labels[k] = todo[r];
    }
    if (tid == 0) {
        a.n_merges[blockIdx.x] = done;
        a.n_clusters[blockIdx.x] = n - done;
    }
}

}  // namespace

extern "C" {

int nplda_ahc_max_n(void) { return kAhcMaxN; }
int nplda_ahc_block(void) { return kAhcBlock; }
int nplda_ahc_small_n(void) { return kSmallN; }

size_t nplda_score_matrix_bytes(const int64_t* offsets_host, int64_t P) {
    const RaggedPlan r = ragged_plan(offsets_host, P);
    return r.status == NPLDA_OK ? (size_t)r.elems * sizeof(float) : 0;
}

size_t nplda_ahc_workspace_bytes(const int64_t* offsets_host, int64_t P) {
    const RaggedPlan r = ragged_plan(offsets_host, P);
    return r.status == NPLDA_OK ? r.ws_bytes : 0;
}

int nplda_score_matrix_f32(const float* z, int64_t ldz, const float* q, const int64_t* offsets_host, const int64_t* offsets,
                           int64_t P, const void* packed, int D0, int D1, int D2, float* out, nplda_stream_t stream) {
    if (D0 <= 0 || D1 <= 0 || D2 <= 0) return NPLDA_EINVAL;
    const RaggedPlan r = ragged_plan(offsets_host, P);
    if (r.status != NPLDA_OK) return r.status;
    if (!nplda_dims_ok(D0, D1, D2)) return (D0 % 4) ? NPLDA_EINVAL : NPLDA_EUNSUPPORTED;
    if (P == 0 || r.rows == 0) return NPLDA_OK;  // (no row, no pointer to check)
    if (!z || !q || !offsets || !packed || !out) return NPLDA_EINVAL;
    const NpldaLayout L = nplda_layout(D0, D1, D2);
    if (ldz < 16 * L.NB || (ldz & 3) || !nplda_aligned16(z) || !nplda_aligned16(packed)) return NPLDA_EINVAL;
    ScoreArgs a = {z, q, (const float*)packed + L.oP, (const long long*)offsets, (long long)ldz, out};
    const dim3 grid((unsigned)P, (unsigned)score_blocks(r.max_n));
    hipStream_t st = (hipStream_t)stream;
    switch (L.NB) {
        case 2: launch_score<2>(a, grid, st); break;
        case 4: launch_score<4>(a, grid, st); break;
        case 8: launch_score<8>(a, grid, st); break;
        case 10: launch_score<10>(a, grid, st); break;
        case 11: launch_score<11>(a, grid, st); break;
        default: launch_score<12>(a, grid, st); break;
    }
    return nplda_launch_status();
}

int nplda_ahc_f32(const float* S, const int64_t* offsets_host, const int64_t* offsets, int64_t P, int linkage, double threshold,
                  int min_clusters, nplda_ahc_merge* merges, int32_t* n_merges, int32_t* n_clusters, int32_t* labels, void* ws,
                  size_t ws_bytes, nplda_stream_t stream) {
    if (linkage < 0 || linkage > 2 || min_clusters < 1 || std::isnan(threshold)) return NPLDA_EINVAL;
    const RaggedPlan r = ragged_plan(offsets_host, P);
    if (r.status != NPLDA_OK) return r.status;
    if (P == 0) return NPLDA_OK;
    if (!offsets || !n_merges || !n_clusters) return NPLDA_EINVAL;
    if (r.rows > 0 && !labels) return NPLDA_EINVAL;
    if (r.records > 0 && (!S || !merges || !ws || !nplda_aligned16(ws) || (((uintptr_t)merges) & 7u))) return NPLDA_EINVAL;
    if (r.records > 0 && ws_bytes < r.ws_bytes) return NPLDA_ENOSPC;
    AhcArgs a = {S, (const long long*)offsets, linkage, min_clusters, threshold, (Merge*)merges,
                 (int*)n_merges, (int*)n_clusters, (int*)labels, (char*)ws};
    hipLaunchKernelGGL(ahc_kernel, dim3((unsigned)P), dim3(kAhcBlock), 0, (hipStream_t)stream, a);
    return nplda_launch_status();
}

}  // extern "C"
