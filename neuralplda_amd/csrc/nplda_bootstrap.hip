// Group bootstrap of the detection metrics on gfx950 (design/k20_bootstrap.md): B resamplings of the groups of both
// trial sides, every replicate an integer re-weighting of ONE sorted trial list — N x B weighted updates, not B sorts.
// Stages, all enqueued on one stream with no read-back (the launch count depends on N, B, G1, G2 only):
//   prep     scores -> sort keys (a NaN score gets the key -inf and is dead), the identity permutation
//   sort     radix sort of the (key, index) pairs                                                   [trials::sort_pairs]
//   gather   label code (the classes of nplda_trials.h), tie-run start flag, g1, g2 and (is_llr) the Cllr term of every trial, in sorted order
// then per tile of kTile = 64 replicates (row 0, the point estimate, is replicate 0 of tile 0 with all counts 1):
//   draw     the multinomial draw counts of both sides by integer atomics into a [group][replicate in tile] table
//   pack     the counts as saturating bytes: one trial's look-up is 64 consecutive bytes across a wave
//   pass 1   a wave walks a run of kRun sorted positions, lane = replicate: weighted class counts, the last position
//            with a positive weight and (is_llr) misses / false alarms at the Bayes thresholds and the two Cllr sums
//   reduce   per replicate over the runs in a fixed order, in two levels (chunks of 64 runs, then the chunks); the class
//            counts become exclusive prefixes (inside the chunk + of the chunks)
//   pass 2   the same walk from the run's prefix: K un-normalised costs at tie-run starts (minimum), the first
//            position with P_miss >= P_fa
//   reduce   minimum over the runs
//   finish   a wave per replicate: the +inf threshold, one division per cost, the EER interpolation (binary search
//            for the previous distinct threshold and a partial walk of its run), act_cost, Cllr, the totals
// Weighted counts are integers below 2^53 carried in fp64 (exact; one instruction per add, and the form pass 2 needs).
#include <hip/hip_runtime.h>

#include <cmath>

#include "nplda_trials.h"

namespace {

constexpr int kMaxBeta = 8;
constexpr int kRun = 512;   // sorted positions per wave-run
constexpr int kTile = 64;   // replicates per tile: one per lane
constexpr int kRedWaves = 16;
constexpr int kChunkRuns = 64;  // runs one block of the first reduction level combines
constexpr int kMaxQ = 3 + 2 * kMaxBeta + 2 + kMaxBeta + 3;  // quantities per (run, replicate), both passes
constexpr long long kMaxN = 0x7fffffffll;
constexpr long long kMaxG = 1ll << 20;
constexpr int kMaxB = 1 << 20;
constexpr unsigned long long kGold = 0x9e3779b97f4a7c15ull;

enum { OP_SUM = 0, OP_SCAN = 1, OP_MAX = 2, OP_MIN = 3 };
enum { CODE_NON = 0, CODE_TGT = 1, CODE_IGNORED = 2, CODE_DEAD = 3, FLAG_START = 4 };
static_assert((int)CODE_NON == (int)trials::kNonTarget && (int)CODE_TGT == (int)trials::kTarget,
              "a class code is trials::label_class's value");

__host__ __device__ inline unsigned long long mix(unsigned long long x) {  // the splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ s, long long n, float* __restrict__ key,
                                                   unsigned* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = s[i];
    key[i] = v != v ? -INFINITY : v;
    idx[i] = (unsigned)i;
}

struct GatherArgs {
    const float* scores;
    const float* target;
    const int* g1;
    const int* g2;
    const float* key;
    const unsigned* idx;
    long long n;
    int G1, G2, llr;
    unsigned char* fl;
    int* g1s;
    int* g2s;
    double* sp;
    unsigned long long* flags;
};

__global__ __launch_bounds__(256) void gather_kernel(const GatherArgs a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;
    const unsigned i = a.idx[p];
    const float s = a.scores[i], t = a.target[i];
    const int cls = trials::label_class(t);
    int code = s != s ? CODE_DEAD : (cls == trials::kNeither ? CODE_IGNORED : cls);
    int ga = a.g1[i], gb = a.g2 ? a.g2[i] : 0;
    if (ga < 0 || ga >= a.G1 || (a.g2 && (gb < 0 || gb >= a.G2))) {  // never used as a table index
        code = CODE_DEAD;
        ga = gb = 0;
        atomicAdd(&a.flags[0], 1ull);
    }
    const float k = a.key[p];
    const int start = (p == 0 || a.key[p - 1] != k) ? FLAG_START : 0;
    a.fl[p] = (unsigned char)(code | start);
    a.g1s[p] = ga;
    if (a.g2) a.g2s[p] = gb;
    if (a.llr) {
        const double v = (double)s;
        a.sp[p] = code <= CODE_TGT ? log1p(exp(-fabs(v))) + fmax(code == CODE_TGT ? -v : v, 0.0) : 0.0;
    }
}

// tab32[(side offset + group) * 64 + replicate in tile] += 1 for every draw of replicates 1 .. B of this tile
__global__ __launch_bounds__(256) void draw_kernel(unsigned* __restrict__ tab32, long long G1, long long G2,
                                                   unsigned long long seed, int tile, int B) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (G1 + G2) * kTile) return;
    const int bl = (int)(t & (kTile - 1));
    const long long e = t >> 6;
    const int side = e >= G1;
    const unsigned long long j = (unsigned long long)(side ? e - G1 : e), G = (unsigned long long)(side ? G2 : G1);
    const long long b = (long long)tile * kTile + bl;
    if (b < 1 || b > B) return;
    const unsigned long long key = mix(seed + kGold * (2ull * (unsigned long long)b + side + 1ull));
    const unsigned long long g = ((mix(key + kGold * (j + 1ull)) >> 32) * G) >> 32;
    atomicAdd(&tab32[((side ? G1 : 0) + (long long)g) * kTile + bl], 1u);
}

__global__ __launch_bounds__(256) void pack_kernel(const unsigned* __restrict__ tab32, unsigned char* __restrict__ tab8,
                                                   long long total, int tile, unsigned long long* __restrict__ flags) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    unsigned v = (tile == 0 && (t & (kTile - 1)) == 0) ? 1u : tab32[t];  // replicate 0: the point estimate
    if (v > 255u) {
        v = 255u;
        atomicAdd(&flags[1], 1ull);
    }
    tab8[t] = (unsigned char)v;
}

struct WalkArgs {
    const float* key;
    const unsigned char* fl;
    const int* g1s;
    const int* g2s;
    const double* sp;
    const unsigned char* tab1;
    const unsigned char* tab2;
    double* part;  // [quantity][run][replicate in tile]
    double* ctot;  // [quantity][chunk of runs][replicate in tile]
    double* tot;   // [quantity][replicate in tile]
    long long n;
    int nruns, nchunks, K;
    double beta[kMaxBeta], th[kMaxBeta];
};

// a Nn >= f Nt for integers below 2^53 held in doubles: in fp64 when the difference is clear of the rounding of the two
// products, else on the exact 128-bit products
__device__ __forceinline__ bool cross_ge(double tg, double Nn, double fa, double Nt) {
    const double x = tg * Nn, y = fa * Nt, d = x - y, tol = (x + y) * 4.5e-16;
    if (d > tol) return true;
    if (d < -tol) return false;
    const unsigned long long a = (unsigned long long)tg, b = (unsigned long long)Nn, c = (unsigned long long)fa,
                             e = (unsigned long long)Nt;
    const unsigned long long xh = __umul64hi(a, b), xl = a * b, yh = __umul64hi(c, e), yl = c * e;
    return xh > yh || (xh == yh && xl >= yl);
}

template <bool G2>
__device__ __forceinline__ double weight_at(const WalkArgs& a, long long p, int lane, int code) {
    unsigned c = a.tab1[(size_t)a.g1s[p] * kTile + lane];
    if (G2) c *= a.tab2[(size_t)a.g2s[p] * kTile + lane];
    return code == CODE_DEAD ? 0.0 : (double)c;
}

template <bool G2, bool LLR, int PASS>
__global__ __launch_bounds__(256) void walk_kernel(const WalkArgs a) {
    const int lane = threadIdx.x & 63;
    const int run = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (run >= a.nruns) return;
    const long long p0 = (long long)run * kRun, p1 = p0 + kRun < a.n ? p0 + kRun : a.n;
    const size_t qs = (size_t)a.nruns * kTile, slot = (size_t)run * kTile + lane;
    const int Q1 = LLR ? 3 + 2 * a.K + 2 : 3;
    if (PASS == 1) {
        double tg = 0.0, nn = 0.0, last = -1.0, ct = 0.0, cn = 0.0;
        double ms[kMaxBeta], fa[kMaxBeta];
#pragma unroll
        for (int k = 0; k < kMaxBeta; ++k) ms[k] = fa[k] = 0.0;
#pragma unroll 4
        for (long long p = p0; p < p1; ++p) {
            const int code = a.fl[p] & 3;
            const double w = weight_at<G2>(a, p, lane, code);
            last = w > 0.0 ? (double)p : last;
            if (code == CODE_TGT) tg += w;
            if (code == CODE_NON) nn += w;
            if (LLR && code <= CODE_TGT) {
                const double s = (double)a.key[p], spv = a.sp[p];
#pragma unroll
                for (int k = 0; k < kMaxBeta; ++k) {
                    if (k < a.K) {
                        if (code == CODE_TGT && s < a.th[k]) ms[k] += w;
                        if (code == CODE_NON && s >= a.th[k]) fa[k] += w;
                    }
                }
                const double term = w > 0.0 ? w * spv : 0.0;  // a zero weight drops an infinite term
                if (code == CODE_TGT) ct += term;
                else cn += term;
            }
        }
        a.part[0 * qs + slot] = tg;
        a.part[1 * qs + slot] = nn;
        a.part[2 * qs + slot] = last;
        if (LLR) {
#pragma unroll
            for (int k = 0; k < kMaxBeta; ++k) {
                if (k < a.K) {
                    a.part[(size_t)(3 + k) * qs + slot] = ms[k];
                    a.part[(size_t)(3 + a.K + k) * qs + slot] = fa[k];
                }
            }
            a.part[(size_t)(3 + 2 * a.K) * qs + slot] = ct;
            a.part[(size_t)(4 + 2 * a.K) * qs + slot] = cn;
        }
    } else {
        // exclusive prefixes over the runs: inside the chunk of runs + of the chunks (integers: exact)
        const size_t cslot = (size_t)(run / kChunkRuns) * kTile + lane, cs = (size_t)a.nchunks * kTile;
        double tg = a.part[0 * qs + slot] + a.ctot[0 * cs + cslot], nn = a.part[1 * qs + slot] + a.ctot[1 * cs + cslot];
        const double Nt = a.tot[0 * kTile + lane], Nn = a.tot[1 * kTile + lane], last = a.tot[2 * kTile + lane];
        double bNt[kMaxBeta], best[kMaxBeta];
#pragma unroll
        for (int k = 0; k < kMaxBeta; ++k) {
            bNt[k] = (k < a.K ? a.beta[k] : 0.0) * Nt;
            best[k] = INFINITY;
        }
        double cross = INFINITY, ctg = 0.0, cfa = 0.0;
#pragma unroll 4
        for (long long p = p0; p < p1; ++p) {
            const int f = a.fl[p], code = f & 3;
            const double w = weight_at<G2>(a, p, lane, code);
            if (f & FLAG_START) {  // a candidate threshold: targets strictly below, non-targets at or above
                const double fav = Nn - nn, tN = tg * Nn;
#pragma unroll
                for (int k = 0; k < kMaxBeta; ++k)
                    if (k < a.K) best[k] = fmin(best[k], fma(bNt[k], fav, tN));  // Nt Nn (P_miss + beta P_fa)
                if (cross == INFINITY && (double)p <= last && cross_ge(tg, Nn, fav, Nt)) {
                    cross = (double)p;
                    ctg = tg;
                    cfa = fav;
                }
            }
            if (code == CODE_TGT) tg += w;
            if (code == CODE_NON) nn += w;
        }
#pragma unroll
        for (int k = 0; k < kMaxBeta; ++k)
            if (k < a.K) a.part[(size_t)(Q1 + k) * qs + slot] = best[k];
        a.part[(size_t)(Q1 + a.K) * qs + slot] = cross;
        a.part[(size_t)(Q1 + a.K + 1) * qs + slot] = ctg;
        a.part[(size_t)(Q1 + a.K + 2) * qs + slot] = cfa;
    }
}

struct ReduceArgs {
    double* part;
    double* ctot;
    double* tot;
    int nruns, nchunks, q0;
    int op[kMaxQ];
};

__device__ __forceinline__ double combine(int op, double x, double y) {
    return op == OP_MAX ? fmax(x, y) : (op == OP_MIN ? fmin(x, y) : x + y);
}

// Level 1, block (c, q): the kChunkRuns runs of chunk c, a quarter per wave, lane = replicate, the four results combined
// in wave order -> ctot; a scanned quantity becomes its exclusive prefix inside the chunk.
__global__ __launch_bounds__(256) void chunk_kernel(const ReduceArgs a) {
    __shared__ double sh[4][kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x, q = a.q0 + blockIdx.y, op = a.op[blockIdx.y];
    const int first = c * kChunkRuns + wave * (kChunkRuns / 4);
    const int r0 = first < a.nruns ? first : a.nruns;
    const int r1 = r0 + kChunkRuns / 4 < a.nruns ? r0 + kChunkRuns / 4 : a.nruns;
    double* col = a.part + (size_t)q * a.nruns * kTile + lane;
    const double id = op == OP_MAX ? -INFINITY : (op == OP_MIN ? INFINITY : 0.0);
    double acc = id;
    for (int r = r0; r < r1; ++r) acc = combine(op, acc, col[(size_t)r * kTile]);
    sh[wave][lane] = acc;
    __syncthreads();
    double off = id, total = id;
    for (int w = 0; w < 4; ++w) {
        if (w == wave) off = total;
        total = combine(op, total, sh[w][lane]);
    }
    if (wave == 0) a.ctot[((size_t)q * a.nchunks + c) * kTile + lane] = total;
    if (op == OP_SCAN) {
        for (int r = r0; r < r1; ++r) {
            const double v = col[(size_t)r * kTile];
            col[(size_t)r * kTile] = off;
            off += v;
        }
    }
}

// Level 2, block q: wave w takes the w-th of 16 contiguous pieces of the chunk results, lane = replicate; the pieces are
// combined in wave order, so the order of every sum depends on the number of runs alone.  A scanned quantity's chunk
// results become exclusive prefixes over the chunks.
__global__ __launch_bounds__(64 * kRedWaves) void reduce_kernel(const ReduceArgs a) {
    __shared__ double sh[kRedWaves][kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = a.q0 + blockIdx.x, op = a.op[blockIdx.x];
    const int n = a.nchunks, chunk = (n + kRedWaves - 1) / kRedWaves;
    const int r0 = wave * chunk < n ? wave * chunk : n;
    const int r1 = r0 + chunk < n ? r0 + chunk : n;
    double* col = a.ctot + (size_t)q * n * kTile + lane;
    const double id = op == OP_MAX ? -INFINITY : (op == OP_MIN ? INFINITY : 0.0);
    double acc = id;
    for (int r = r0; r < r1; ++r) acc = combine(op, acc, col[(size_t)r * kTile]);
    sh[wave][lane] = acc;
    __syncthreads();
    double off = id, total = id;
    for (int w = 0; w < kRedWaves; ++w) {
        if (w == wave) off = total;
        total = combine(op, total, sh[w][lane]);
    }
    if (wave == 0) a.tot[(size_t)q * kTile + lane] = total;
    if (op == OP_SCAN) {
        for (int r = r0; r < r1; ++r) {
            const double v = col[(size_t)r * kTile];
            col[(size_t)r * kTile] = off;
            off += v;
        }
    }
}

struct FinishArgs {
    WalkArgs w;
    int tile, B, llr, g2;
    double* out;
    long long* totals;
};

// block l = replicate l of the tile; the 64 lanes share the partial walk to the previous distinct threshold
__global__ __launch_bounds__(64) void finish_kernel(const FinishArgs f) {
    const WalkArgs& a = f.w;
    const int l = blockIdx.x, lane = threadIdx.x;
    const long long b = (long long)f.tile * kTile + l;
    if (b > f.B) return;
    const int K = a.K, Q1 = f.llr ? 3 + 2 * K + 2 : 3, ncol = K + 1 + (f.llr ? K + 1 : 0);
    const size_t qs = (size_t)a.nruns * kTile;
    const double Nt = a.tot[0 * kTile + l], Nn = a.tot[1 * kTile + l];
    double* out = f.out + (size_t)b * ncol;
    if (lane == 0) {
        f.totals[2 * b] = (long long)Nt;
        f.totals[2 * b + 1] = (long long)Nn;
    }
    if (Nt == 0.0 || Nn == 0.0) {  // a degenerate replicate
        if (lane < ncol) out[lane] = NAN;
        return;
    }
    double eer = 0.5;  // no crossing: (P_miss + P_fa) / 2 of the first threshold, (0 + 1) / 2
    const double cross = a.tot[(size_t)(Q1 + K) * kTile + l];
    if (cross != INFINITY) {  // cross >= 1: position 0 has P_miss = 0 < P_fa = 1
        const long long c = (long long)cross, rc = c / kRun;
        const double ctg = a.part[(size_t)(Q1 + K + 1) * qs + rc * kTile + l];
        const double cfa = a.part[(size_t)(Q1 + K + 2) * qs + rc * kTile + l];
        const long long q = trials::lower_bound(a.key, a.n, a.key[c - 1]), rq = q / kRun;
        double t0 = 0.0, n0 = 0.0;
        for (long long p = rq * kRun + lane; p < q; p += 64) {
            const int code = a.fl[p] & 3;
            unsigned cw = a.tab1[(size_t)a.g1s[p] * kTile + l];
            if (f.g2) cw *= a.tab2[(size_t)a.g2s[p] * kTile + l];
            if (code == CODE_TGT) t0 += (double)cw;
            if (code == CODE_NON) n0 += (double)cw;
        }
        t0 = wave_sum(t0);  // integers: exact in any order
        n0 = wave_sum(n0);
        const size_t cs = (size_t)a.nchunks * kTile, cq = (size_t)(rq / kChunkRuns) * kTile + l;
        t0 += a.part[0 * qs + rq * kTile + l] + a.ctot[0 * cs + cq];
        n0 += a.part[1 * qs + rq * kTile + l] + a.ctot[1 * cs + cq];
        const double pm0 = t0 / Nt, pf0 = (Nn - n0) / Nn, pm1 = ctg / Nt, pf1 = cfa / Nn;
        const double x0 = pm0 - pf0, x1 = pm1 - pf1;
        const double w = (x1 - x0) != 0.0 ? -x0 / (x1 - x0) : 0.5;
        eer = pm0 + w * (pm1 - pm0);
    }
    if (lane < K) {
        const double u = fmin(a.tot[(size_t)(Q1 + lane) * kTile + l], Nt * Nn);  // Nt Nn: the +inf threshold
        out[lane] = u / (Nt * Nn);
        if (f.llr) {
            const double ms = a.tot[(size_t)(3 + lane) * kTile + l], fa = a.tot[(size_t)(3 + K + lane) * kTile + l];
            out[K + 1 + lane] = ms / Nt + a.beta[lane] * (fa / Nn);
        }
    }
    if (lane == 0) {
        out[K] = eer;
        if (f.llr) {
            const double st = a.tot[(size_t)(3 + 2 * K) * kTile + l] * 1.4426950408889634;  // 1 / ln 2
            const double sn = a.tot[(size_t)(4 + 2 * K) * kTile + l] * 1.4426950408889634;
            out[2 * K + 1] = 0.5 * (st / Nt + sn / Nn);
        }
    }
}

struct Plan {
    size_t o_flags, o_key_in, o_key, o_idx_in, o_idx, o_fl, o_g1s, o_g2s, o_sp, o_tab32, o_tab8, o_part, o_ctot, o_tot, o_tmp;
    size_t tmp_bytes, total;
    int nruns, nchunks;
};

// the sort's temporary storage is reserved from N, without a device (trials::sort_reserve_bytes)
void make_plan(long long n, long long G1, long long G2, Plan* p) {
    const size_t nn = (size_t)n, gg = (size_t)(G1 + G2);
    p->nruns = (int)((n + kRun - 1) / kRun);
    p->nchunks = (p->nruns + kChunkRuns - 1) / kChunkRuns;
    size_t o = 0;
    p->o_flags = o; o += 256;
    p->o_key_in = o; o += up256(nn * 4);
    p->o_key = o; o += up256(nn * 4);
    p->o_idx_in = o; o += up256(nn * 4);
    p->o_idx = o; o += up256(nn * 4);
    p->o_fl = o; o += up256(nn);
    p->o_g1s = o; o += up256(nn * 4);
    p->o_g2s = o; o += up256(nn * 4);
    p->o_sp = o; o += up256(nn * 8);
    p->o_tab32 = o; o += up256(gg * kTile * 4);
    p->o_tab8 = o; o += up256(gg * kTile);
    p->o_part = o; o += up256((size_t)kMaxQ * p->nruns * kTile * 8);
    p->o_ctot = o; o += up256((size_t)kMaxQ * p->nchunks * kTile * 8);
    p->o_tot = o; o += up256((size_t)kMaxQ * kTile * 8);
    p->tmp_bytes = trials::sort_reserve_bytes(nn, 4, 4);
    p->o_tmp = o; o += p->tmp_bytes;
    p->total = o;
}

bool sizes_ok(int64_t N, int64_t G1, int64_t G2, int B) {
    return N >= 2 && N <= kMaxN && G1 >= 1 && G1 <= kMaxG && G2 >= 0 && G2 <= kMaxG && B >= 1 && B <= kMaxB;
}

template <bool G2, bool LLR>
void launch_walks(const WalkArgs& w, int pass, hipStream_t st) {
    const dim3 grid((unsigned)((w.nruns + 3) / 4));
    if (pass == 1) hipLaunchKernelGGL((walk_kernel<G2, LLR, 1>), grid, dim3(256), 0, st, w);
    else hipLaunchKernelGGL((walk_kernel<G2, LLR, 2>), grid, dim3(256), 0, st, w);
}

void launch_walk(const WalkArgs& w, bool g2, bool llr, int pass, hipStream_t st) {
    if (g2) llr ? launch_walks<true, true>(w, pass, st) : launch_walks<true, false>(w, pass, st);
    else llr ? launch_walks<false, true>(w, pass, st) : launch_walks<false, false>(w, pass, st);
}

}  // namespace

extern "C" {

int nplda_bootstrap_run(void) { return kRun; }
int nplda_bootstrap_tile(void) { return kTile; }

size_t nplda_bootstrap_workspace_bytes(int64_t N, int64_t G1, int64_t G2, int B) {
    if (!sizes_ok(N, G1, G2, B)) return 0;
    Plan p;
    make_plan(N, G1, G2, &p);
    return p.total;
}

int nplda_bootstrap_f32(const float* scores, const float* target, const int32_t* g1, const int32_t* g2, int64_t N, int64_t G1,
                        int64_t G2, int B, uint64_t seed, const double* betas, int K, int is_llr, double* out,
                        int64_t* totals, void* workspace, size_t workspace_bytes, nplda_stream_t stream) {
    if (!scores || !target || !g1 || !betas || !out || !totals || !workspace) return NPLDA_EINVAL;
    if (N < 2 || B < 1 || G1 < 1 || G2 < 0 || K < 1 || (g2 != nullptr) != (G2 > 0)) return NPLDA_EINVAL;
    if (K > kMaxBeta || !sizes_ok(N, G1, G2, B)) return NPLDA_EUNSUPPORTED;
    for (int k = 0; k < K; ++k)
        if (!(betas[k] > 0.0) || std::isinf(betas[k])) return NPLDA_EINVAL;
    if (!nplda_aligned16(workspace) || ((uintptr_t)out & 7u) || ((uintptr_t)totals & 7u) || ((uintptr_t)scores & 3u) ||
        ((uintptr_t)target & 3u) || ((uintptr_t)g1 & 3u) || ((uintptr_t)g2 & 3u))
        return NPLDA_EINVAL;
    Plan p;
    make_plan(N, G1, G2, &p);
    if (workspace_bytes < p.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned long long* flags = (unsigned long long*)(ws + p.o_flags);
    float* key_in = (float*)(ws + p.o_key_in);
    float* key = (float*)(ws + p.o_key);
    unsigned* idx_in = (unsigned*)(ws + p.o_idx_in);
    unsigned* idx = (unsigned*)(ws + p.o_idx);
    unsigned* tab32 = (unsigned*)(ws + p.o_tab32);
    unsigned char* tab8 = (unsigned char*)(ws + p.o_tab8);
    const bool llr = is_llr != 0, has2 = G2 > 0;
    const unsigned nblk = (unsigned)((N + 255) / 256);
    if (hipError_t e = hipMemsetAsync(flags, 0, 256, st)) return (int)e;
    hipLaunchKernelGGL(prep_kernel, dim3(nblk), dim3(256), 0, st, scores, (long long)N, key_in, idx_in);
    if (int rc = nplda_launch_status()) return rc;
    if (int rc = trials::sort_pairs(ws + p.o_tmp, p.tmp_bytes, key_in, key, idx_in, idx, (size_t)N, st)) return rc;
    GatherArgs g;
    g.scores = scores; g.target = target; g.g1 = g1; g.g2 = g2; g.key = key; g.idx = idx; g.n = N;
    g.G1 = (int)G1; g.G2 = (int)G2; g.llr = llr;
    g.fl = (unsigned char*)(ws + p.o_fl); g.g1s = (int*)(ws + p.o_g1s); g.g2s = (int*)(ws + p.o_g2s);
    g.sp = (double*)(ws + p.o_sp); g.flags = flags;
    hipLaunchKernelGGL(gather_kernel, dim3(nblk), dim3(256), 0, st, g);
    if (int rc = nplda_launch_status()) return rc;

    WalkArgs w;
    w.key = key; w.fl = g.fl; w.g1s = g.g1s; w.g2s = g.g2s; w.sp = g.sp;
    w.tab1 = tab8; w.tab2 = tab8 + (size_t)G1 * kTile;
    w.part = (double*)(ws + p.o_part); w.ctot = (double*)(ws + p.o_ctot); w.tot = (double*)(ws + p.o_tot);
    w.n = N; w.nruns = p.nruns; w.nchunks = p.nchunks; w.K = K;
    for (int k = 0; k < kMaxBeta; ++k) {
        w.beta[k] = k < K ? betas[k] : 1.0;
        w.th[k] = std::log(w.beta[k]);
    }
    const int Q1 = llr ? 3 + 2 * K + 2 : 3;
    ReduceArgs r1, r2;
    r1.part = r2.part = w.part; r1.ctot = r2.ctot = w.ctot; r1.tot = r2.tot = w.tot;
    r1.nruns = r2.nruns = p.nruns; r1.nchunks = r2.nchunks = p.nchunks;
    r1.q0 = 0; r2.q0 = Q1;
    for (int q = 0; q < kMaxQ; ++q) {
        r1.op[q] = q < 2 ? OP_SCAN : (q == 2 ? OP_MAX : OP_SUM);
        r2.op[q] = OP_MIN;
    }
    const long long tab_total = (G1 + G2) * kTile;
    const unsigned tblk = (unsigned)((tab_total + 255) / 256);
    const int ntiles = (B + 1 + kTile - 1) / kTile;
    for (int tile = 0; tile < ntiles; ++tile) {
        if (hipError_t e = hipMemsetAsync(tab32, 0, (size_t)tab_total * 4, st)) return (int)e;
        hipLaunchKernelGGL(draw_kernel, dim3(tblk), dim3(256), 0, st, tab32, (long long)G1, (long long)G2,
                           (unsigned long long)seed, tile, B);
        hipLaunchKernelGGL(pack_kernel, dim3(tblk), dim3(256), 0, st, (const unsigned*)tab32, tab8, tab_total, tile, flags);
        launch_walk(w, has2, llr, 1, st);
        hipLaunchKernelGGL(chunk_kernel, dim3(p.nchunks, Q1), dim3(256), 0, st, r1);
        hipLaunchKernelGGL(reduce_kernel, dim3(Q1), dim3(64 * kRedWaves), 0, st, r1);
        launch_walk(w, has2, llr, 2, st);
        hipLaunchKernelGGL(chunk_kernel, dim3(p.nchunks, K + 1), dim3(256), 0, st, r2);
        hipLaunchKernelGGL(reduce_kernel, dim3(K + 1), dim3(64 * kRedWaves), 0, st, r2);
        FinishArgs f;
        f.w = w; f.tile = tile; f.B = B; f.llr = llr; f.g2 = has2; f.out = out; f.totals = (long long*)totals;
        hipLaunchKernelGGL(finish_kernel, dim3(kTile), dim3(64), 0, st, f);
        if (int rc = nplda_launch_status()) return rc;
    }
    return NPLDA_OK;
}

}  // extern "C"
