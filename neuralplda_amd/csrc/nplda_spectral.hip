// nplda_spectral.hip — spectral clustering with an auto-tuned neighbour count (NME-SC), P ragged problems per call
// (gfx950).  design/k25_spectral.md has the contract, the kernel shapes and the budget.
//
// A CELL is a (problem, candidate neighbour count) pair.  Three launches:
//   graph_kernel    one workgroup per cell: a wave per row selects the m largest off-diagonal scores (a bitwise threshold
//                   search over order-preserving keys in LDS, equal keys by ascending column), B as bytes in the workspace;
//                   then L = diag(d) - (B + B^T) / 2 in fp64 (every entry a multiple of 1/2, nothing rounds) and W = I.
//   jacobi_kernel   one workgroup per cell: cyclic Jacobi in fp64 with the round-robin ordering.  A step computes its n / 2
//                   rotations from the pre-step matrix, then ONE pass applies them: the 2 x 2 piece of pair k's rows and
//                   pair l's columns becomes J_k^T M J_l, in a form whose bits are the same for the piece and its mirror,
//                   so L stays exactly symmetric; the rows of W = V^T of pair k take J_k^T.  Two barriers per step.  The
//                   tail ranks the diagonal, writes the eigenvalues, the eigengap count and the normalised eigenvectors.
//   finish_kernel   one workgroup per problem: the candidate with the smallest ratio, then k-means on its embedding.
// kmeans_kernel is the k-means of finish_kernel on a caller-given matrix.  __syncthreads() only: no cross-block hand-off, no
// floating-point atomics, no memset, nothing read back; every loop is bounded by n, a sweep limit or max_iters.
#include <cmath>

#include "nplda_cohort_common.h"
#include "nplda_ragged.h"

// nothing in this file may be contracted into a multiply-add: the mirrored pieces of the Jacobi pass and the k-means sums
// are specified one multiplication and one addition at a time
#pragma clang fp contract(off)

namespace {

constexpr int kMaxN = 2048;          // rows of a problem: two fp64 matrices of a cell take 16 n^2 bytes
constexpr int kMaxK = 64;            // clusters, the 64 slots of the VB-HMM and the DER
constexpr int kMaxC = 16;            // candidates
constexpr int kSmallN = 128;         // a call whose largest problem has at most this many rows runs the eigensolver with
constexpr int kSmallBlock = 256;     // this many threads per cell, any other with kBlock
constexpr int kBlock = 1024;
constexpr int kMaxSweeps = 30;
constexpr int kGraphBlock = 256;     // four waves, a row each
constexpr int kFinishBlock = 256;
constexpr long long kMaxP = (1ll << 22) - 1;

__host__ __device__ inline long long even_up(long long n) { return n + (n & 1); }
// bytes of a cell: A and W (ne x ne fp64, ne = n rounded up to even), B (n x n bytes)
__host__ __device__ inline long long cell_bytes(long long n) {
    const long long ne = even_up(n);
    return 16 * ne * ne + ((n * n + 15) & ~15ll);
}
// bytes of a problem next to its cells: the k-means distances
__host__ __device__ inline long long prob_bytes(long long n) { return (8 * n + 15) & ~15ll; }
__host__ __device__ inline long long vec_rows(long long n, int maxc) { return n < maxc + 1 ? n : maxc + 1; }

// what a problem of n rows takes with C candidates (csrc/nplda_ragged.h): n^2 matrix elements, the workspace bytes of its C
// cells and its k-means distances, and the rows x n doubles of its cells in `vectors`.  kVecs is a start on the device only:
// the caller sizes `vectors` (ops.spectral), and make_plan, which has no maxc, leaves that term unread.
enum { kElems, kWsBytes, kVecs, kTerms };
struct Terms {
    int C, maxc;
    __host__ __device__ void operator()(long long n, long long, long long* t) const {
        t[kElems] = n * n;
        t[kWsBytes] = C * cell_bytes(n) + prob_bytes(n);
        t[kVecs] = C * vec_rows(n, maxc) * n;
    }
};

struct Plan {
    int status;
    long long rows, max_n, elems;
    size_t ws_bytes;
};

Plan make_plan(const int64_t* offs, int64_t P, int C) {
    Plan r = {NPLDA_OK, 0, 0, 0, 0};
    if (C < 0 || C > kMaxC) {
        r.status = NPLDA_EINVAL;
        return r;
    }
    long long ws = 0;
    r.status = ragged_walk(offs, offs, P, kMaxP, [&](long long n, long long) {
        if (n > kMaxN) return NPLDA_EUNSUPPORTED;
        long long t[kTerms];
        Terms{C, 0}(n, n, t);
        if (n > r.max_n) r.max_n = n;
        r.elems += t[kElems];
        ws += t[kWsBytes];
        return NPLDA_OK;
    });
    if (r.status == NPLDA_OK && P > 0) r.rows = offs[P];
    r.ws_bytes = up256((size_t)ws) + 256;
    return r;
}

// ---- device: where problem p starts ---------------------------------------------------------------------------------------------

struct Starts {
    long long row0, n, elem0, ws0, vec0;
};

__device__ __forceinline__ Starts problem_starts(const long long* __restrict__ offs, long long p, int C, int maxc,
                                                 long long* red /* [48] */) {
    long long sum[kTerms];
    ragged_starts(offs, p, Terms{C, maxc}, red, sum);
    Starts s;
    s.elem0 = sum[kElems];
    s.ws0 = sum[kWsBytes];
    s.vec0 = sum[kVecs];
    s.row0 = offs[p];
    s.n = offs[p + 1] - s.row0;
    return s;
}

struct Args {
    const float* S;
    const long long* offs;
    int nb[kMaxC];
    int C, min_clusters, max_clusters, max_iters;
    double *eigenvalues, *ratio;
    int *kstar, *n_sweeps, *converged, *chosen, *n_clusters, *n_kmeans_iters, *labels;
    double *embedding, *degrees, *vectors;
    char* ws;
};

// ---- (a) the graph ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kGraphBlock) void graph_kernel(const Args a) {
    __shared__ long long red[48];
    __shared__ unsigned keys[kGraphBlock / 64][kMaxN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cand = blockIdx.y;
    const Starts s = problem_starts(a.offs, blockIdx.x, a.C, a.max_clusters, red);
    const int n = (int)s.n;
    if (n <= 0) return;
    const int ne = (int)even_up(n);
    const int c = a.nb[cand];
    const int m = c < n - 1 ? c : n - 1;
    const float* S = a.S + s.elem0;
    char* cell = a.ws + s.ws0 + (long long)cand * cell_bytes(n);
    double* A = (double*)cell;
    double* W = A + (size_t)ne * ne;
    unsigned char* B = (unsigned char*)(W + (size_t)ne * ne);
    unsigned* key = keys[wave];
    const unsigned long long below = (1ull << lane) - 1ull;

    for (int i0 = 0; i0 < n; i0 += kGraphBlock / 64) {
        const int i = i0 + wave;
        const bool on = i < n;           // wave-uniform
        const int ic = on ? i : n - 1;   // (clamped: a wave without a row reads the last one and stores nothing)
        __syncthreads();                 // the keys of the last row have been used
        for (int j = lane; j < n; j += 64) {
            unsigned b = __float_as_uint(S[(size_t)ic * n + j]);
            if ((b << 1) == 0u) b = 0u;  // -0.0f equals +0.0f
            key[j] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // unsigned order = float order
        }
        __syncthreads();
        if (!on) continue;
        // the m-th largest key among j != i: the largest T with at least m keys >= T, bit by bit
        unsigned T = 0u;
        if (m > 0) {
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned t = T | (1u << bit);
                int cnt = 0;
                for (int j0 = 0; j0 < n; j0 += 64) {
                    const int j = j0 + lane;
                    cnt += __popcll(__ballot(j < n && j != i && key[j] >= t));
                }
                if (cnt >= m) T = t;
            }
        }
        int above = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            above += __popcll(__ballot(j < n && j != i && key[j] > T));
        }
        const int need = m - above;  // keys equal to T to take, by ascending column
        int seen = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = j < n && j != i && m > 0;
            const unsigned k = valid ? key[j] : 0u;
            const bool eq = valid && k == T;
            const unsigned long long bal = __ballot(eq);
            const bool sel = valid && (k > T || (eq && seen + __popcll(bal & below) < need));
            if (j < n) B[(size_t)i * n + j] = sel ? 1 : 0;
            seen += __popcll(bal);
        }
    }
    __syncthreads();  // B is complete

    for (int i = wave; i < ne; i += kGraphBlock / 64) {
        double d = 0.0;
        for (int j = lane; j < ne; j += 64) {
            double v = 0.0;
            if (i < n && j < n && j != i) {
                v = 0.5 * (double)((int)B[(size_t)i * n + j] + (int)B[(size_t)j * n + i]);
                d += v;  // multiples of 1/2 below 2^12: exact in any order
                v = -v;
            }
            if (j != i) A[(size_t)i * ne + j] = v;
            W[(size_t)i * ne + j] = j == i ? 1.0 : 0.0;
        }
        d = wave_sum(d);
        if (lane == 0) {
            A[(size_t)i * ne + i] = d;  // (the pad row of an odd n: 0)
            if (a.degrees && i < n) a.degrees[s.row0 * a.C + (long long)cand * n + i] = d;
        }
    }
}

// ---- (b) the eigensolver ----------------------------------------------------------------------------------------------------------

// pair i of round r among ne players (ne even): the circle method with player ne - 1 fixed
__device__ __forceinline__ void pair_of(int r, int i, int ne, int& p, int& q) {
    const int mod = ne - 1;
    int x = r + i;
    if (x >= mod) x -= mod;
    int y = i == 0 ? mod : r - i;
    if (y < 0) y += mod;
    p = x < y ? x : y;
    q = x < y ? y : x;
}

template <int BLK>
__global__ __launch_bounds__(BLK) void jacobi_kernel(const Args a) {
    constexpr int MAXH = BLK == kBlock ? kMaxN / 2 : kSmallN / 2;
    constexpr int NW = BLK / 64;
    __shared__ long long red[48];
    __shared__ double shd[3 * MAXH];  // the step's c, s, t; afterwards the diagonal
    __shared__ int shi[2 * MAXH];     // the step's p, q; afterwards the rank order
    __shared__ double wred[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cand = blockIdx.y;
    const long long cellno = (long long)blockIdx.x * a.C + cand;
    const Starts st = problem_starts(a.offs, blockIdx.x, a.C, a.max_clusters, red);
    const int n = (int)st.n;
    const int maxc = a.max_clusters;
    double* ev = a.eigenvalues + cellno * (maxc + 2);
    const int c = a.nb[cand];
    const int kfloor = a.min_clusters > 1 ? a.min_clusters : 1;
    if (n <= 0 || n > 2 * MAXH) {  // (n > 2 MAXH cannot happen: the host picks the block by the largest problem)
        for (int r = tid; r < maxc + 2; r += BLK) ev[r] = __builtin_nan("");
        if (tid == 0) {
            a.kstar[cellno] = 1;
            a.ratio[cellno] = __builtin_inf();
            a.n_sweeps[cellno] = 0;
            a.converged[cellno] = 1;
        }
        return;
    }
    const int ne = (int)even_up(n), h = ne / 2;
    char* cell = a.ws + st.ws0 + (long long)cand * cell_bytes(n);
    double* A = (double*)cell;
    double* W = A + (size_t)ne * ne;
    double *cs_c = shd, *cs_s = shd + MAXH, *cs_t = shd + 2 * MAXH;
    int *pi = shi, *qi = shi + MAXH;

    // the threshold: ||L||_F 2^-53 / ne.  The sum of squares is exact (multiples of 1/4 below 2^53) in any order.
    double ss = 0.0;
    for (int e = tid; e < ne * ne; e += BLK) {
        const double v = A[e];
        ss += v * v;
    }
    ss = wave_sum(ss);
    if (lane == 0) wred[wave] = ss;
    __syncthreads();
    ss = 0.0;
    for (int u = 0; u < NW; ++u) ss += wred[u];
    const double thr = sqrt(ss) * 0x1p-53 / (double)ne;

    int sweeps = 0, conv = 0;
    for (int sw = 0; sw < kMaxSweeps && !conv; ++sw) {
        int any = 0;
        for (int r = 0; r < ne - 1; ++r) {
            int rot = 0;
            if (tid < h) {
                int p, q;
                pair_of(r, tid, ne, p, q);
                const double app = A[(size_t)p * ne + p], aqq = A[(size_t)q * ne + q], apq = A[(size_t)p * ne + q];
                double cc = 1.0, sn = 0.0, t = 0.0;
                if (fabs(apq) > thr) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    cc = 1.0 / sqrt(t * t + 1.0);
                    sn = t * cc;
                    rot = 1;
                }
                cs_c[tid] = cc;
                cs_s[tid] = sn;
                cs_t[tid] = t;
                pi[tid] = p;
                qi[tid] = rot ? q : -1 - q;  // (the sign carries "no rotation")
            }
            const int some = __syncthreads_or(rot);
            any |= some;
            if (some) {
                // A <- J^T A J, piece by piece; the diagonal pieces take the closed form
                for (int e = tid; e < h * h; e += BLK) {
                    const int k = e / h, l = e - k * h;
                    const int qk0 = qi[k], ql0 = qi[l];
                    if (qk0 < 0 && ql0 < 0) continue;  // neither pair rotates
                    const int pk = pi[k], pl = pi[l], qk = qk0 < 0 ? -1 - qk0 : qk0, ql = ql0 < 0 ? -1 - ql0 : ql0;
                    double* r0 = A + (size_t)pk * ne;
                    double* r1 = A + (size_t)qk * ne;
                    if (k == l) {
                        const double x = cs_t[k] * r0[qk];
                        r0[pk] = r0[pk] - x;
                        r1[qk] = r1[qk] + x;
                        r0[qk] = 0.0;
                        r1[pk] = 0.0;
                        continue;
                    }
                    const double ck = cs_c[k], sk = cs_s[k], cl = cs_c[l], sl = cs_s[l];
                    const double m00 = r0[pl], m01 = r0[ql], m10 = r1[pl], m11 = r1[ql];
                    const double cc = ck * cl, cs = ck * sl, sc = sk * cl, s2 = sk * sl;
                    r0[pl] = (cc * m00 + s2 * m11) - (cs * m01 + sc * m10);
                    r0[ql] = (cc * m01 - s2 * m10) + (cs * m00 - sc * m11);
                    r1[pl] = (cc * m10 - s2 * m01) + (sc * m00 - cs * m11);
                    r1[ql] = (s2 * m00 + cc * m11) + (cs * m10 + sc * m01);
                }
                // W <- J^T W: rows p and q of pair k
                for (int e = tid; e < h * ne; e += BLK) {
                    const int k = e / ne, j = e - k * ne;
                    const int qk0 = qi[k];
                    if (qk0 < 0) continue;
                    double* w0 = W + (size_t)pi[k] * ne + j;
                    double* w1 = W + (size_t)qk0 * ne + j;
                    const double ck = cs_c[k], sk = cs_s[k], x = *w0, y = *w1;
                    *w0 = ck * x - sk * y;
                    *w1 = sk * x + ck * y;
                }
            }
            __syncthreads();
        }
        ++sweeps;
        if (!any) conv = 1;
    }

    // the tail: rank the diagonal (equal values by position), eigenvalues, the count, the eigenvectors
    double* dg = shd;
    int* order = shi;
    auto at = [&](int r) {  // the position with rank r, clamped to the problem
        const int o = order[r];
        return o < 0 ? 0 : (o < n ? o : n - 1);
    };
    for (int i = tid; i < n; i += BLK) dg[i] = A[(size_t)i * ne + i];
    __syncthreads();
    for (int i = tid; i < n; i += BLK) {
        const double v = dg[i];
        int rk = 0;
        for (int j = 0; j < n; ++j) {
            const double u = dg[j];
            rk += (u < v || (u == v && j < i)) ? 1 : 0;
        }
        rk = rk < n ? rk : n - 1;  // (a NaN, outside the contract, cannot push a subscript out)
        order[rk] = i;
    }
    __syncthreads();
    const int K = maxc < n - 1 ? maxc : n - 1;
    for (int r = tid; r < maxc + 2; r += BLK) {
        double v = __builtin_nan("");
        if (r <= K) v = dg[at(r)];
        if (r == maxc + 1) v = dg[at(n - 1)];
        ev[r] = v;
    }
    if (wave == 0) {
        const int k = lane + 1;
        const bool valid = k >= kfloor && k <= K;
        double gap = 0.0;
        int bk = kNone;
        if (valid) {
            gap = dg[at(k)] - dg[at(k - 1)];
            bk = k;
        }
        wave_best(gap, bk);
        if (lane == 0) {
            const double top = dg[at(n - 1)];
            int ks = kfloor < (n > 1 ? n : 1) ? kfloor : (n > 1 ? n : 1);
            double ratio = __builtin_inf();
            if (n > 1 && bk != kNone && top > 0.0) {
                const double g = gap / top;
                if (g > 0.0) {
                    ks = bk;
                    ratio = (double)c / g;
                }
            }
            a.kstar[cellno] = ks;
            a.ratio[cellno] = ratio;
            a.n_sweeps[cellno] = sweeps;
            a.converged[cellno] = conv;
        }
    }
    // the K + 1 smallest eigenvectors with unit length, as rows, over A (its diagonal is in LDS)
    double* Ev = A;
    double* vout = a.vectors ? a.vectors + st.vec0 + (long long)cand * vec_rows(n, maxc) * n : nullptr;
    for (int r = wave; r <= K; r += NW) {
        const double* w = W + (size_t)at(r) * ne;
        double s2 = 0.0;
        for (int j = lane; j < n; j += 64) s2 += w[j] * w[j];
        s2 = wave_sum(s2);
        const double len = sqrt(s2);
        for (int j = lane; j < n; j += 64) {
            const double v = w[j] / len;
            Ev[(size_t)r * n + j] = v;
            if (vout) vout[(size_t)r * n + j] = v;
        }
    }
}

// ---- (c) the candidate and the partition ------------------------------------------------------------------------------------------

struct KmShared {
    double cen[kMaxK * kMaxK];
    int asg[kMaxN];
    int first[kMaxK], rank[kMaxK];
    double bv[kFinishBlock / 64];
    int bi[kFinishBlock / 64];
};

// squared distance of row i to centre c, in column order, one multiplication and one addition at a time
__device__ __forceinline__ double dist2(const double* __restrict__ X, long long rs, long long cs, int i, const double* cen, int d) {
    double acc = 0.0;
    for (int j = 0; j < d; ++j) {
        const double diff = __dsub_rn(X[i * rs + j * cs], cen[j]);
        acc = __dadd_rn(acc, __dmul_rn(diff, diff));
    }
    return acc;
}

// k-means on the n x d matrix X(i, j) = X[i rs + j cs] with k <= min(n, 64) centres, by the whole block
__device__ void kmeans_block(KmShared& sh, const double* __restrict__ X, long long rs, long long cs, int n, int d, int k,
                             int max_iters, double* mind, int* labels, int* n_clusters, int* n_iters) {
    constexpr int B = kFinishBlock;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < d; j += B) sh.cen[j] = X[j * cs];
    __syncthreads();
    for (int i = tid; i < n; i += B) mind[i] = dist2(X, rs, cs, i, sh.cen, d);
    for (int c = 1; c < k; ++c) {
        double v = -1.0;
        int bi = kNone;
        for (int i = tid; i < n; i += B) {  // rows ascending on a thread: the first of equal values stays
            const double m = mind[i];
            if (bi == kNone || m > v) {
                v = m;
                bi = i;
            }
        }
        wave_best(v, bi);
        if (lane == 0) {
            sh.bv[wave] = v;
            sh.bi[wave] = bi;
        }
        __syncthreads();
        v = sh.bv[0];
        bi = sh.bi[0];
        for (int w = 1; w < B / 64; ++w)
            if (before(sh.bv[w], sh.bi[w], v, bi)) {
                v = sh.bv[w];
                bi = sh.bi[w];
            }
        bi = bi < n ? bi : n - 1;
        for (int j = tid; j < d; j += B) sh.cen[c * d + j] = X[bi * rs + j * cs];
        __syncthreads();
        for (int i = tid; i < n; i += B) {
            const double m = dist2(X, rs, cs, i, sh.cen + c * d, d);
            if (m < mind[i]) mind[i] = m;
        }
    }
    int iters = 0;
    for (int it = 0; it < max_iters; ++it) {
        int changed = 0;
        for (int i = tid; i < n; i += B) {
            double bv = dist2(X, rs, cs, i, sh.cen, d);
            int bc = 0;
            for (int c = 1; c < k; ++c) {
                const double m = dist2(X, rs, cs, i, sh.cen + c * d, d);
                if (m < bv) {
                    bv = m;
                    bc = c;
                }
            }
            if (it == 0 || sh.asg[i] != bc) changed = 1;
            sh.asg[i] = bc;
        }
        ++iters;
        if (!__syncthreads_or(changed)) break;  // the assignment of the last iteration again
        for (int e = tid; e < k * d; e += B) {
            const int c = e / d, j = e - c * d;
            double sum = 0.0;
            int cnt = 0;
            for (int i = 0; i < n; ++i)  // row order
                if (sh.asg[i] == c) {
                    sum = __dadd_rn(sum, X[i * rs + j * cs]);
                    ++cnt;
                }
            if (cnt > 0) sh.cen[e] = sum / (double)cnt;  // a centre without rows keeps its place
        }
        __syncthreads();
    }
    // labels: the dense rank of the row's cluster in order of the clusters' smallest members
    if (tid < kMaxK) sh.first[tid] = n;
    __syncthreads();
    for (int i = tid; i < n; i += B) atomicMin(&sh.first[sh.asg[i] & (kMaxK - 1)], i);
    __syncthreads();
    if (tid < kMaxK) {
        int rk = 0;
        const int f = tid < k ? sh.first[tid] : n;
        for (int c = 0; c < k; ++c) rk += sh.first[c] < f ? 1 : 0;
        sh.rank[tid] = rk;
    }
    __syncthreads();
    for (int i = tid; i < n; i += B) labels[i] = sh.rank[sh.asg[i] & (kMaxK - 1)];
    if (tid == 0) {
        int live = 0;
        for (int c = 0; c < k; ++c) live += sh.first[c] < n ? 1 : 0;
        *n_clusters = live;
        *n_iters = iters;
    }
}

__global__ __launch_bounds__(kFinishBlock) void finish_kernel(const Args a) {
    __shared__ long long red[48];
    __shared__ KmShared sh;
    const int tid = threadIdx.x;
    const long long p = blockIdx.x;
    const Starts st = problem_starts(a.offs, p, a.C, a.max_clusters, red);
    const int n = (int)st.n;
    int best = 0;
    for (int c = 1; c < a.C; ++c)
        if (a.ratio[p * a.C + c] < a.ratio[p * a.C + best]) best = c;  // the lowest index among equal ratios
    if (n <= 0) {
        if (tid == 0) {
            a.chosen[p] = best;
            a.n_clusters[p] = 0;
            a.n_kmeans_iters[p] = 0;
        }
        return;
    }
    int k = a.kstar[p * a.C + best];
    k = k < n ? k : n;
    k = k < kMaxK ? k : kMaxK;
    k = k > 1 ? k : 1;
    const double* Ev = (const double*)(a.ws + st.ws0 + (long long)best * cell_bytes(n));  // rows = eigenvectors
    double* mind = (double*)(a.ws + st.ws0 + (long long)a.C * cell_bytes(n));
    if (a.embedding) {
        double* E = a.embedding + st.row0 * a.max_clusters;
        for (int e = tid; e < n * k; e += kFinishBlock) {
            const int i = e / k, j = e - i * k;
            E[e] = Ev[(size_t)j * n + i];
        }
    }
    if (tid == 0) a.chosen[p] = best;
    kmeans_block(sh, Ev, 1, n, n, k, k, a.max_iters, mind, a.labels + st.row0, a.n_clusters + p, a.n_kmeans_iters + p);
}

struct KmArgs {
    const double* E;
    const long long* offs;
    int dim, k, max_iters;
    int *n_clusters, *n_iters, *labels;
    char* ws;
};

__global__ __launch_bounds__(kFinishBlock) void kmeans_kernel(const KmArgs a) {
    __shared__ long long red[48];
    __shared__ KmShared sh;
    const long long p = blockIdx.x;
    const Starts st = problem_starts(a.offs, p, 0, 0, red);  // ws0: the sum of prob_bytes
    const int n = (int)st.n;
    if (n <= 0) {
        if (threadIdx.x == 0) {
            a.n_clusters[p] = 0;
            a.n_iters[p] = 0;
        }
        return;
    }
    const int k = a.k < n ? a.k : n;
    kmeans_block(sh, a.E + st.row0 * a.dim, a.dim, 1, n, a.dim, k, a.max_iters, (double*)(a.ws + st.ws0), a.labels + st.row0,
                 a.n_clusters + p, a.n_iters + p);
}

}  // namespace

extern "C" {

int nplda_spectral_max_n(void) { return kMaxN; }
int nplda_spectral_max_k(void) { return kMaxK; }
int nplda_spectral_max_candidates(void) { return kMaxC; }
int nplda_spectral_block(void) { return kBlock; }
int nplda_spectral_small_n(void) { return kSmallN; }
int nplda_spectral_small_block(void) { return kSmallBlock; }
int nplda_spectral_max_sweeps(void) { return kMaxSweeps; }

size_t nplda_spectral_workspace_bytes(const int64_t* offsets_host, int64_t P, int n_candidates) {
    if (n_candidates < 1) return 0;
    const Plan r = make_plan(offsets_host, P, n_candidates);
    return r.status == NPLDA_OK ? r.ws_bytes : 0;
}

size_t nplda_spectral_kmeans_workspace_bytes(const int64_t* offsets_host, int64_t P) {
    const Plan r = make_plan(offsets_host, P, 0);
    return r.status == NPLDA_OK ? r.ws_bytes : 0;
}

int nplda_spectral_f32(const float* S, const int64_t* offsets_host, const int64_t* offsets, int64_t P, const int32_t* neighbours,
                       int n_candidates, int min_clusters, int max_clusters, int max_iters, double* eigenvalues, int32_t* kstar,
                       double* ratio, int32_t* n_sweeps, int32_t* converged, int32_t* chosen, int32_t* n_clusters,
                       int32_t* n_kmeans_iters, int32_t* labels, double* embedding, double* degrees, double* vectors, void* ws,
                       size_t ws_bytes, nplda_stream_t stream) {
    if (!neighbours || n_candidates < 1 || n_candidates > kMaxC) return NPLDA_EINVAL;
    for (int c = 0; c < n_candidates; ++c)
        if (neighbours[c] < 1 || (c > 0 && neighbours[c] <= neighbours[c - 1])) return NPLDA_EINVAL;
    if (min_clusters < 1 || max_clusters < min_clusters || max_clusters > kMaxK || max_iters < 1) return NPLDA_EINVAL;
    const Plan r = make_plan(offsets_host, P, n_candidates);
    if (r.status != NPLDA_OK) return r.status;
    if (P == 0) return NPLDA_OK;
    if (!offsets || !eigenvalues || !kstar || !ratio || !n_sweeps || !converged || !chosen || !n_clusters || !n_kmeans_iters)
        return NPLDA_EINVAL;
    if ((((uintptr_t)eigenvalues) | ((uintptr_t)ratio) | ((uintptr_t)embedding) | ((uintptr_t)degrees) | ((uintptr_t)vectors)) & 7u)
        return NPLDA_EINVAL;
    if (r.rows > 0 && (!S || !labels || !ws || !nplda_aligned16(ws))) return NPLDA_EINVAL;
    if (r.rows > 0 && ws_bytes < r.ws_bytes) return NPLDA_ENOSPC;
    Args a;
    a.S = S;
    a.offs = (const long long*)offsets;
    for (int c = 0; c < kMaxC; ++c) a.nb[c] = c < n_candidates ? neighbours[c] : 0;
    a.C = n_candidates;
    a.min_clusters = min_clusters;
    a.max_clusters = max_clusters;
    a.max_iters = max_iters;
    a.eigenvalues = eigenvalues;
    a.ratio = ratio;
    a.kstar = (int*)kstar;
    a.n_sweeps = (int*)n_sweeps;
    a.converged = (int*)converged;
    a.chosen = (int*)chosen;
    a.n_clusters = (int*)n_clusters;
    a.n_kmeans_iters = (int*)n_kmeans_iters;
    a.labels = (int*)labels;
    a.embedding = embedding;
    a.degrees = degrees;
    a.vectors = vectors;
    a.ws = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    const dim3 cells((unsigned)P, (unsigned)n_candidates);
    if (r.rows > 0) hipLaunchKernelGGL(graph_kernel, cells, dim3(kGraphBlock), 0, st, a);
    if (r.max_n <= kSmallN) hipLaunchKernelGGL((jacobi_kernel<kSmallBlock>), cells, dim3(kSmallBlock), 0, st, a);
    else hipLaunchKernelGGL((jacobi_kernel<kBlock>), cells, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)P), dim3(kFinishBlock), 0, st, a);
    return nplda_launch_status();
}

int nplda_spectral_kmeans_f64(const double* E, const int64_t* offsets_host, const int64_t* offsets, int64_t P, int dim, int k,
                              int max_iters, int32_t* n_clusters, int32_t* n_iters, int32_t* labels, void* ws, size_t ws_bytes,
                              nplda_stream_t stream) {
    if (dim < 1 || dim > kMaxK || k < 1 || k > kMaxK || max_iters < 1) return NPLDA_EINVAL;
    const Plan r = make_plan(offsets_host, P, 0);
    if (r.status != NPLDA_OK) return r.status;
    if (P == 0) return NPLDA_OK;
    if (!offsets || !n_clusters || !n_iters) return NPLDA_EINVAL;
    if (r.rows > 0 && (!E || (((uintptr_t)E) & 7u) || !labels || !ws || !nplda_aligned16(ws))) return NPLDA_EINVAL;
    if (r.rows > 0 && ws_bytes < r.ws_bytes) return NPLDA_ENOSPC;
    KmArgs a = {E, (const long long*)offsets, dim, k, max_iters, (int*)n_clusters, (int*)n_iters, (int*)labels, (char*)ws};
    hipLaunchKernelGGL(kmeans_kernel, dim3((unsigned)P), dim3(kFinishBlock), 0, (hipStream_t)stream, a);
    return nplda_launch_status();
}

}  // extern "C"
