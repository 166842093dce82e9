// Isotonic regression of the labels on the scores (PAV) on gfx950: minimum Cllr, the equal error rate on the ROC convex
// hull and the PAV calibration map — design/k18_pav_rocch.md.  All three come from the strict lower convex hull of the
// cumulative (trials, targets) diagram of the score bins.
// Stages, all enqueued on one stream with no read-back (the launch count depends on N alone):
//   label   scores -> sort keys (an excluded trial or a NaN score gets a positive NaN key: it sorts behind +inf), labels
//           -> packed (target << 32 | non-target) counts                    [nplda_trials.h, policy Excluded::kNanKey]
//   sort    radix sort of the (key, count) pairs, then the exclusive scan of the packed counts    [trials::sort_pairs]
//   bins    flag the last trial of every tie run and whether the point after it can be a vertex (pav_flag), scan the
//           flags, compact the candidates into points (x = trials, y = targets up to there)
//   hull    level 0: one thread per chunk of kChunk points scans it in place (monotone chain); then ceil(log2(chunks))
//           levels of (bridge: one thread per pair of adjacent hulls, nested bisection on int64 cross products | copy:
//           one thread per surviving point, L[0 .. l*] ++ R[r* ..) to the left child's base of the other buffer)
//   finish  block table (lo, hi, n, t, llr) and, in one workgroup with fixed-order fp64 sums, min Cllr and the ROCCH EER
// The integer logic is csrc/nplda_pav_core.h, shared with the host replay tests/c/pav_core_host.cpp.
#include <hip/hip_runtime.h>

#include "nplda_pav_core.h"
#include "nplda_trials.h"

namespace {

constexpr int kChunk = 32;         // points per level-0 thread
constexpr int kMaxBlocks = 4096;   // grid cap of the grid-stride kernels
constexpr double kInv2Ln2 = 0.72134752044448170368;  // 1 / (2 ln 2)

// y0 + w * d with the product rounded before the sum, as the definition (and a host reference) evaluates it: the
// compiler's default contraction would fuse the two, and __dmul_rn / __dadd_rn are plain operators to it
__device__ __forceinline__ double lerp_unfused(double y0, double w, double d) {
#pragma clang fp contract(off)
    const double step = w * d;
    return y0 + step;
}

struct Meta {
    long long nk, nt, nn, bins, m;  // kept trials, targets, non-targets, tie runs, hull input points
};

struct Grid {
    unsigned blocks;
    long long trips;  // iterations of the grid-stride loop: counted on the host from N
};
Grid grid_for(long long work) {
    long long b = (work + 255) / 256;
    if (b < 1) b = 1;
    Grid g;
    g.blocks = (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
    g.trips = (work + (long long)g.blocks * 256 - 1) / ((long long)g.blocks * 256);
    if (g.trips < 1) g.trips = 1;
    return g;
}

template <class T>
__global__ __launch_bounds__(256) void pav_label_kernel(const T* __restrict__ s, const float* __restrict__ t, long long n,
                                                        long long trips, T* __restrict__ key,
                                                        unsigned long long* __restrict__ lab) {
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < trips; ++it, i += stride) {
        if (i >= n) return;
        trials::key_and_count<trials::Excluded::kNanKey>(s[i], t[i], key[i], lab[i]);
    }
}

__device__ __forceinline__ unsigned long long total_of(const unsigned long long* __restrict__ pref,
                                                       const unsigned long long* __restrict__ val, long long n) {
    return pref[n - 1] + val[n - 1];
}

template <class T>
__global__ __launch_bounds__(256) void pav_flag_kernel(const T* __restrict__ key, const unsigned long long* __restrict__ lab,
                                                       const unsigned long long* __restrict__ pref, long long n,
                                                       long long trips, int filter, unsigned long long* __restrict__ flag) {
    const unsigned long long tot = total_of(pref, lab, n);
    const long long nk = (long long)(tot >> 32) + (long long)(tot & 0xffffffffull);
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < trips; ++it, i += stride) {
        if (i >= n) return;
        flag[i] = pav_flag<T>(key, (const uint64_t*)lab, (const uint64_t*)pref, nk, i, filter);
    }
}

// points: [P_0] [the dummy bin's end] candidates ... [P_M + second dummy bin]; with the Laplace rule every real point is
// shifted by the (2, 1) of the dummy bin in front
__global__ __launch_bounds__(256) void pav_point_kernel(const unsigned long long* __restrict__ lab,
                                                        const unsigned long long* __restrict__ pref,
                                                        const unsigned long long* __restrict__ flag,
                                                        const unsigned long long* __restrict__ fpref, long long n,
                                                        long long trips, int laplace, PavPt* __restrict__ pts,
                                                        Meta* __restrict__ meta) {
    const long long stride = (long long)gridDim.x * 256;
    const unsigned lead = laplace ? 2u : 1u, xo = laplace ? 2u : 0u, yo = laplace ? 1u : 0u;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        const unsigned long long tot = total_of(pref, lab, n), ftot = total_of(fpref, flag, n);
        const long long nt = (long long)(tot >> 32), nn = (long long)(tot & 0xffffffffull);
        const long long cand = (long long)(ftot & 0xffffffffull);
        pts[0] = PavPt{0u, 0u};
        if (laplace) {
            pts[1] = PavPt{2u, 1u};
            pts[2 + cand] = PavPt{(unsigned)(nt + nn) + 4u, (unsigned)nt + 2u};
        }
        meta->nk = nt + nn;
        meta->nt = nt;
        meta->nn = nn;
        meta->bins = (long long)(ftot >> 32);
        meta->m = cand + (laplace ? 3 : 1);
    }
    for (long long it = 0; it < trips; ++it, i += stride) {
        if (i >= n) return;
        if (!(flag[i] & 1ull)) continue;
        const long long idx = (long long)(fpref[i] & 0xffffffffull);
        pts[lead + idx] = PavPt{(unsigned)(i + 1) + xo, (unsigned)((pref[i] + lab[i]) >> 32) + yo};
    }
}

__global__ __launch_bounds__(256) void pav_chunk_kernel(PavPt* __restrict__ pts, const Meta* __restrict__ meta,
                                                        long long chunks, long long trips, int* __restrict__ cnt) {
    const long long m = meta->m;
    const long long stride = (long long)gridDim.x * 256;
    long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < trips; ++it, c += stride) {
        if (c >= chunks) return;
        const long long b0 = c * kChunk;
        const long long n = b0 >= m ? 0 : (m - b0 < kChunk ? m - b0 : kChunk);
        cnt[c] = n > 0 ? pav_chunk_scan(pts + b0, (int)n) : 0;
    }
}

__global__ __launch_bounds__(256) void pav_bridge_kernel(const PavPt* __restrict__ src, const int* __restrict__ csrc,
                                                         long long nsrc, long long groups, long long span, long long trips,
                                                         PavBridge* __restrict__ br, int* __restrict__ cdst) {
    const long long stride = (long long)gridDim.x * 256;
    long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < trips; ++it, g += stride) {
        if (g >= groups) return;
        const int kl = csrc[2 * g];
        const int kr = 2 * g + 1 < nsrc ? csrc[2 * g + 1] : 0;
        const PavBridge b = pav_bridge(src + g * span, kl, src + g * span + (span >> 1), kr);
        br[g] = b;
        cdst[g] = pav_merged_count(b);
    }
}

__global__ __launch_bounds__(256) void pav_copy_kernel(const PavPt* __restrict__ src, PavPt* __restrict__ dst,
                                                       const PavBridge* __restrict__ br, const Meta* __restrict__ meta,
                                                       int level, long long trips) {
    const long long m = meta->m;
    const long long span = pav_span(kChunk, level);
    const long long stride = (long long)gridDim.x * 256;
    long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < trips; ++it, p += stride) {
        if (p >= m) return;
        const long long g = p >> (level + 5), e = p - g * span;  // kChunk = 32 = 1 << 5
        const long long s = pav_merged_src(br[g], span, e);
        if (s >= 0) dst[p] = src[g * span + s];
    }
}
static_assert(kChunk == 32, "pav_copy_kernel shifts by level + 5");

template <class T>
struct TableArgs {
    const T* key;
    const PavPt* hull;
    const int* count;
    const Meta* meta;
    int laplace;
    long long cap, trips;
    double *lo, *hi, *llr;
    long long *n, *t;
};

template <class T>
__global__ __launch_bounds__(256) void pav_table_kernel(const TableArgs<T> a) {
    const long long nb = (long long)a.count[0] - 1;
    const long long lim = nb < a.cap ? nb : a.cap;
    const long long nk = a.meta->nk;
    const long long off = a.laplace ? 2 : 0;
    const double prior = log((double)(a.meta->nt + off) / (double)(a.meta->nn + off));
    const long long stride = (long long)gridDim.x * 256;
    long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < a.trips; ++it, b += stride) {
        if (b >= lim) return;
        const PavPt p = a.hull[b], q = a.hull[b + 1];
        const long long n = (long long)q.x - (long long)p.x, t = (long long)q.y - (long long)p.y;
        long long i0 = (long long)p.x - off, i1 = (long long)q.x - off;
        if (i0 < 0) i0 = 0;
        if (i1 > nk) i1 = nk;
        double lo, hi;
        if (i1 > i0) {  // the block's real bins
            lo = (double)a.key[i0];
            hi = (double)a.key[i1 - 1];
        } else {  // dummy bins alone: the one at -inf, the one at +inf, or (no trial kept at all) both
            lo = p.x == 0u ? -INFINITY : INFINITY;
            hi = (long long)q.x == nk + 4 ? INFINITY : -INFINITY;
        }
        a.lo[b] = lo;
        a.hi[b] = hi;
        a.n[b] = n;
        a.t[b] = t;
        a.llr[b] = log((double)t / (double)(n - t)) - prior;
    }
}

struct FinishArgs {
    const PavPt* hull;
    const int* count;
    const Meta* meta;
    int laplace;
    long long cap;
    double* summary;
};

// one workgroup: every thread sums the blocks b = tid, tid + 256, ... in that order, then a fixed LDS tree
__global__ __launch_bounds__(256) void pav_finish_kernel(const FinishArgs a) {
    __shared__ double red[2][256];
    const int nv = a.count[0];
    const long long nb = (long long)nv - 1;
    const long long off = a.laplace ? 2 : 0;
    const long long Nt = a.meta->nt + off, Nn = a.meta->nn + off;
    const bool both = a.meta->nt > 0 && a.meta->nn > 0;
    const double rt = (double)Nt / (double)Nn, rn = (double)Nn / (double)Nt;
    double st = 0.0, sn = 0.0;
    const long long per = (nb + 255) / 256;
    long long b = threadIdx.x;
    for (long long it = 0; it < per; ++it, b += 256) {
        if (b >= nb) break;
        const PavPt p = a.hull[b], q = a.hull[b + 1];
        const double n = (double)((long long)q.x - (long long)p.x), t = (double)((long long)q.y - (long long)p.y);
        const double f = n - t;
        if (t > 0.0) st += t * log1p(f / t * rt);
        if (f > 0.0) sn += f * log1p(t / f * rn);
    }
    red[0][threadIdx.x] = st;
    red[1][threadIdx.x] = sn;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double mc = NAN, eer = NAN;
    if (both && nv >= 2) {
        mc = kInv2Ln2 * (red[0][0] / (double)Nt + red[1][0] / (double)Nn);
        // d_v = T_v / N_t - 1 + F_v / N_n rises strictly from -1 to 1 along the hull; its sign is decided exactly:
        // d_v < 0  <=>  T_v N_n + F_v N_t < N_t N_n  (all below 2^64)
        const unsigned long long unt = (unsigned long long)Nt, unn = (unsigned long long)Nn;
        int lo = 1, hi = nv - 1;  // first v with d_v >= 0: d_0 = -1, d_{nv - 1} = 1
        for (int step = 0; step < 64 && lo < hi; ++step) {
            const int mid = lo + ((hi - lo) >> 1);
            const PavPt p = a.hull[mid];
            const unsigned long long T = p.y, F = (unsigned long long)p.x - p.y;
            if (T * unn + F * unt >= unt * unn) hi = mid;
            else lo = mid + 1;
        }
        const PavPt p = a.hull[lo - 1], q = a.hull[lo];
        const double pm0 = (double)p.y / (double)Nt, pf0 = 1.0 - (double)(p.x - p.y) / (double)Nn;
        const double pm1 = (double)q.y / (double)Nt, pf1 = 1.0 - (double)(q.x - q.y) / (double)Nn;
        const double d0 = pm0 - pf0, d1 = pm1 - pf1;
        const double w = -d0 / (d1 - d0);
        eer = lerp_unfused(pm0, w, pm1 - pm0);
    }
    a.summary[0] = (double)a.meta->nt;
    a.summary[1] = (double)a.meta->nn;
    a.summary[2] = (double)a.meta->bins;
    a.summary[3] = (double)nb;
    a.summary[4] = mc;
    a.summary[5] = eer;
    a.summary[6] = nb > a.cap ? 1.0 : 0.0;
    a.summary[7] = 0.0;
}

template <class T, class O>
__global__ __launch_bounds__(256) void pav_apply_kernel(const T* __restrict__ s, long long n, long long trips,
                                                        const double* __restrict__ lo, const double* __restrict__ hi,
                                                        const double* __restrict__ llr, long long nb, O* __restrict__ out) {
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long it = 0; it < trips; ++it, i += stride) {
        if (i >= n) return;
        const double v = (double)s[i];
        double r;
        if (v != v) {
            r = v;
        } else {
            long long a = 0, z = nb;  // first block with hi >= v, nb when there is none
            for (int step = 0; step < 64 && a < z; ++step) {
                const long long mid = a + ((z - a) >> 1);
                if (hi[mid] >= v) z = mid;
                else a = mid + 1;
            }
            if (a >= nb) {
                r = llr[nb - 1];
            } else if (lo[a] <= v || a == 0) {
                r = llr[a];
            } else {  // hi[a - 1] < v < lo[a]
                const double h = hi[a - 1], l = lo[a], y0 = llr[a - 1], y1 = llr[a];
                if (isinf(h)) r = y0;
                else if (isinf(l)) r = y1;
                else if (isinf(y0)) r = y0;
                else if (isinf(y1)) r = y1;
                else {
                    const double w = (v - h) / (l - h);
                    r = lerp_unfused(y0, w, y1 - y0);
                    r = r < y0 ? y0 : (r > y1 ? y1 : r);
                }
            }
        }
        out[i] = (O)r;
    }
}

struct Plan {
    size_t o_keys_in, o_keys, o_lab_in, o_lab, o_pref, o_fpref, o_ptsa, o_ptsb, o_cnta, o_cntb, o_br, o_meta, o_tmp;
    size_t tmp_bytes, total;
    long long maxpts, chunks;
    int levels;
};

// the sort's and the scans' temporary storage is reserved from N, without a device (trials::sort_reserve_bytes)
void make_plan(long long n, size_t ksz, Plan* p) {
    const size_t nn = (size_t)n;
    p->maxpts = n + 4;
    p->chunks = pav_hulls(p->maxpts, kChunk, 0);
    p->levels = pav_levels(p->maxpts, kChunk);
    size_t o = 0;
    p->o_keys_in = o; o += up256(nn * ksz);
    p->o_keys = o; o += up256(nn * ksz);
    p->o_lab_in = o; o += up256(nn * 8);  // reused for the bin flags once the sort has read it
    p->o_lab = o; o += up256(nn * 8);
    p->o_pref = o; o += up256(nn * 8);
    p->o_fpref = o; o += up256(nn * 8);
    p->o_ptsa = o; o += up256((size_t)p->maxpts * sizeof(PavPt));
    p->o_ptsb = o; o += up256((size_t)p->maxpts * sizeof(PavPt));
    p->o_cnta = o; o += up256((size_t)p->chunks * sizeof(int));
    p->o_cntb = o; o += up256((size_t)p->chunks * sizeof(int));
    p->o_br = o; o += up256((size_t)pav_hulls(p->maxpts, kChunk, 1) * sizeof(PavBridge));
    p->o_meta = o; o += up256(sizeof(Meta));
    p->tmp_bytes = trials::sort_reserve_bytes(nn, ksz, 8);
    p->o_tmp = o; o += p->tmp_bytes;
    p->total = o;
}

template <class T>
int pav_fit(const T* scores, const float* target, int64_t N, int laplace, double* lo, double* hi, int64_t* nout,
            int64_t* tout, double* llr, int64_t cap, double* summary, void* workspace, size_t workspace_bytes,
            nplda_stream_t stream, int stop_after = 0) {
    if (!scores || !target || !lo || !hi || !nout || !tout || !llr || !summary || !workspace) return NPLDA_EINVAL;
    if (N < 2 || cap < 1) return NPLDA_EINVAL;
    if (N > 0x7fffffffll) return NPLDA_EUNSUPPORTED;
    if (!nplda_aligned16(workspace) || ((uintptr_t)summary & 7u) || ((uintptr_t)lo & 7u) || ((uintptr_t)hi & 7u) ||
        ((uintptr_t)nout & 7u) || ((uintptr_t)tout & 7u) || ((uintptr_t)llr & 7u) || ((uintptr_t)scores & (sizeof(T) - 1)) ||
        ((uintptr_t)target & 3u))
        return NPLDA_EINVAL;
    Plan p;
    make_plan(N, sizeof(T), &p);
    if (workspace_bytes < p.total) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    T* keys_in = (T*)(ws + p.o_keys_in);
    T* keys = (T*)(ws + p.o_keys);
    unsigned long long* lab_in = (unsigned long long*)(ws + p.o_lab_in);
    unsigned long long* lab = (unsigned long long*)(ws + p.o_lab);
    unsigned long long* pref = (unsigned long long*)(ws + p.o_pref);
    unsigned long long* flag = lab_in;
    unsigned long long* fpref = (unsigned long long*)(ws + p.o_fpref);
    PavPt* pts[2] = {(PavPt*)(ws + p.o_ptsa), (PavPt*)(ws + p.o_ptsb)};
    int* cnt[2] = {(int*)(ws + p.o_cnta), (int*)(ws + p.o_cntb)};
    PavBridge* br = (PavBridge*)(ws + p.o_br);
    Meta* meta = (Meta*)(ws + p.o_meta);
    const Grid gn = grid_for(N);
    hipLaunchKernelGGL(pav_label_kernel<T>, dim3(gn.blocks), dim3(256), 0, st, scores, target, (long long)N, gn.trips,
                       keys_in, lab_in);
    if (int rc = nplda_launch_status()) return rc;
    if (int rc = trials::sort_pairs(ws + p.o_tmp, p.tmp_bytes, keys_in, keys, lab_in, lab, pref, (size_t)N, st)) return rc;
    if (stop_after == 1) return NPLDA_OK;
    hipLaunchKernelGGL(pav_flag_kernel<T>, dim3(gn.blocks), dim3(256), 0, st, (const T*)keys,
                       (const unsigned long long*)lab, (const unsigned long long*)pref, (long long)N, gn.trips, 1, flag);
    if (int rc = nplda_launch_status()) return rc;
    if (int rc = trials::exclusive_scan(ws + p.o_tmp, p.tmp_bytes, flag, fpref, (size_t)N, st)) return rc;
    hipLaunchKernelGGL(pav_point_kernel, dim3(gn.blocks), dim3(256), 0, st, (const unsigned long long*)lab,
                       (const unsigned long long*)pref, (const unsigned long long*)flag, (const unsigned long long*)fpref,
                       (long long)N, gn.trips, laplace ? 1 : 0, pts[0], meta);
    if (int rc = nplda_launch_status()) return rc;
    if (stop_after == 2) return NPLDA_OK;
    const Grid gc = grid_for(p.chunks);
    hipLaunchKernelGGL(pav_chunk_kernel, dim3(gc.blocks), dim3(256), 0, st, pts[0], (const Meta*)meta, p.chunks, gc.trips,
                       cnt[0]);
    if (int rc = nplda_launch_status()) return rc;
    const Grid gp = grid_for(p.maxpts);
    int cur = 0;
    for (int L = 1; L <= p.levels; ++L) {
        const long long groups = pav_hulls(p.maxpts, kChunk, L), nsrc = pav_hulls(p.maxpts, kChunk, L - 1);
        const Grid gg = grid_for(groups);
        hipLaunchKernelGGL(pav_bridge_kernel, dim3(gg.blocks), dim3(256), 0, st, (const PavPt*)pts[cur],
                           (const int*)cnt[cur], nsrc, groups, (long long)pav_span(kChunk, L), gg.trips, br, cnt[cur ^ 1]);
        if (int rc = nplda_launch_status()) return rc;
        hipLaunchKernelGGL(pav_copy_kernel, dim3(gp.blocks), dim3(256), 0, st, (const PavPt*)pts[cur], pts[cur ^ 1],
                           (const PavBridge*)br, (const Meta*)meta, L, gp.trips);
        if (int rc = nplda_launch_status()) return rc;
        cur ^= 1;
    }
    if (stop_after == 3) return NPLDA_OK;
    TableArgs<T> ta;
    ta.key = keys; ta.hull = pts[cur]; ta.count = cnt[cur]; ta.meta = meta; ta.laplace = laplace ? 1 : 0; ta.cap = cap;
    ta.lo = lo; ta.hi = hi; ta.llr = llr; ta.n = (long long*)nout; ta.t = (long long*)tout;
    const long long tw = cap < p.maxpts ? cap : p.maxpts;
    const Grid gt = grid_for(tw);
    ta.trips = gt.trips;
    hipLaunchKernelGGL(pav_table_kernel<T>, dim3(gt.blocks), dim3(256), 0, st, ta);
    if (int rc = nplda_launch_status()) return rc;
    FinishArgs fa;
    fa.hull = pts[cur]; fa.count = cnt[cur]; fa.meta = meta; fa.laplace = laplace ? 1 : 0; fa.cap = cap; fa.summary = summary;
    hipLaunchKernelGGL(pav_finish_kernel, dim3(1), dim3(256), 0, st, fa);
    return nplda_launch_status();
}

template <class T>
int pav_apply(const T* scores, int64_t N, const double* lo, const double* hi, const double* llr, int64_t nb, void* out,
              int out_f64, nplda_stream_t stream) {
    if (N < 0 || nb < 1 || !lo || !hi || !llr) return NPLDA_EINVAL;
    if (N > 0x7fffffffll || nb > 0x7fffffffll) return NPLDA_EUNSUPPORTED;
    if (((uintptr_t)lo & 7u) || ((uintptr_t)hi & 7u) || ((uintptr_t)llr & 7u)) return NPLDA_EINVAL;
    if (N == 0) return NPLDA_OK;
    if (!scores || !out || ((uintptr_t)scores & (sizeof(T) - 1)) || ((uintptr_t)out & (out_f64 ? 7u : 3u)))
        return NPLDA_EINVAL;
    const Grid g = grid_for(N);
    hipStream_t st = (hipStream_t)stream;
    if (out_f64)
        hipLaunchKernelGGL((pav_apply_kernel<T, double>), dim3(g.blocks), dim3(256), 0, st, scores, (long long)N, g.trips, lo,
                           hi, llr, (long long)nb, (double*)out);
    else
        hipLaunchKernelGGL((pav_apply_kernel<T, float>), dim3(g.blocks), dim3(256), 0, st, scores, (long long)N, g.trips, lo,
                           hi, llr, (long long)nb, (float*)out);
    return nplda_launch_status();
}

}  // namespace

extern "C" {

int nplda_pav_chunk(void) { return kChunk; }

size_t nplda_pav_workspace_bytes(int64_t N, int is_f64) {
    if (N < 2 || N > 0x7fffffffll) return 0;
    Plan p;
    make_plan(N, is_f64 ? sizeof(double) : sizeof(float), &p);
    return p.total;
}

int nplda_pav_fit_f32(const float* scores, const float* target, int64_t N, int laplace, double* lo, double* hi, int64_t* n,
                      int64_t* t, double* llr, int64_t cap, double* summary, void* workspace, size_t workspace_bytes,
                      nplda_stream_t stream) {
    return pav_fit<float>(scores, target, N, laplace, lo, hi, n, t, llr, cap, summary, workspace, workspace_bytes, stream);
}

int nplda_pav_fit_f64(const double* scores, const float* target, int64_t N, int laplace, double* lo, double* hi, int64_t* n,
                      int64_t* t, double* llr, int64_t cap, double* summary, void* workspace, size_t workspace_bytes,
                      nplda_stream_t stream) {
    return pav_fit<double>(scores, target, N, laplace, lo, hi, n, t, llr, cap, summary, workspace, workspace_bytes, stream);
}

int nplda_pav_fit_stages_f32(const float* scores, const float* target, int64_t N, int laplace, double* lo, double* hi,
                             int64_t* n, int64_t* t, double* llr, int64_t cap, double* summary, void* workspace,
                             size_t workspace_bytes, int stop_after, nplda_stream_t stream) {
    if (stop_after < 0 || stop_after > 3) return NPLDA_EINVAL;
    return pav_fit<float>(scores, target, N, laplace, lo, hi, n, t, llr, cap, summary, workspace, workspace_bytes, stream,
                          stop_after);
}

int nplda_pav_apply_f32(const float* scores, int64_t N, const double* lo, const double* hi, const double* llr, int64_t nb,
                        void* out, int out_f64, nplda_stream_t stream) {
    return pav_apply<float>(scores, N, lo, hi, llr, nb, out, out_f64, stream);
}

int nplda_pav_apply_f64(const double* scores, int64_t N, const double* lo, const double* hi, const double* llr, int64_t nb,
                        void* out, int out_f64, nplda_stream_t stream) {
    return pav_apply<double>(scores, N, lo, hi, llr, nb, out, out_f64, stream);
}

}  // extern "C"
