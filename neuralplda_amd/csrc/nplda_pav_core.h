// nplda_pav_core.h — the integer logic of the PAV / ROC-convex-hull kernels (csrc/nplda_pav.hip, design/k18_pav_rocch.md)
// as __host__ __device__ functions: the same text runs in the kernels and in tests/c/pav_core_host.cpp, which replays the
// whole chunk scan + merge tree serially on the host against an O(n) stack.
//
// Objects.  A point is a cumulative (trials, targets) count; points are sorted by x, strictly increasing.  The strict lower
// convex hull of a run of points is kept as a contiguous array of points.  Level 0 cuts the array into chunks of C points
// and scans each one (monotone chain, in place); level L >= 1 merges hulls 2g and 2g + 1 of level L - 1, which sit at
// g * span(L) and g * span(L) + span(L) / 2 with span(L) = C << L, into one hull at g * span(L) of the other buffer.
// Every coordinate is below 2^31 + 4, so every cross product is exact in int64: no floating point takes part.
// Every loop has a counted bound (binary searches: at most 64 steps).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PAV_HD __host__ __device__ inline
#else
#define PAV_HD inline
#endif

struct PavPt {
    uint32_t x, y;  // trials, targets up to and including this bin
};

struct PavBridge {
    int32_t l, r, kl, kr;  // merged hull = L[0 .. l] ++ R[r .. kr)
};

// cross(b - a, c - b): > 0 iff a -> b -> c turns left (b lies strictly below the chord a c)
PAV_HD int64_t pav_cross(PavPt a, PavPt b, PavPt c) {
    const int64_t ux = (int64_t)b.x - (int64_t)a.x, uy = (int64_t)b.y - (int64_t)a.y;
    const int64_t vx = (int64_t)c.x - (int64_t)b.x, vy = (int64_t)c.y - (int64_t)b.y;
    return ux * vy - uy * vx;
}

// Monotone chain over p[0 .. n), in place (the stack never passes the read position): pop the top b while
// cross(b - a, c - b) <= 0.  Returns the number of hull points, which are left in p[0 .. count).
PAV_HD int pav_chunk_scan(PavPt* p, int n) {
    int k = 0;
    for (int i = 0; i < n; ++i) {
        const PavPt c = p[i];
        // at most i pops in total over the whole scan; each step of this loop removes one point
        for (int guard = 0; guard < n && k >= 2; ++guard) {
            if (pav_cross(p[k - 2], p[k - 1], c) > 0) break;
            --k;
        }
        p[k++] = c;
    }
    return k;
}

// Tangent from a point l left of the hull R[0 .. kr), kr >= 1: the first j with l -> R[j] -> R[j + 1] turning left,
// kr - 1 when there is none.  The slope from l to R[j] falls strictly, then rises strictly (R is strictly convex), so the
// predicate is monotone in j; of two collinear candidates the farther one is taken (the nearer would not be a vertex).
PAV_HD int pav_tangent(PavPt l, const PavPt* R, int kr) {
    int lo = 0, hi = kr - 1;  // answer in [lo, hi]
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pav_cross(l, R[mid], R[mid + 1]) > 0) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Common lower tangent of two adjacent hulls, L[0 .. kl) entirely left of R[0 .. kr).  l* is the first i for which R does
// NOT lie strictly above the line of edge (L[i], L[i + 1]) — then the hull turns towards R at L[i] — and kl - 1 when
// there is none; "R strictly above the edge line" is "the tangent point from L[i] is", and is monotone in i because the
// edge slopes rise.  r* is the tangent point from L[l*].  kr == 0 (no right neighbour) keeps L whole.
PAV_HD PavBridge pav_bridge(const PavPt* L, int kl, const PavPt* R, int kr) {
    PavBridge b;
    b.kl = kl;
    b.kr = kr;
    if (kl <= 0) {  // nothing on the left: cannot happen for adjacent runs unless both are empty
        b.l = -1;
        b.r = 0;
        return b;
    }
    if (kr <= 0) {
        b.l = kl - 1;
        b.r = 0;
        return b;
    }
    int lo = 0, hi = kl - 1;  // answer in [lo, hi]
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        const int r = pav_tangent(L[mid], R, kr);
        // cross(b - a, c - b) == cross(b - a, c - a): <= 0 iff R[r] lies on or below the extended edge
        if (pav_cross(L[mid], L[mid + 1], R[r]) <= 0) hi = mid;
        else
            lo = mid + 1;
    }
    b.l = lo;
    b.r = pav_tangent(L[lo], R, kr);
    return b;
}

// ---- index arithmetic of the merge tree ------------------------------------------------------------------------------

PAV_HD int64_t pav_span(int C, int level) { return (int64_t)C << level; }

// hulls at `level` (0 = chunks) that an array with room for maxpts points holds
PAV_HD int64_t pav_hulls(int64_t maxpts, int C, int level) {
    const int64_t s = pav_span(C, level);
    return (maxpts + s - 1) / s;
}

// merge levels until one hull is left: the smallest L with C << L >= maxpts
PAV_HD int pav_levels(int64_t maxpts, int C) {
    int L = 0;
    for (; L < 62 && pav_span(C, L) < maxpts; ++L) {
    }
    return L;
}

PAV_HD int pav_merged_count(PavBridge b) { return b.l + 1 + (b.kr - b.r); }

// Source slot (relative to the group's base, span = the MERGED span) of slot e of the merged hull, -1 past its end.
PAV_HD int64_t pav_merged_src(PavBridge b, int64_t span, int64_t e) {
    if (e <= b.l) return e;
    const int64_t j = (int64_t)b.r + (e - b.l - 1);
    return j < b.kr ? (span >> 1) + j : -1;
}

// ---- binning: which sorted positions end a tie run, and which of those can be a vertex -------------------------------
// key: sorted scores of the nk kept trials; lab: packed labels (target << 32 | non-target); pref: exclusive prefix sums
// of lab.  Returns (1 << 32) for the last trial of a tie run, + 1 when the point after it is a hull candidate: the last
// bin's always is; any other vertex has a smaller slope before it than after it, so the bin before it holds a non-target
// and the bin after it a target.  Tie runs are walked by a doubling search followed by a bisection, both counted.

template <class K>
PAV_HD int64_t pav_run_end(const K* key, int64_t nk, int64_t i) {  // last index of the tie run that starts at i
    const K v = key[i];
    int64_t step = 1, lo = i, hi = nk;  // key[lo] == v; hi: key[hi] != v or hi == nk
    for (int g = 0; g < 40; ++g) {
        const int64_t q = i + step;
        if (q >= nk) break;
        if (key[q] == v) {
            lo = q;
            step <<= 1;
        } else {
            hi = q;
            break;
        }
    }
    for (int g = 0; g < 64 && hi - lo > 1; ++g) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] == v) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <class K>
PAV_HD int64_t pav_run_start(const K* key, int64_t i) {  // first index of the tie run that ends at i
    const K v = key[i];
    int64_t step = 1, hi = i, lo = -1;  // key[hi] == v; lo: key[lo] != v or lo == -1
    for (int g = 0; g < 40; ++g) {
        const int64_t q = i - step;
        if (q < 0) break;
        if (key[q] == v) {
            hi = q;
            step <<= 1;
        } else {
            lo = q;
            break;
        }
    }
    for (int g = 0; g < 64 && hi - lo > 1; ++g) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] == v) hi = mid;
        else lo = mid;
    }
    return hi;
}

template <class K>
PAV_HD uint64_t pav_flag(const K* key, const uint64_t* lab, const uint64_t* pref, int64_t nk, int64_t i, int filter) {
    if (i >= nk) return 0;
    if (i == nk - 1) return (1ull << 32) | 1ull;
    if (key[i + 1] == key[i]) return 0;
    if (!filter) return (1ull << 32) | 1ull;
    bool non_before = (lab[i] & 0xffffffffull) != 0;
    if (!non_before) {
        const int64_t s = pav_run_start(key, i);
        non_before = ((pref[i] + lab[i]) & 0xffffffffull) != (pref[s] & 0xffffffffull);
    }
    if (!non_before) return 1ull << 32;
    bool tgt_after = (lab[i + 1] >> 32) != 0;
    if (!tgt_after) {
        const int64_t e = pav_run_end(key, nk, i + 1);
        tgt_after = ((pref[e] + lab[e]) >> 32) != (pref[i + 1] >> 32);
    }
    return (1ull << 32) | (tgt_after ? 1ull : 0ull);
}
