// nplda_ragged.h — the layout of P ragged problems per call: a table of P + 1 offsets (two tables side by side where a problem
// has two lengths), and per-problem regions of the outputs and the workspace packed in problem order.
//
// A family states what a problem of a given length takes ONCE, as a functor
//     __host__ __device__ void operator()(long long na, long long nb, long long* terms /* [K] */) const
// (elements, records, workspace bytes, ...): its host plan sums the terms to size the buffers, its kernels sum them over the
// problems in front of theirs to find their regions, so the two cannot disagree.  A one-table family passes its table twice
// to the walk and gets its one length in both places.
#pragma once
#include "nplda_common.h"

// Host: the checks every family makes on its tables, then each(na, nb) per problem, in order, until one returns a status
// other than NPLDA_OK.  Limits on the lengths and the totals are the caller's, inside `each`.
template <class Each>
inline int ragged_walk(const int64_t* a, const int64_t* b, int64_t P, long long max_P, Each each) {
    if (P < 0 || (P > 0 && (!a || !b))) return NPLDA_EINVAL;
    if (P > max_P) return NPLDA_EUNSUPPORTED;
    if (P > 0 && (a[0] != 0 || b[0] != 0)) return NPLDA_EINVAL;
    for (int64_t p = 0; p < P; ++p) {
        const long long na = a[p + 1] - a[p], nb = b[p + 1] - b[p];
        if (na < 0 || nb < 0) return NPLDA_EINVAL;
        const int status = each(na, nb);
        if (status != NPLDA_OK) return status;
    }
    return NPLDA_OK;
}

// Device: sums[k] = the sum of term k over the problems in front of p of a one-table family, on every thread, by the whole
// block (any block size that is a multiple of 64, at most 1024).  Integers: exact in any order.  One barrier; `red` is 16 K
// words of LDS, slot 16 k + wave.
template <int K, class Terms>
__device__ __forceinline__ void ragged_starts(const long long* __restrict__ offs, long long p, const Terms terms,
                                              long long* red /* [16 * K] */, long long (&sums)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) sums[k] = 0;
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long q = threadIdx.x; q < p; q += 64 * nw) {
        const long long n = offs[q + 1] - offs[q];
        long long t[K];
        terms(n, n, t);
#pragma unroll
        for (int k = 0; k < K; ++k) sums[k] += t[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        sums[k] = wave_sum(sums[k]);
        if ((threadIdx.x & 63) == 0) red[16 * k + wave] = sums[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {  // (a loop per term: a kernel that uses one start keeps one loop)
        long long s = 0;
        for (int w = 0; w < nw; ++w) s += red[16 * k + w];
        sums[k] = s;
    }
}
