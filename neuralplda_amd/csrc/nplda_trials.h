// nplda_trials.h — what the score-evaluation families (nplda_detcost, nplda_pav, nplda_bootstrap, nplda_calib) share:
// the rule "which trial counts, and as what", and the host front end of their device sort and prefix scan
// (nplda_trials.hip, the one translation unit that instantiates the sort library).
#pragma once
#include "nplda_common.h"

namespace trials {

// ---- the trial rule ---------------------------------------------------------------------------------------------------
// The class of a label (utils/models.py:407-408): target iff t > 0.5, non-target iff t < 0.5; 0.5 and NaN are in neither.
enum : int { kNeither = -1, kNonTarget = 0, kTarget = 1 };
__host__ __device__ inline int label_class(float t) { return t > 0.5f ? kTarget : (t < 0.5f ? kNonTarget : kNeither); }

// (target << 32) | non-target: ONE 64-bit prefix sum over these carries both class counts.
__host__ __device__ inline unsigned long long packed_count(int cls) {
    return cls == kTarget ? (1ull << 32) : (cls == kNonTarget ? 1ull : 0ull);
}

// The canonical positive NaN, the sort key of a trial that must not be met by a search: the radix sort puts it behind
// +inf, so such trials form the tail of the sorted array, where `<` and `==` stay monotone.  (A NaN with the sign bit set
// would sort in front of -inf and break every binary search: a NaN score never keeps its own bits as a key.)
template <class T> __device__ __forceinline__ T nan_key();
template <> __device__ __forceinline__ float nan_key<float>() { return __uint_as_float(0x7fc00000u); }
template <> __device__ __forceinline__ double nan_key<double>() { return __longlong_as_double(0x7ff8000000000000ll); }

// The sort key of a trial that its LABEL excludes (a NaN score always gets nan_key):
//   kKeepScore  its score: it stays a candidate threshold among the kept trials (nplda_detcost)
//   kNanKey     nan_key: it joins the tail (nplda_pav, whose bins hold kept trials only)
enum class Excluded { kKeepScore, kNanKey };

// (score, label) -> (sort key, packed count).  A NaN score removes the trial whatever its label.
template <Excluded POLICY, class T>
__device__ __forceinline__ void key_and_count(T score, float label, T& key, unsigned long long& count) {
    const bool nan = score != score;
    count = nan ? 0ull : packed_count(label_class(label));
    key = (POLICY == Excluded::kKeepScore ? !nan : count != 0ull) ? score : nan_key<T>();
}

// first position of the ascending keys with key >= v
__device__ __forceinline__ long long lower_bound(const float* __restrict__ key, long long n, float v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- sort and scan: the host front end --------------------------------------------------------------------------------
// The sort library's own size queries need a device; a workspace plan must not (it is part of argument checking).  So the
// temporary storage is RESERVED from n alone — room for the sort's alternate (key, value) buffers, its per-block digit
// counters and the scan's look-back states — and every call below checks the library's actual request against the
// reservation (NPLDA_ENOSPC when it is larger) before it enqueues anything.
inline size_t sort_reserve_bytes(size_t n, size_t key_bytes, size_t value_bytes) {
    return up256(n * (key_bytes + value_bytes) + 2 * n + ((size_t)4 << 20));
}

// Stable ascending sort of n (key, value) pairs on all key bits.  With `prefix` the exclusive prefix sums of the sorted
// values follow.  `tmp` holds `reserved` bytes.  Returns NPLDA_OK, NPLDA_ENOSPC or a HIP error.
int sort_pairs(void* tmp, size_t reserved, const float* key_in, float* key, const unsigned long long* val_in,
               unsigned long long* val, unsigned long long* prefix, size_t n, hipStream_t stream);
int sort_pairs(void* tmp, size_t reserved, const double* key_in, double* key, const unsigned long long* val_in,
               unsigned long long* val, unsigned long long* prefix, size_t n, hipStream_t stream);
int sort_pairs(void* tmp, size_t reserved, const float* key_in, float* key, const unsigned* val_in, unsigned* val, size_t n,
               hipStream_t stream);

// out[i] = in[0] + ... + in[i - 1]
int exclusive_scan(void* tmp, size_t reserved, const unsigned long long* in, unsigned long long* out, size_t n,
                   hipStream_t stream);

}  // namespace trials
