// The device sort and prefix scan of the score-evaluation families (nplda_trials.h): rocPRIM — the plain-library part,
// like a library GEMM — instantiated here once for every (key, value) pair in use.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "nplda_trials.h"

namespace trials {

namespace {

using u64 = unsigned long long;

// rocPRIM with a null temporary pointer returns its request in `bytes` and enqueues nothing
template <class K, class V>
int sort_at(void* tmp, size_t& bytes, const K* key_in, K* key, const V* val_in, V* val, size_t n, hipStream_t st) {
    return (int)rocprim::radix_sort_pairs(tmp, bytes, key_in, key, val_in, val, n, 0, 8 * sizeof(K), st);
}

int scan_at(void* tmp, size_t& bytes, const u64* in, u64* out, size_t n, hipStream_t st) {
    return (int)rocprim::exclusive_scan(tmp, bytes, in, out, 0ull, n, rocprim::plus<u64>(), st);
}

template <class K, class V>
int checked_sort(void* tmp, size_t reserved, const K* key_in, K* key, const V* val_in, V* val, size_t n, hipStream_t st) {
    size_t bytes = 0;
    if (int rc = sort_at(nullptr, bytes, key_in, key, val_in, val, n, st)) return rc;
    if (bytes > reserved) return NPLDA_ENOSPC;
    bytes = reserved;
    return sort_at(tmp, bytes, key_in, key, val_in, val, n, st);
}

template <class K>
int sort_then_scan(void* tmp, size_t reserved, const K* key_in, K* key, const u64* val_in, u64* val, u64* prefix, size_t n,
                   hipStream_t st) {
    if (int rc = checked_sort(tmp, reserved, key_in, key, val_in, val, n, st)) return rc;
    return prefix ? exclusive_scan(tmp, reserved, val, prefix, n, st) : NPLDA_OK;
}

}  // namespace

int sort_pairs(void* tmp, size_t reserved, const float* key_in, float* key, const u64* val_in, u64* val, u64* prefix,
               size_t n, hipStream_t stream) {
    return sort_then_scan(tmp, reserved, key_in, key, val_in, val, prefix, n, stream);
}

int sort_pairs(void* tmp, size_t reserved, const double* key_in, double* key, const u64* val_in, u64* val, u64* prefix,
               size_t n, hipStream_t stream) {
    return sort_then_scan(tmp, reserved, key_in, key, val_in, val, prefix, n, stream);
}

int sort_pairs(void* tmp, size_t reserved, const float* key_in, float* key, const unsigned* val_in, unsigned* val, size_t n,
               hipStream_t stream) {
    return checked_sort(tmp, reserved, key_in, key, val_in, val, n, stream);
}

int exclusive_scan(void* tmp, size_t reserved, const u64* in, u64* out, size_t n, hipStream_t stream) {
    size_t bytes = 0;
    if (int rc = scan_at(nullptr, bytes, in, out, n, stream)) return rc;
    if (bytes > reserved) return NPLDA_ENOSPC;
    bytes = reserved;
    return scan_at(tmp, bytes, in, out, n, stream);
}

}  // namespace trials
