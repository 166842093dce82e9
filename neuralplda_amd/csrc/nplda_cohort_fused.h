// nplda_cohort_fused.h — host interface of the fused cohort-statistics path (nplda_cohort_fused.hip) for the dispatch
// in nplda_cohort.hip.
#pragma once
#include "nplda_common.h"

namespace nplda {

struct FusedPlan {
    bool eligible;
    int nbands, nx, nsub;             // column bands (a multiple of 8), column tiles, candidate sub-lists per row
    int q, ksub;                      // list bands per column band (a band's columns in q parts, each with its own
                                      // sub-lists), slots per sub-list
    int cap;                          // candidate keys one row may bring to the select kernel (its LDS run)
    float zhi, fhi;                   // proposed candidate fraction fhi and its normal quantile zhi = Phi^-1(fhi)
    size_t fixed_bytes, row_bytes;    // workspace: fixed part and per row (rows are planned in multiples of 128)
    long long max_rows;               // rows one launch may cover (32-bit list offsets)
};

FusedPlan cohort_fused_plan(long long M, int topn, int Mp);

// The fused workspace: its ONE description is the "workspace map" in nplda_cohort_fused.hip; these answer from it.
constexpr int kFallbackBlocks = 64;  // blocks of cohort_fallback_kernel, each with a scratch score row at the workspace's end
constexpr int kFusedFailWord = 8;    // 32-bit word of the workspace that counts the last chunk's rows left to the fallback
// bytes for `rows` rows (a multiple of 128): fixed part + per-row arrays + the scratch rows
size_t fused_workspace_bytes(const FusedPlan& p, long long rows, long long M);
// rows (a multiple of 128, at most p.max_rows) whose arrays a workspace of ws_bytes >= fused_workspace_bytes(p, 128, M) holds
long long fused_rows_cap(const FusedPlan& p, size_t ws_bytes, long long M);
float* fused_scratch_rows(void* ws, size_t ws_bytes, long long M);  // [kFallbackBlocks][M rounded up to 4]

// Blocks of `kernel` resident at once, a multiple of 8 (at least 8) so that a persistent block keeps its XCD; 0: query failed.
template <class K>
inline long long resident_blocks(K kernel, int threads) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess)
        return 0;
    const long long r = (long long)cus * per_cu / 8 * 8;
    return r < 8 ? 8 : r;
}
long long cohort_fused_resident_blocks();

// What cohort_fused_run is asked for: plain host structs, one brace initialiser per group at the call site.
struct CohortRows { const float* z; const float* q; long long R; double* stats; };  // one chunk of the row table
struct CohortTable {
    const float* z; const float* q; long long M, ldz;
    // null, or a CohortState (the fixed part of a workspace in which cohort_fused_prepare has left the cohort's moments):
    // the pre-pass is skipped and the covariance image / moment vectors are read from there
    const unsigned char* prepared;
};
struct CohortModel { const float* P; int ksteps, D2; };  // D2: the embedding dimension (picks the short last k-block)
struct CohortSelect { int topn, lowest; };
struct CohortExec {
    unsigned char* ws; long long rows_cap;  // the workspace and the rows its per-row arrays were carved for
    bool prepass;                           // the cohort's moments are still to be formed (the call's first chunk)
    long long resident; hipStream_t st;
};
struct FusedRequest { CohortRows rows; CohortTable coh; CohortModel net; CohortSelect sel; CohortExec exec; };
// The rows that need the general path (device): the caller runs cohort_fallback_kernel on them.
struct FusedResult { int rc; const unsigned* fail_rows; const unsigned* nfail; };

// Runs the fused path on the chunk's rows (R <= exec.rows_cap).
FusedResult cohort_fused_run(const FusedPlan& p, const FusedRequest& q);
// The cohort-only part of the fused path (Gram matrix + first moments, covariance image folded with P) into `state`
// (plan.fixed_bytes bytes, 256-byte aligned): what every call on the same (model, cohort) would recompute.
int cohort_fused_prepare(const FusedPlan& p, const CohortTable& coh, const CohortModel& net, unsigned char* state, hipStream_t st);

}  // namespace nplda
