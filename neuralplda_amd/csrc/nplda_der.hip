// nplda_der.hip — diarization error rate with the optimal speaker mapping, P ragged problems per call (gfx950).
// design/k24_der.md has the definitions, the phases and what was measured.  Integers only: no floating point anywhere.
//
// Three launches on the caller's stream:
//   der_init_kernel   every frame of every recording: reference mask = 0, flag = (no UEM table ? kInUem : 0);
//   der_paint_kernel  a workgroup per (recording, share of its turns): OR a turn's speaker bit into the 64-bit masks of its
//                     frames, OR kInCollar into the flags of the frames within the collar of its two boundaries, OR kInUem
//                     into the frames of a UEM region.  Integer OR-atomics: the result does not depend on the order;
//   der_count_kernel  ONE workgroup per problem (a recording and one hypothesis for it).  The frames go by in chunks of
//                     kChunk; in the turn form the hypothesis masks of a chunk are painted into LDS first.  A thread walks
//                     kPer CONSECUTIVE frames and adds a run of equal (R, H) to the 64 x 64 matrix in LDS with one integer
//                     atomic per speaker pair and RUN, not per frame; the five counts stay in registers as int64.  Wave 0
//                     then solves the assignment with a column per lane and writes the outputs.
#include "nplda_common.h"

namespace {

constexpr int kDerMaxS = 64;                       // a speaker per bit of the frame masks and per lane of the assignment
constexpr int kDerBlock = 256;                     // threads of the counting workgroup
constexpr int kDerWaves = kDerBlock / 64;
constexpr int kPer = 16;                           // consecutive frames a thread walks per chunk
constexpr int kChunk = kDerBlock * kPer;           // frames per chunk: 4096 (32 KB of hypothesis masks in LDS)
constexpr int kPaintSplit = 8;                     // workgroups that share a recording's turns in der_paint_kernel
constexpr long long kDerMaxT = 0x7fffffffll;       // frames per recording: turn bounds are int32
constexpr long long kDerMaxP = 1ll << 24, kDerMaxR = 1ll << 24;
constexpr long long kDerMaxFrames = 1ll << 40;     // frames per call
constexpr unsigned kInUem = 1u, kInCollar = 2u;    // flag bits; a frame is scored when its flag == kInUem
constexpr int kNCounts = 6;                        // scored, total, miss, fa, sum of min(|R|, |H|), matched

// ---- host: the checks every entry point shares ----------------------------------------------------------------------------------

// P + 1 non-decreasing offsets that start at 0 -> the last one, or -1
long long table_total(const int64_t* o, int64_t n) {
    if (!o || o[0] != 0) return -1;
    for (int64_t i = 0; i < n; ++i)
        if (o[i + 1] < o[i]) return -1;
    return o[n];
}

struct DerPlan {
    int status;
    long long frames;
    size_t mask_bytes, ws_bytes;
};

DerPlan der_plan(const int64_t* frame_offs, int64_t Rn) {
    DerPlan r = {NPLDA_OK, 0, 0, 0};
    if (Rn < 0 || !frame_offs) {
        r.status = NPLDA_EINVAL;
        return r;
    }
    if (Rn > kDerMaxR) {
        r.status = NPLDA_EUNSUPPORTED;
        return r;
    }
    r.frames = table_total(frame_offs, Rn);
    if (r.frames < 0) {
        r.status = NPLDA_EINVAL;
        return r;
    }
    for (int64_t i = 0; i < Rn; ++i)
        if (frame_offs[i + 1] - frame_offs[i] > kDerMaxT) r.status = NPLDA_EUNSUPPORTED;
    if (r.frames > kDerMaxFrames) r.status = NPLDA_EUNSUPPORTED;
    r.mask_bytes = up256((size_t)r.frames * 8);
    r.ws_bytes = r.mask_bytes + up256((size_t)r.frames * 4) + 256;
    return r;
}

// ---- device ------------------------------------------------------------------------------------------------------------------------

struct DerArgs {
    const long long* frame_offs;
    long long Rn, frames;
    const long long* ref_offs;
    const int* ref_turns;
    long long n_ref;
    const long long* uem_offs;
    const int* uem;
    long long n_uem;
    int collar, skip_overlap, S_ref, S_hyp;
    const int* prob_reco;
    const long long* hyp_offs;  // the turn form, or null
    const int* hyp_turns;
    long long n_hyp;
    const int* frame_item;  // the labelled-items form
    const long long* item_offs;
    const int* item_labels;
    long long n_items;
    long long* counts;
    int *map_ref, *C;
    unsigned long long* mask;
    unsigned* flag;
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the frames of recording r, inside the workspace whatever the device table says
__device__ __forceinline__ void recording(const DerArgs& a, long long r, long long& f0, long long& T) {
    f0 = clampll(a.frame_offs[r], 0, a.frames);
    T = clampll(a.frame_offs[r + 1], f0, a.frames) - f0;
    if (T > kDerMaxT) T = kDerMaxT;
}

__global__ __launch_bounds__(256) void der_init_kernel(unsigned long long* mask, unsigned* flag, long long frames, unsigned value) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < frames; i += (long long)gridDim.x * 256) {
        mask[i] = 0ull;
        flag[i] = value;
    }
}

__global__ __launch_bounds__(256) void der_paint_kernel(DerArgs a) {
    const long long r = blockIdx.x;
    const int tid = threadIdx.x;
    long long f0, T;
    recording(a, r, f0, T);
    unsigned long long* mask = a.mask + f0;
    unsigned* flag = a.flag + f0;
    const long long k0 = clampll(a.ref_offs[r], 0, a.n_ref), k1 = clampll(a.ref_offs[r + 1], k0, a.n_ref);
    const long long c = a.collar;
    for (long long k = k0 + blockIdx.y; k < k1; k += kPaintSplit) {
        const int s = a.ref_turns[3 * k + 2];
        if (s < 0 || s >= a.S_ref) continue;  // a speaker outside the limit: the turn does not exist
        const long long b = clampll(a.ref_turns[3 * k], 0, T), e = clampll(a.ref_turns[3 * k + 1], 0, T);
        if (e < b) continue;
        const unsigned long long bit = 1ull << s;
        for (long long f = b + tid; f < e; f += 256) atomicOr(mask + f, bit);
        if (c > 0) {
            const long long b0 = clampll(b - c, 0, T), b1 = clampll(b + c, 0, T), e0 = clampll(e - c, 0, T), e1 = clampll(e + c, 0, T);
            for (long long f = b0 + tid; f < b1; f += 256) atomicOr(flag + f, kInCollar);
            for (long long f = e0 + tid; f < e1; f += 256) atomicOr(flag + f, kInCollar);
        }
    }
    if (a.uem_offs) {
        const long long u0 = clampll(a.uem_offs[r], 0, a.n_uem), u1 = clampll(a.uem_offs[r + 1], u0, a.n_uem);
        for (long long k = u0 + blockIdx.y; k < u1; k += kPaintSplit) {
            const long long b = clampll(a.uem[2 * k], 0, T), e = clampll(a.uem[2 * k + 1], 0, T);
            for (long long f = b + tid; f < e; f += 256) atomicOr(flag + f, kInUem);
        }
    }
}

// (ONE kernel for both forms of the hypotheses.  The labelled-items form does not touch `hyp`; compiled on its own with 16 KB
// of LDS it ran eight workgroups per CU instead of three and took 9.5 ms where this one takes 6.2: more problems in flight
// are more recordings' masks competing for the L2.  design/k24_der.md.)
struct DerShared {
    int C[kDerMaxS * kDerMaxS];
    unsigned long long hyp[kChunk];
    unsigned long long red[8];  // scored, total, miss, fa, sum of min, OR of R, OR of H
};

__device__ __forceinline__ void add_run(int* C, unsigned long long R, unsigned long long H, int len) {
    if (R == 0ull || H == 0ull) return;
    for (unsigned long long rr = R; rr; rr &= rr - 1) {
        const int i = __builtin_ctzll(rr);
        for (unsigned long long hh = H; hh; hh &= hh - 1) atomicAdd(&C[i * kDerMaxS + __builtin_ctzll(hh)], len);
    }
}

// Maximum-weight one-to-one assignment on the n x n corner of C (n <= 64, weights >= 0), on ONE wave with all 64 lanes active:
// shortest augmenting paths on the costs -C with integer potentials.  Lane j holds column j (its potential v, the row p assigned
// to it, the slack minv and the predecessor column `way` of the current search) and, as a row, the potential u of row j and
// the column rowcol assigned to it.  Rows enter in increasing order; among the columns of equal smallest slack the LOWEST is
// taken: that is the whole tie rule, and it makes the mapping a function of C alone.  -> rowcol of this lane's row (every row
// below n has a column afterwards).
__device__ int assign_rows(const int* C, int n, int lane) {
    const long long kInf = 0x1fffffffffffffffll, kClosed = 0x7fffffffffffffffll;
    long long u = 0, v = 0;
    int p = -1, rowcol = -1;
    for (int i = 0; i < n; ++i) {
        long long minv = kInf;
        int way = -1, j0 = -1, i0 = i;
        bool used = false;
        unsigned long long usedmask = 0ull;
        for (int it = 0; it <= n; ++it) {
            const long long ui0 = __shfl(u, i0, 64);
            const bool open = !used && lane < n;
            if (open) {
                const long long cur = -(long long)C[i0 * kDerMaxS + lane] - ui0 - v;
                if (cur < minv) {
                    minv = cur;
                    way = j0;
                }
            }
            const long long cand = open ? minv : kClosed;
            const long long delta = wave_min(cand);
            if (delta == kClosed) break;  // (no open column: cannot happen while i < n)
            const int j1 = __builtin_ctzll(__ballot(cand == delta));
            const bool in_tree = lane == i || (rowcol >= 0 && ((usedmask >> rowcol) & 1ull));
            if (in_tree) u += delta;
            if (used) v -= delta;
            else if (lane < n) minv -= delta;
            j0 = j1;
            used = used || lane == j0;
            usedmask |= 1ull << j0;
            i0 = __shfl(p, j0, 64);
            if (i0 < 0) break;
        }
        for (int it = 0; it <= n && j0 >= 0; ++it) {  // turn the path round
            const int j1 = __shfl(way, j0, 64);
            const int r = j1 < 0 ? i : __shfl(p, j1, 64);
            if (lane == j0) p = r;
            if (lane == r) rowcol = j0;
            j0 = j1;
        }
    }
    return rowcol;
}

__global__ __launch_bounds__(kDerBlock) void der_count_kernel(DerArgs a) {
    __shared__ DerShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long prob = blockIdx.x;
    for (int i = tid; i < kDerMaxS * kDerMaxS; i += kDerBlock) sh.C[i] = 0;
    if (tid < 8) sh.red[tid] = 0ull;
    const long long r = a.prob_reco[prob];
    long long f0 = 0, T = 0;
    if (r >= 0 && r < a.Rn) recording(a, r, f0, T);
    const bool by_turns = a.hyp_offs != nullptr;
    long long h0 = 0, h1 = 0, i0 = 0, nI = 0;
    if (by_turns) {
        h0 = clampll(a.hyp_offs[prob], 0, a.n_hyp);
        h1 = clampll(a.hyp_offs[prob + 1], h0, a.n_hyp);
    } else {
        i0 = clampll(a.item_offs[prob], 0, a.n_items);
        nI = clampll(a.item_offs[prob + 1], i0, a.n_items) - i0;
    }
    const unsigned long long* mask = a.mask + f0;
    const unsigned* flag = a.flag + f0;
    const int* item = by_turns ? nullptr : a.frame_item + f0;
    __syncthreads();

    long long scored = 0, total = 0, miss = 0, fa = 0, smin = 0;
    unsigned long long orR = 0ull, orH = 0ull;
    for (long long c0 = 0; c0 < T; c0 += kChunk) {  // (block-uniform bounds: the barriers inside are reached by everyone)
        const long long c1 = c0 + kChunk < T ? c0 + kChunk : T;
        if (by_turns) {
            for (int i = tid; i < kChunk; i += kDerBlock) sh.hyp[i] = 0ull;
            __syncthreads();
            for (long long k = h0 + wave; k < h1; k += kDerWaves) {  // a wave per turn, a lane per frame
                const int s = a.hyp_turns[3 * k + 2];
                if (s < 0 || s >= a.S_hyp) continue;
                const long long b = clampll(a.hyp_turns[3 * k], c0, c1), e = clampll(a.hyp_turns[3 * k + 1], c0, c1);
                for (long long f = b + lane; f < e; f += 64) atomicOr(&sh.hyp[f - c0], 1ull << s);
            }
            __syncthreads();
        }
        const long long fb = c0 + (long long)tid * kPer;
        const long long fe = fb + kPer < c1 ? fb + kPer : c1;
        unsigned long long curR = 0ull, curH = 0ull;
        int len = 0;
        for (long long f = fb; f < fe; ++f) {
            unsigned long long R = mask[f], H;
            int pr = __popcll(R);
            const bool sc = flag[f] == kInUem && !(a.skip_overlap && pr > 1);
            if (by_turns) {
                H = sh.hyp[f - c0];
            } else {
                const int it = item[f];
                const int lab = (it >= 0 && it < nI) ? a.item_labels[i0 + it] : -1;
                H = (lab >= 0 && lab < a.S_hyp) ? 1ull << lab : 0ull;
            }
            if (!sc) {
                R = 0ull;
                H = 0ull;
                pr = 0;
            }
            const int ph = __popcll(H);
            scored += sc ? 1 : 0;
            total += pr;
            miss += pr > ph ? pr - ph : 0;
            fa += ph > pr ? ph - pr : 0;
            smin += pr < ph ? pr : ph;
            orR |= R;
            orH |= H;
            if (R == curR && H == curH) {
                ++len;
            } else {
                add_run(sh.C, curR, curH, len);
                curR = R;
                curH = H;
                len = 1;
            }
        }
        add_run(sh.C, curR, curH, len);
        if (by_turns) __syncthreads();  // the chunk's masks are read; the next chunk may clear them
    }
    // integer atomics in LDS: the sums do not depend on the order
    atomicAdd(&sh.red[0], (unsigned long long)scored);
    atomicAdd(&sh.red[1], (unsigned long long)total);
    atomicAdd(&sh.red[2], (unsigned long long)miss);
    atomicAdd(&sh.red[3], (unsigned long long)fa);
    atomicAdd(&sh.red[4], (unsigned long long)smin);
    atomicOr(&sh.red[5], orR);
    atomicOr(&sh.red[6], orH);
    __syncthreads();

    if (a.C)
        for (int i = tid; i < kDerMaxS * kDerMaxS; i += kDerBlock) a.C[prob * (kDerMaxS * kDerMaxS) + i] = sh.C[i];
    if (wave == 0) {
        const unsigned long long allR = sh.red[5], allH = sh.red[6];
        const int nr = allR ? 64 - __builtin_clzll(allR) : 0, nh = allH ? 64 - __builtin_clzll(allH) : 0;
        const int n = nr > nh ? nr : nh;
        const int col = assign_rows(sh.C, n, lane);
        const int w = (lane < n && col >= 0) ? sh.C[lane * kDerMaxS + col] : 0;
        a.map_ref[prob * kDerMaxS + lane] = w > 0 ? col : -1;  // a pair that shares no scored frame is no mapping
        const long long matched = wave_sum((long long)w);
        if (lane < kNCounts) a.counts[prob * kNCounts + lane] = lane < 5 ? (long long)sh.red[lane] : matched;
    }
}

}  // namespace

extern "C" {

int nplda_der_max_speakers(void) { return kDerMaxS; }
int nplda_der_block(void) { return kDerBlock; }

size_t nplda_der_workspace_bytes(const int64_t* frame_offsets_host, int64_t Rn) {
    const DerPlan r = der_plan(frame_offsets_host, Rn);
    return r.status == NPLDA_OK ? r.ws_bytes : 0;
}

int nplda_der_i64(const int64_t* frame_offsets_host, const int64_t* frame_offsets, int64_t Rn, const int64_t* ref_offsets_host,
                  const int64_t* ref_offsets, const int32_t* ref_turns, const int64_t* uem_offsets_host, const int64_t* uem_offsets,
                  const int32_t* uem, int collar, int skip_overlap, int n_ref_speakers, int n_hyp_speakers,
                  const int32_t* prob_reco_host, const int32_t* prob_reco, int64_t P, const int64_t* hyp_offsets_host,
                  const int64_t* hyp_offsets, const int32_t* hyp_turns, const int32_t* frame_item, const int64_t* item_offsets_host,
                  const int64_t* item_offsets, const int32_t* item_labels, int64_t* counts, int32_t* map_ref, int32_t* C, void* ws,
                  size_t ws_bytes, nplda_stream_t stream) {
    if (collar < 0 || n_ref_speakers < 0 || n_hyp_speakers < 0 || P < 0) return NPLDA_EINVAL;
    const DerPlan r = der_plan(frame_offsets_host, Rn);
    if (r.status == NPLDA_EINVAL) return r.status;
    const long long n_ref = table_total(ref_offsets_host, Rn);
    if (n_ref < 0) return NPLDA_EINVAL;
    long long n_uem = 0, n_hyp = 0, n_items = 0;
    if ((uem_offsets_host != nullptr) != (uem_offsets != nullptr)) return NPLDA_EINVAL;
    if (uem_offsets_host && (n_uem = table_total(uem_offsets_host, Rn)) < 0) return NPLDA_EINVAL;
    const bool by_turns = hyp_offsets_host != nullptr;
    if (by_turns == (item_offsets_host != nullptr)) return NPLDA_EINVAL;  // exactly one form of the hypotheses
    if (by_turns ? (frame_item || item_offsets || item_labels) : (hyp_offsets || hyp_turns)) return NPLDA_EINVAL;
    if (by_turns && (n_hyp = table_total(hyp_offsets_host, P)) < 0) return NPLDA_EINVAL;
    if (!by_turns && (n_items = table_total(item_offsets_host, P)) < 0) return NPLDA_EINVAL;
    if (P > 0 && !prob_reco_host) return NPLDA_EINVAL;
    for (int64_t p = 0; p < P; ++p)
        if (prob_reco_host[p] < 0 || prob_reco_host[p] >= Rn) return NPLDA_EINVAL;
    if (r.status != NPLDA_OK) return r.status;
    if (n_ref_speakers > kDerMaxS || n_hyp_speakers > kDerMaxS || P > kDerMaxP) return NPLDA_EUNSUPPORTED;
    if (P == 0) return NPLDA_OK;
    auto a8 = [](const void* p) { return (((uintptr_t)p) & 7u) == 0; };
    auto a4 = [](const void* p) { return (((uintptr_t)p) & 3u) == 0; };
    if (!frame_offsets || !ref_offsets || !prob_reco || !counts || !map_ref) return NPLDA_EINVAL;
    if (by_turns ? !hyp_offsets : !item_offsets) return NPLDA_EINVAL;
    if ((n_ref > 0 && !ref_turns) || (n_uem > 0 && !uem) || (n_hyp > 0 && !hyp_turns) || (n_items > 0 && !item_labels))
        return NPLDA_EINVAL;
    if (!by_turns && r.frames > 0 && !frame_item) return NPLDA_EINVAL;
    if (!a8(frame_offsets) || !a8(ref_offsets) || !a8(uem_offsets) || !a8(hyp_offsets) || !a8(item_offsets) || !a8(counts))
        return NPLDA_EINVAL;
    if (!a4(ref_turns) || !a4(uem) || !a4(prob_reco) || !a4(hyp_turns) || !a4(frame_item) || !a4(item_labels) || !a4(map_ref) ||
        !a4(C))
        return NPLDA_EINVAL;
    if (!ws || !nplda_aligned16(ws)) return NPLDA_EINVAL;
    if (ws_bytes < r.ws_bytes) return NPLDA_ENOSPC;

    DerArgs a;
    a.frame_offs = (const long long*)frame_offsets;
    a.Rn = Rn;
    a.frames = r.frames;
    a.ref_offs = (const long long*)ref_offsets;
    a.ref_turns = (const int*)ref_turns;
    a.n_ref = n_ref;
    a.uem_offs = (const long long*)uem_offsets;
    a.uem = (const int*)uem;
    a.n_uem = n_uem;
    a.collar = collar;
    a.skip_overlap = skip_overlap != 0;
    a.S_ref = n_ref_speakers;
    a.S_hyp = n_hyp_speakers;
    a.prob_reco = (const int*)prob_reco;
    a.hyp_offs = (const long long*)hyp_offsets;
    a.hyp_turns = (const int*)hyp_turns;
    a.n_hyp = n_hyp;
    a.frame_item = (const int*)frame_item;
    a.item_offs = (const long long*)item_offsets;
    a.item_labels = (const int*)item_labels;
    a.n_items = n_items;
    a.counts = (long long*)counts;
    a.map_ref = (int*)map_ref;
    a.C = (int*)C;
    a.mask = (unsigned long long*)ws;
    a.flag = (unsigned*)((char*)ws + r.mask_bytes);
    hipStream_t st = (hipStream_t)stream;
    if (r.frames > 0) {
        const long long want = (r.frames + 255) / 256;
        const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
        hipLaunchKernelGGL(der_init_kernel, dim3(blocks), dim3(256), 0, st, a.mask, a.flag, r.frames, uem_offsets ? 0u : kInUem);
        hipLaunchKernelGGL(der_paint_kernel, dim3((unsigned)Rn, kPaintSplit), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(der_count_kernel, dim3((unsigned)P), dim3(kDerBlock), 0, st, a);
    return nplda_launch_status();
}

}  // extern "C"
