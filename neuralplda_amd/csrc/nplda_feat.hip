// nplda_feat.hip — the front end of the E-TDNN extractor on gfx950: Kaldi feature-matrix bodies (FM / DM / CM / CM2 / CM3)
// as they lie in an archive -> float32 MFCC rows, energy VAD (compute-vad-energy), sliding-window mean normalisation
// (apply-cmvn-sliding --norm-vars=false --center=true) and voiced-frame selection (select-voiced-frames), producing the
// (sum T'_u, 30) rows nplda_xvec_extract_f32 takes.  design/k13_feature_frontend.md.
//
// All kernels are memory-bound (about 30 B in and 0.8 KB of fp32 / fp64 traffic per frame); they aim at coalesced access
// and few launches, nothing more.  Every sum has a fixed order and there are no atomics: two calls give the same bits,
// and an utterance's rows do not depend on the rest of the batch.
#include "nplda_common.h"

namespace {

constexpr int F = NPLDA_FEAT_DIM;  // 30 columns
constexpr int TILE = 64;           // frames per tile
constexpr int LDT = F + 1;         // LDS row stride of a tile: odd, so that a column of 64 rows hits 64 different banks
constexpr int NT = 256;            // threads per block

struct Desc {  // nplda_feat_desc of the header, 40 bytes
    int32_t format, rows, cols;
    float min_value, range;
    int32_t reserved;
    int64_t hdr_off, data_off;
};
static_assert(sizeof(Desc) == 40, "descriptor layout");

// The utterance that holds global frame r: the last u with offsets[u] <= r (utterances of no frames are stepped over).
__device__ inline int utt_of(const int64_t* __restrict__ offsets, int U, int64_t r) {
    int lo = 0, hi = U;  // invariant: offsets[lo] <= r < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline double u16_value(double min_value, double range, unsigned v) {
    return min_value + range * (1.0 / 65535.0) * (double)v;
}

struct RowInfo {  // what a tile keeps in LDS about each of its rows
    int format;
    float min_value, range;
    int64_t T, t, hdr_off, data_off;  // frames of the row's utterance, the row's frame in it, its body in the payload
};

// ---- decode ------------------------------------------------------------------------------------------------------------

struct DecodeArgs {
    const uint8_t* payload;
    int64_t payload_bytes;
    const Desc* desc;
    const int64_t* offsets;
    int U;
    int64_t R;
    float* out;
};

// A block decodes TILE consecutive rows of the OUTPUT (which may belong to several utterances).  Row-major bodies (FM, DM,
// CM2, CM3) are read in output order; a CM body is column-major, so it is read one column at a time — lane i of a wave
// takes frame i of the tile, 64 consecutive bytes — and every value goes through an LDS tile from which the 64 x 30 floats
// are stored as one contiguous run.
__global__ __launch_bounds__(NT) void feat_decode_kernel(DecodeArgs a) {
    __shared__ float tile[TILE * LDT];
    __shared__ RowInfo row[TILE];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * TILE;
    if (tid < TILE) {
        const int64_t r = r0 + tid;
        RowInfo ri;
        ri.format = -1;  // beyond R, or an entry that fails its checks: NaN rows
        ri.min_value = ri.range = 0.f;
        ri.T = ri.t = ri.hdr_off = ri.data_off = 0;
        if (r < a.R) {
            const int u = utt_of(a.offsets, a.U, r);
            const Desc d = a.desc[u];
            const int64_t off = a.offsets[u];
            const int64_t T = a.offsets[u + 1] - off;
            int64_t esz = 0;
            switch (d.format) {
                case NPLDA_FEAT_FM: esz = 4; break;
                case NPLDA_FEAT_DM: esz = 8; break;
                case NPLDA_FEAT_CM2: esz = 2; break;
                case NPLDA_FEAT_CM: case NPLDA_FEAT_CM3: esz = 1; break;
                default: break;
            }
            bool ok = esz != 0 && d.cols == F && d.rows == T && d.data_off >= 0 && (d.data_off % esz) == 0 &&
                      d.data_off + T * F * esz <= a.payload_bytes;
            if (d.format == NPLDA_FEAT_CM)
                ok = ok && d.hdr_off >= 0 && (d.hdr_off & 1) == 0 && d.hdr_off + 8 * F <= a.payload_bytes;
            if (ok) {
                ri.format = d.format; ri.min_value = d.min_value; ri.range = d.range;
                ri.T = T; ri.t = r - off; ri.hdr_off = d.hdr_off; ri.data_off = d.data_off;
            }
        }
        row[tid] = ri;
    }
    __syncthreads();
    // row-major bodies, in output order
    for (int k = tid; k < TILE * F; k += NT) {
        const int i = k / F, c = k - i * F;
        const int fmt = row[i].format;
        if (fmt == NPLDA_FEAT_CM) continue;
        float v = __builtin_nanf("");
        if (fmt >= 0) {
            const int64_t e = row[i].t * F + c;
            const uint8_t* p = a.payload + row[i].data_off;
            const double lo = (double)row[i].min_value, range = (double)row[i].range;
            if (fmt == NPLDA_FEAT_FM) v = reinterpret_cast<const float*>(p)[e];
            else if (fmt == NPLDA_FEAT_DM) v = (float)reinterpret_cast<const double*>(p)[e];
            else if (fmt == NPLDA_FEAT_CM2) v = (float)u16_value(lo, range, reinterpret_cast<const uint16_t*>(p)[e]);
            else v = (float)(lo + range * ((double)p[e] * (1.0 / 255.0)));
        }
        tile[i * LDT + c] = v;
    }
    // CM bodies, a column per wave and pass
    {
        const int i = tid & 63;
        if (row[i].format == NPLDA_FEAT_CM) {
            const int64_t T = row[i].T, t = row[i].t;
            const double lo = (double)row[i].min_value, range = (double)row[i].range;
            const uint16_t* hdr = reinterpret_cast<const uint16_t*>(a.payload + row[i].hdr_off);
            const uint8_t* body = a.payload + row[i].data_off;
            for (int c = tid >> 6; c < F; c += NT / 64) {
                const double p0 = u16_value(lo, range, hdr[4 * c]), p25 = u16_value(lo, range, hdr[4 * c + 1]);
                const double p75 = u16_value(lo, range, hdr[4 * c + 2]), p100 = u16_value(lo, range, hdr[4 * c + 3]);
                const unsigned b = body[(int64_t)c * T + t];
                double v;
                if (b <= 64) v = p0 + (p25 - p0) * (double)b * (1.0 / 64.0);
                else if (b <= 192) v = p25 + (p75 - p25) * (double)(b - 64) * (1.0 / 128.0);
                else v = p75 + (p100 - p75) * (double)(b - 192) * (1.0 / 63.0);
                tile[i * LDT + c] = (float)v;
            }
        }
    }
    __syncthreads();
    const int64_t left = a.R - r0;
    const int n = (int)(left < TILE ? left : TILE) * F;
    float* o = a.out + r0 * F;
    for (int k = tid; k < n; k += NT) {
        const int i = k / F;
        o[k] = tile[i * LDT + (k - i * F)];
    }
}

// ---- energy VAD --------------------------------------------------------------------------------------------------------

struct VadArgs {
    const float* frames;
    const int64_t* offsets;
    double energy_threshold, energy_mean_scale, proportion_threshold;
    int context;
    uint8_t* mask;
};

// One block per utterance: the mean of c0 in fp64 (a fixed strided partition, then a fixed tree), then the window vote.
__global__ __launch_bounds__(NT) void feat_vad_kernel(VadArgs a) {
    __shared__ double part[NT];
    const int tid = threadIdx.x;
    const int64_t off = a.offsets[blockIdx.x];
    const int64_t T = a.offsets[blockIdx.x + 1] - off;
    if (T <= 0) return;
    const float* c0 = a.frames + off * F;
    double s = 0.0;
    for (int64_t t = tid; t < T; t += NT) s += (double)c0[t * F];
    part[tid] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    const double thr = a.energy_threshold + a.energy_mean_scale * (part[0] / (double)T);
    for (int64_t t = tid; t < T; t += NT) {
        int64_t lo = t - a.context, hi = t + a.context;
        if (lo < 0) lo = 0;
        if (hi > T - 1) hi = T - 1;
        int num = 0;
        for (int64_t t2 = lo; t2 <= hi; ++t2) num += (double)c0[t2 * F] > thr ? 1 : 0;
        a.mask[off + t] = (double)num >= (double)(hi - lo + 1) * a.proportion_threshold ? 1 : 0;
    }
}

// ---- voiced counts and their running sum -------------------------------------------------------------------------------

struct CountArgs {
    const uint8_t* mask;  // NULL: every frame is kept
    const int64_t* offsets;
    int32_t* counts;
};

__global__ __launch_bounds__(NT) void feat_count_kernel(CountArgs a) {
    __shared__ int part[NT];
    const int tid = threadIdx.x;
    const int64_t off = a.offsets[blockIdx.x];
    const int64_t T = a.offsets[blockIdx.x + 1] - off;
    if (a.mask == nullptr) {
        if (tid == 0) a.counts[blockIdx.x] = (int32_t)T;
        return;
    }
    int n = 0;
    for (int64_t t = tid; t < T; t += NT) n += a.mask[off + t] != 0;
    part[tid] = n;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) a.counts[blockIdx.x] = part[0];
}

struct ScanArgs {
    const int32_t* counts;
    int U, min_frames;
    int64_t* out_offsets;  // U + 1: first output row of every utterance; an utterance below min_frames takes none
};

// One block: thread i owns a run of ceil(U / 1024) utterances.
__global__ __launch_bounds__(1024) void feat_scan_kernel(ScanArgs a) {
    __shared__ int64_t run[1024];
    const int tid = threadIdx.x;
    const int per = (a.U + 1023) / 1024;
    const int u0 = tid * per, u1 = min(u0 + per, a.U);
    int64_t s = 0;
    for (int u = u0; u < u1; ++u) {
        const int c = a.counts[u];
        s += c >= a.min_frames ? c : 0;
    }
    run[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t acc = 0;
        for (int i = 0; i < 1024; ++i) {
            const int64_t v = run[i];
            run[i] = acc;
            acc += v;
        }
    }
    __syncthreads();
    s = run[tid];
    for (int u = u0; u < u1; ++u) {
        a.out_offsets[u] = s;
        const int c = a.counts[u];
        s += c >= a.min_frames ? c : 0;
    }
    if (u0 < a.U && u1 == a.U) a.out_offsets[a.U] = s;  // the thread that owns the last utterance
}

// ---- sliding CMN + select ----------------------------------------------------------------------------------------------

struct CmnArgs {
    const float* frames;
    const int64_t* offsets;
    const uint8_t* mask;         // NULL: every frame is kept
    const int64_t* out_offsets;  // from feat_scan_kernel
    int window;                  // 0: no normalisation
    double* prefix;              // (R + U) x 30: exclusive prefix sums of every utterance's columns, T_u + 1 rows each
    float* out;
};

// One block per utterance.  Phase 1: exclusive fp64 prefix sums of the 30 columns over time, 64 frames per step: thread
// (j, c) adds frames 8 j .. 8 j + 7 of column c in order, the eight partial sums are added in order on top of the carry.
// Phase 2: frame t's window [s, e) is two rows of the prefix table; the voiced frames' x - mean go out in their order
// (rank = the carry plus the number of voiced frames before t in the 64-frame step, from one ballot).
__global__ __launch_bounds__(NT) void feat_cmn_select_kernel(CmnArgs a) {
    __shared__ float tile[TILE * LDT];
    __shared__ double sub[8 * 32];
    __shared__ double carry[32];
    __shared__ int rank[TILE];
    __shared__ int kept_before, kept_step;
    const int tid = threadIdx.x;
    const int u = blockIdx.x;
    const int64_t off = a.offsets[u];
    const int64_t T = a.offsets[u + 1] - off;
    const int64_t obase = a.out_offsets[u];
    if (T <= 0 || a.out_offsets[u + 1] == obase) return;  // empty, or left out (below min_frames)
    const float* x = a.frames + off * F;
    double* P = a.prefix + (off + u) * F;
    if (a.window > 0) {
        const int c = tid & 31, j = tid >> 5;
        if (tid < 32) carry[tid] = 0.0;
        if (tid < F) P[tid] = 0.0;
        for (int64_t t0 = 0; t0 < T; t0 += TILE) {
            const int rows = (int)(T - t0 < TILE ? T - t0 : TILE);
            __syncthreads();
            for (int k = tid; k < rows * F; k += NT) {
                const int i = k / F;
                tile[i * LDT + (k - i * F)] = x[t0 * F + k];
            }
            __syncthreads();
            const int i0 = 8 * j, i1 = min(i0 + 8, rows);
            double s = 0.0;
            if (c < F)
                for (int i = i0; i < i1; ++i) s += (double)tile[i * LDT + c];
            sub[j * 32 + c] = s;
            __syncthreads();
            if (c < F) {
                double base = carry[c];
                for (int jj = 0; jj < j; ++jj) base += sub[jj * 32 + c];
                for (int i = i0; i < i1; ++i) {
                    base += (double)tile[i * LDT + c];
                    P[(t0 + i + 1) * F + c] = base;
                }
            }
            __syncthreads();
            if (j == 7 && c < F) {
                double base = carry[c];
                for (int jj = 0; jj < 8; ++jj) base += sub[jj * 32 + c];
                carry[c] = base;
            }
        }
    }
    if (tid == 0) kept_before = 0;
    __syncthreads();  // the block's own prefix rows are visible to all of its waves from here
    const int W = a.window;
    for (int64_t t0 = 0; t0 < T; t0 += TILE) {
        const int rows = (int)(T - t0 < TILE ? T - t0 : TILE);
        if (tid < TILE) {
            const bool v = tid < rows && (a.mask == nullptr || a.mask[off + t0 + tid] != 0);
            const unsigned long long b = __ballot(v);
            rank[tid] = v ? __popcll(b & ((1ull << tid) - 1ull)) : -1;
            if (tid == 0) kept_step = __popcll(b);
        }
        __syncthreads();
        const int before = kept_before;
        for (int k = tid; k < rows * F; k += NT) {
            const int i = k / F, c = k - i * F;
            const int rk = rank[i];
            if (rk < 0) continue;
            const int64_t t = t0 + i;
            double v = (double)x[t * F + c];
            if (W > 0) {
                int64_t s = t - W / 2, e = s + W;
                if (s < 0) { e -= s; s = 0; }
                if (e > T) { s -= e - T; e = T; }
                if (s < 0) s = 0;
                v -= (P[e * F + c] - P[s * F + c]) / (double)(e - s);
            }
            a.out[(obase + before + rk) * F + c] = (float)v;
        }
        __syncthreads();
        if (tid == 0) kept_before = before + kept_step;
    }
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" {

int nplda_feat_decode_f32(const void* payload, size_t payload_bytes, const void* desc, const int64_t* offsets, int64_t n_utts,
                          int64_t total_frames, float* frames, nplda_stream_t stream) {
    if (n_utts < 0 || total_frames < 0 || n_utts > INT32_MAX) return NPLDA_EINVAL;
    if (n_utts == 0 || total_frames == 0) return NPLDA_OK;
    if (!payload || !desc || !offsets || !frames || (((uintptr_t)payload) & 7u) || (((uintptr_t)desc) & 7u)) return NPLDA_EINVAL;
    DecodeArgs a;
    a.payload = (const uint8_t*)payload; a.payload_bytes = (int64_t)payload_bytes; a.desc = (const Desc*)desc;
    a.offsets = offsets; a.U = (int)n_utts; a.R = total_frames; a.out = frames;
    const int64_t tiles = (total_frames + TILE - 1) / TILE;
    if (tiles > INT32_MAX) return NPLDA_EUNSUPPORTED;
    hipLaunchKernelGGL(feat_decode_kernel, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, a);
    return nplda_launch_status();
}

int nplda_feat_vad_energy_f32(const float* frames, const int64_t* offsets, int64_t n_utts, int64_t total_frames,
                              double energy_threshold, double energy_mean_scale, double proportion_threshold,
                              int frames_context, uint8_t* mask, nplda_stream_t stream) {
    if (n_utts < 0 || total_frames < 0 || n_utts > INT32_MAX || frames_context < 0) return NPLDA_EINVAL;
    if (n_utts == 0 || total_frames == 0) return NPLDA_OK;
    if (!frames || !offsets || !mask) return NPLDA_EINVAL;
    VadArgs a;
    a.frames = frames; a.offsets = offsets; a.energy_threshold = energy_threshold; a.energy_mean_scale = energy_mean_scale;
    a.proportion_threshold = proportion_threshold; a.context = frames_context; a.mask = mask;
    hipLaunchKernelGGL(feat_vad_kernel, dim3((unsigned)n_utts), dim3(NT), 0, (hipStream_t)stream, a);
    return nplda_launch_status();
}

size_t nplda_feat_workspace_bytes(int64_t total_frames, int64_t n_utts) {
    if (total_frames < 0 || n_utts < 0) return 0;
    return align256((size_t)(n_utts + 1) * sizeof(int64_t)) + align256((size_t)(total_frames + n_utts) * F * sizeof(double));
}

int nplda_feat_cmn_select_f32(const float* frames, const int64_t* offsets, int64_t n_utts, int64_t total_frames,
                              const uint8_t* mask, int cmn_window, int min_frames, float* out, int32_t* counts, void* ws,
                              size_t ws_bytes, nplda_stream_t stream) {
    if (n_utts < 0 || total_frames < 0 || n_utts > INT32_MAX || cmn_window < 0) return NPLDA_EINVAL;
    if (n_utts == 0) return NPLDA_OK;
    if (!offsets || !counts || !ws || (total_frames > 0 && (!frames || !out)) || (((uintptr_t)ws) & 7u)) return NPLDA_EINVAL;
    if (ws_bytes < nplda_feat_workspace_bytes(total_frames, n_utts)) return NPLDA_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    int64_t* out_offsets = (int64_t*)ws;
    double* prefix = (double*)((char*)ws + align256((size_t)(n_utts + 1) * sizeof(int64_t)));
    CountArgs c;
    c.mask = mask; c.offsets = offsets; c.counts = counts;
    hipLaunchKernelGGL(feat_count_kernel, dim3((unsigned)n_utts), dim3(NT), 0, st, c);
    if (int rc = nplda_launch_status()) return rc;
    ScanArgs s;
    s.counts = counts; s.U = (int)n_utts; s.min_frames = min_frames; s.out_offsets = out_offsets;
    hipLaunchKernelGGL(feat_scan_kernel, dim3(1), dim3(1024), 0, st, s);
    if (int rc = nplda_launch_status()) return rc;
    if (total_frames == 0) return NPLDA_OK;
    CmnArgs a;
    a.frames = frames; a.offsets = offsets; a.mask = mask; a.out_offsets = out_offsets; a.window = cmn_window;
    a.prefix = prefix; a.out = out;
    hipLaunchKernelGGL(feat_cmn_select_kernel, dim3((unsigned)n_utts), dim3(NT), 0, st, a);
    return nplda_launch_status();
}

}  // extern "C"
