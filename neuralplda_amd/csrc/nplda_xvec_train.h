// nplda_xvec_train.h — what the two training paths of the E-TDNN extractor share: the running-statistics path
// (nplda_xvec_bwd.hip) and the batch-statistics path (nplda_xvec_bn.hip).  Buffer layouts, index helpers and the argument
// checks of a backward entry point are inline.  The two chains are defined once, in nplda_xvec_bwd.hip, next to their
// kernels (the library's version script keeps them out of the dynamic symbol table): the training forward is
// train_forward_head, the caller's own layer loop, train_forward_tail; a backward is backward_head, the caller's pooling
// backward, then per layer the caller's batch-norm step if any, layer_param_grads, and the caller's data-gradient GEMM on
// data_grad_args.
#pragma once
#include "nplda_xvec_body.h"

namespace nplda_xvec_train {

using namespace nplda_xvec;

constexpr int kCtx[kTdnn] = {4, 4, 8, 8, 14, 14, 22, 22, 22, 22};  // frames lost through tdnn1..tdnn<l+1>
constexpr int kLead = 16;     // zeroed rows in front of every dA buffer (>= max d (c - 1) = 8)
constexpr int kWgKC = 16;     // frames per staged wgrad chunk
constexpr int kWgTargetBlocks = 512;
constexpr int kColSplits = 1024;  // row splits of the bias column sums (enough blocks to stream dA at bandwidth)

// the transposed image holds layers 1..10 (tdnn2..tdnn10, lin11): per tap the Dout x Din block transposed
inline LayerGeom geomT(int l, size_t start) {
    const Layer s = kShape[l];
    return geom_of(Layer{s.Dout, s.Din, s.c, s.d}, start);
}
inline size_t packedT_offset(int l) {
    size_t o = 0;
    for (int i = 1; i < l; ++i) o = geomT(i, o).end;
    return o;
}
inline size_t packedT_floats() { return packedT_offset(kLayers); }

// flat gradient: for l = 0..10, W_l (Dout, c Din) then b_l (Dout)
inline size_t grad_offset(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += (size_t)kShape[i].Dout * (kShape[i].c * kShape[i].Din + 1);
    return o;
}

struct SavedLayout {
    long long rows, live, urows;
    size_t oX, oRem, oO[kTdnn], oM[kTdnn], oP, total;  // bytes
};

inline SavedLayout saved_layout(long long R, long long U) {
    SavedLayout s;
    s.live = whole_tiles(R);
    s.rows = s.live + kRowSlack;
    s.urows = whole_tiles(U);
    size_t o = 0;
    s.oX = o;
    o = align256(o + (size_t)s.rows * kFeatP * 4);
    s.oRem = o;
    o = align256(o + (size_t)s.rows * 4);
    for (int l = 0; l < kTdnn; ++l) {
        s.oO[l] = o;
        o = align256(o + (size_t)s.rows * out_ld(l) * 4);
    }
    for (int l = 0; l < kTdnn; ++l) {
        s.oM[l] = o;
        o = align256(o + (size_t)s.rows * out_ld(l));
    }
    s.oP = o;
    s.total = align256(o + (size_t)s.urows * kPooledLd * 4);
    return s;
}

struct WgPlan {
    int Mt, Nt, S, cps;
    long long nchunks;
};

inline WgPlan wg_plan(int l, long long kmax) {
    const Layer s = kShape[l];
    WgPlan p;
    p.Mt = (s.Dout + 127) / 128;
    p.Nt = (s.c * round_up(s.Din, 16) + 127) / 128;
    p.nchunks = (kmax + kWgKC - 1) / kWgKC;
    const int tiles = p.Mt * p.Nt;
    long long S = (kWgTargetBlocks + tiles - 1) / tiles;
    if (S > p.nchunks) S = p.nchunks;
    if (S < 1) S = 1;
    p.cps = (int)((p.nchunks + S - 1) / S);
    if (p.cps < 1) p.cps = 1;
    p.S = (int)((p.nchunks + p.cps - 1) / p.cps);
    if (p.S < 1) p.S = 1;
    return p;
}

struct WsLayoutB {
    size_t oDx, oDp, oX, oY, oZ, oPart, oCol, total;  // bytes
};

inline WsLayoutB bwd_layout(long long R, long long U) {
    const SavedLayout s = saved_layout(R, U);
    const long long brow = kLead + s.rows;
    size_t part = 0;
    for (int l = 0; l < kLayers; ++l) {
        const WgPlan p = wg_plan(l, l < kTdnn ? s.live : U);
        const size_t f = (size_t)p.S * p.Mt * 128 * p.Nt * 128;
        part = f > part ? f : part;
    }
    WsLayoutB w;
    size_t o = 0;
    w.oDx = o;
    o = align256(o + (size_t)s.urows * kEmbDim * 4);
    w.oDp = o;
    o = align256(o + (size_t)s.urows * kPooledLd * 4);
    w.oX = o;
    o = align256(o + (size_t)brow * out_ld(kTdnn - 1) * 4);
    w.oY = o;
    o = align256(o + (size_t)brow * kEmbDim * 4);
    w.oZ = o;
    o = align256(o + (size_t)brow * kEmbDim * 4);
    w.oPart = o;
    o = align256(o + part * 4);
    w.oCol = o;
    w.total = align256(o + (size_t)kColSplits * out_ld(kTdnn - 1) * 8);
    return w;
}

// The argument checks of a backward entry point, in the order that is part of the ABI; the caller's grid limits
// (EUNSUPPORTED) and buffer sizes (ENOSPC) follow them, in that order.  *nothing: n_utts == 0, return OK.
inline int check_backward(int64_t n_utts, int64_t total_frames, int pooling, int64_t lddx, const void* saved,
                          const void* offsets, const void* dxvec, const void* packed, const void* packed_t,
                          const void* grad, const void* ws, bool* nothing) {
    *nothing = false;
    if (n_utts < 0 || total_frames < 0) return NPLDA_EINVAL;
    if (bad_pooling(pooling)) return NPLDA_EINVAL;
    *nothing = n_utts == 0;
    if (*nothing) return NPLDA_OK;
    if (!none_null({saved, offsets, dxvec, packed, packed_t, grad, ws}) ||
        !all_aligned16({saved, packed, packed_t, grad, ws}) || lddx < kEmbDim)
        return NPLDA_EINVAL;
    return NPLDA_OK;
}

// the backward's buffers, carved from the caller's `saved` (read) and workspace (written)
struct BwdBuffers {
    const char* sb;            // saved
    float *dx, *dpool;         // dxvec zero-padded to (urows, 512); dpooled (urows, 3008)
    float* part;               // split-K partials of the weight gradients
    double* colp;              // partials of the bias column sums
    float *bufX, *bufY, *bufZ; // brow rows each: dA10 (ld 1504), and the ping-pong pair of dA9..dA1 (ld 512)
    const float* pooled;
    long long brow;            // kLead zeroed rows, then the saved rows
};

inline BwdBuffers bwd_buffers(const SavedLayout& L, const WsLayoutB& W, const void* saved, void* ws) {
    const char* sb = (const char*)saved;
    char* wb = (char*)ws;
    return BwdBuffers{sb, (float*)(wb + W.oDx), (float*)(wb + W.oDp), (float*)(wb + W.oPart), (double*)(wb + W.oCol),
                      (float*)(wb + W.oX), (float*)(wb + W.oY), (float*)(wb + W.oZ), (const float*)(sb + L.oP),
                      kLead + L.rows};
}

// The data gradient of layer l (tdnn<l+1>, l >= 1): dA_l at dA, the layer's transposed image, negative taps; the result
// goes to a.out = the ping-pong buffer of dA_{l-1} behind its kLead zeroed rows, row stride 512.
inline GemmArgs data_grad_args(int l, const float* PT, const float* dA, long long ldA, const BwdBuffers& b,
                               long long live) {
    float* nxt = ((kTdnn - 1 - l) & 1 ? b.bufZ : b.bufY) + (size_t)kLead * kEmbDim;
    return gemm_args(PT, geomT(l, packedT_offset(l)), dA, ldA, nxt, kEmbDim, live, -kShape[l].d, 0);
}

// ---- defined in nplda_xvec_bwd.hip ---------------------------------------------------------------------------------

// Training forward, before the layer loop: the padded input image, rem[r] = frames left in row r's utterance (this one
// included, 0 outside every utterance), and the zeroed slack rows of the ten activation buffers of `saved`.
int train_forward_head(const float* x, int layout, long long ld_in, const int64_t* offsets, long long U, long long R,
                       const SavedLayout& L, char* saved, hipStream_t st);
// Training forward, after the layer loop: statistics pooling of the tdnn10 rows of `saved` into its pooled rows (padded
// with zero rows to whole tiles) and lin11 with the extraction epilogue into out.
int train_forward_tail(const float* P, const int64_t* offsets, long long U, long long R, int pooling,
                       const SavedLayout& L, char* saved, float* out, long long ldx, hipStream_t st);
// Backward, before the pooling backward: dxvec zero-padded, dW11 = dxvec^T pooled, db11 = sum dxvec, dpooled = dxvec W11
// (b.dpool), and the zeroed bufX and leading rows of bufY / bufZ.  *dA, *ldA: where dA10 goes (bufX behind its lead).
int backward_head(const BwdBuffers& b, const SavedLayout& L, long long U, const float* dxvec, long long lddx,
                  const float* PT, float* grad, hipStream_t st, float** dA, long long* ldA);
// dW_l and db_l of tdnn<l+1> from dA_l and the layer's saved input rows
int layer_param_grads(int l, const float* dA, long long ldA, const BwdBuffers& b, const SavedLayout& L, float* grad,
                      hipStream_t st);

}  // namespace nplda_xvec_train
