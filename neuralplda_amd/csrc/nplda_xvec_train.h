// nplda_xvec_train.h — what the two training paths of the E-TDNN extractor share: the running-statistics path
// (nplda_xvec_bwd.hip) and the batch-statistics path (nplda_xvec_bn.hip).  Buffer layouts and index helpers are inline;
// the launchers of the weight-gradient, column-sum, plain-store GEMM and row-index kernels are defined once, in
// nplda_xvec_bwd.hip, next to their kernels (the library's version script keeps them out of the dynamic symbol table).
#pragma once
#include "nplda_xvec_body.h"

namespace nplda_xvec_train {

using namespace nplda_xvec;

constexpr int kCtx[kTdnn] = {4, 4, 8, 8, 14, 14, 22, 22, 22, 22};  // frames lost through tdnn1..tdnn<l+1>
constexpr int kLead = 16;     // zeroed rows in front of every dA buffer (>= max d (c - 1) = 8)
constexpr int kWgKC = 16;     // frames per staged wgrad chunk
constexpr int kWgTargetBlocks = 512;
constexpr int kColSplits = 1024;  // row splits of the bias column sums (enough blocks to stream dA at bandwidth)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int out_ld(int l) { return l == kTdnn - 1 ? 16 * ((kPoolDim + 15) / 16) : kEmbDim; }

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
inline LayerGeom geomF(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o = geom(i, o).end;
    return geom(l, o);
}

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
    s.live = (R + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock;
    s.rows = s.live + kRowSlack;
    s.urows = (U + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock;
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

inline GemmArgs gemm_args(const float* img, const LayerGeom& G, const float* in, long long ld_in, float* out,
                          long long ld_out, long long row_limit, int dil, int relu_bn) {
    GemmArgs a;
    a.in = in; a.ld_in = ld_in;
    a.frag = reinterpret_cast<const f32x4*>(img + G.oFrag);
    a.bias = img + G.oBias; a.mean = img + G.oMean; a.inv = img + G.oInv;
    a.out = out; a.ld_out = ld_out; a.row_limit = row_limit;
    a.nkb = G.nkb; a.nkbp = G.nkbp; a.XBp = G.XBp; a.Np = G.Np; a.kbt = G.Dinp / 16; a.dil = dil;
    a.relu_bn = relu_bn;
    return a;
}

// ---- launchers defined in nplda_xvec_bwd.hip ---------------------------------------------------------------------

// rem[r] = frames left in row r's utterance (this one included), 0 outside every utterance, for r < rows
int launch_rem(const int64_t* offsets, long long U, long long R, long long rows, int* rem, hipStream_t st);
// the GEMM with the extraction epilogue (bias, and ReLU / running-statistics batch norm when a.relu_bn)
int launch_gemm_extract(const GemmArgs& a, long long rows, hipStream_t st);
// dW_l (torch layout) from dA rows and the layer's input rows: split-K partials in `part`, summed in split order
int launch_wgrad(int l, const float* A, long long lda, int acols, const float* B, long long ldb, long long kmax,
                 float* part, float* out, hipStream_t st);
// out[col] = sum over nrows of A[:, col]: fp64 partials in `part` (kColSplits x N doubles at most), fixed order
int launch_colsum(const float* A, long long lda, long long nrows, int N, double* part, float* out, hipStream_t st);

}  // namespace nplda_xvec_train
