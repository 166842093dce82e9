// nplda_xvec.h — shape table and packed-image layout of the E-TDNN x-vector extractor (utils/models.py:29-214).
//
// Layers 0..9 are tdnn1..tdnn10 (TDNN: unfold c frames at dilation d, nn.Linear, ReLU, eval BatchNorm1d(affine=False));
// layer 10 is lin11 (nn.Linear(3000, 512), bias only) on the statistics-pooled rows.  Every layer is ONE GEMM of the
// same kernel (nplda_xvec.hip): rows are frames (utterances for lin11), K = c * Dinp, N = Dout.
//
// Padding: a layer's input width is padded to Dinp (a multiple of 16: tdnn1 30 -> 32, lin11 3000 -> 3008) so that every
// k16-block of the implicit unfold lies inside one context tap; the pad columns of the activations are zero and the
// packed weights are zero there.  K-blocks are padded to a multiple of the staging chunk (kXvecKC) and column blocks to
// a multiple of the slice width (kXvecNS); the padding of the weight image is zero and the kernel skips padded k-blocks.
//
// Packed image, per layer (offsets in floats, every array 16-byte aligned):
//   frag[kb][xb][lane][i] = W[16 xb + (lane & 15)][k(16 kb + 4 (lane >> 4) + i)]   kb < nkbp, xb < XBp
//       k(kp) = (kp / Dinp) * Din + kp % Dinp  when kp % Dinp < Din and kp / Dinp < c, else the entry is 0
//   bias[XBp * 16], mean[XBp * 16], inv[XBp * 16]   (inv = 1 / sqrt(running_var + eps); pads 0 / 0 / 1)
#pragma once
#include <stddef.h>

namespace nplda_xvec {

constexpr int kLayers = 11;   // tdnn1..tdnn10, lin11
constexpr int kTdnn = 10;
constexpr int kKC = 4;        // k16-blocks per staged weight chunk
constexpr int kNS = 8;        // 16-column blocks per column slice (128 output columns per block)
constexpr int kRowsPerBlock = 128;  // 4 waves x 32 rows
constexpr int kFeat = 30;     // MFCC features per frame
constexpr int kFeatP = 32;
constexpr int kContext = 22;  // frames an utterance loses through the stack: 4 + 4 + 6 + 8
constexpr int kRowSlack = 16; // rows past the last tile a layer may read (max d (c - 1) = 8)
constexpr int kPoolDim = 1500;
constexpr int kPoolLd = 16 * ((kPoolDim + 15) / 16);  // out_ld(kTdnn - 1) for device code (the windows pooling kernel)
constexpr int kPooledLd = 3008;
constexpr int kEmbDim = 512;

struct Layer {
    int Din, Dout, c, d;
};

constexpr Layer kShape[kLayers] = {
    {30, 512, 5, 1},  {512, 512, 1, 1}, {512, 512, 3, 2}, {512, 512, 1, 1}, {512, 512, 3, 3}, {512, 512, 1, 1},
    {512, 512, 3, 4}, {512, 512, 1, 1}, {512, 512, 1, 1}, {512, 1500, 1, 1}, {3000, 512, 1, 1},
};

struct LayerGeom {
    int Din, Dout, c, d, Dinp, Kp, nkb, nkbp, XB, XBp, Np;
    size_t oFrag, oBias, oMean, oInv, end;
};

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

inline LayerGeom geom_of(const Layer s, size_t start) {
    LayerGeom g;
    g.Din = s.Din; g.Dout = s.Dout; g.c = s.c; g.d = s.d;
    g.Dinp = round_up(s.Din, 16);
    g.Kp = s.c * g.Dinp;
    g.nkb = g.Kp / 16;
    g.nkbp = round_up(g.nkb, kKC);
    g.XB = (s.Dout + 15) / 16;
    g.XBp = round_up(g.XB, kNS);
    g.Np = 16 * g.XB;
    g.oFrag = start;
    g.oBias = g.oFrag + (size_t)g.nkbp * g.XBp * 256;
    g.oMean = g.oBias + (size_t)g.XBp * 16;
    g.oInv = g.oMean + (size_t)g.XBp * 16;
    g.end = g.oInv + (size_t)g.XBp * 16;
    return g;
}

inline LayerGeom geom(int l, size_t start) { return geom_of(kShape[l], start); }

inline size_t packed_floats() {
    size_t o = 0;
    for (int l = 0; l < kLayers; ++l) o = geom(l, o).end;
    return o;
}

// layer l inside the packed image
inline LayerGeom geomF(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o = geom(i, o).end;
    return geom(l, o);
}

// ---- workspace arithmetic shared by extraction and the two training paths ------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline long long whole_tiles(long long n) { return (n + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock; }
inline int out_ld(int l) { return l == kTdnn - 1 ? kPoolLd : kEmbDim; }  // row stride of tdnn<l+1>'s output

}  // namespace nplda_xvec
