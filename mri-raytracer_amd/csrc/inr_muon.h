// Muon (csrc/inr_muon.hip): the per-layer table of the Newton-Schulz products, their operand views and the scratch layouts,
// written once for the device kernels and for the host (tests/native/inr_muon_harness.hip walks them under AddressSanitizer +
// UBSan over buffers of exactly the real sizes).  DESIGN.md section 17.
//
// A weight matrix is W[in][out], row-major, at wOff in the flat layout of mrirt_inr_forward_f32.  Newton-Schulz iterates on
// X (r x c, r <= c): W's own shape when in <= out, its transpose otherwise.  X is never moved in memory: element (i, j) of X
// is p[wOff + i sR + j sC] with (sR, sC) = (out, 1) or (1, out), so every buffer that holds an X keeps the flat layout and
// "transpose back" costs nothing.  The Gram matrices A = X X^T and B = c1 A + c2 A A are r x r, row-major, at gOff.
#pragma once
#include <math.h>
#include <stdint.h>

#include "inr_optim.h"

namespace mrirt {

constexpr uint32_t kMuonThreads = 256;
constexpr uint32_t kMuonMaxSteps = 16;
constexpr int kMuonBN = 64;                   // every product runs the 64 x 64 block tile: one launch serves all layers

struct MuonLayer {
    uint32_t in, out, r, c, wOff, gOff;
    int64_t sR, sC;
    float scale;                 // sqrt(max(1, out / in)), fp64 on the host, rounded once
    uint32_t pad;
};

struct MuonPlan {
    uint32_t numLayers, maxR, maxC, pad;
    uint64_t nw, nb, gramElems;
    MuonLayer layer[kTrMaxLayers];
};

MRIRT_HD MuonPlan muon_plan(uint32_t numLayers, uint32_t inDim, uint32_t hidden, uint32_t outDim) {
    MuonPlan P = {};
    P.numLayers = numLayers;
    uint32_t w = 0, g = 0, b = 0;
    for (uint32_t l = 0; l < numLayers && l < (uint32_t)kTrMaxLayers; ++l) {
        MuonLayer& y = P.layer[l];
        y.in = l == 0 ? inDim : hidden;
        y.out = l + 1 >= numLayers ? outDim : hidden;
        const bool t = y.in > y.out;
        y.r = t ? y.out : y.in; y.c = t ? y.in : y.out;
        y.sR = t ? 1 : (int64_t)y.out; y.sC = t ? (int64_t)y.out : 1;
        y.wOff = w; y.gOff = g;
        const double ratio = (double)y.out / (double)y.in;
        y.scale = (float)sqrt(ratio > 1.0 ? ratio : 1.0);
        w += y.in * y.out; g += y.r * y.r; b += y.out;
        if (y.r > P.maxR) P.maxR = y.r;
        if (y.c > P.maxC) P.maxC = y.c;
    }
    P.nw = w; P.nb = b; P.gramElems = g;
    return P;
}

// the layer that flat weight element i belongs to
MRIRT_HD uint32_t muon_layer_of(const MuonPlan& P, int64_t i) {
    uint32_t l = P.numLayers - 1;
    while (l > 0 && i < (int64_t)P.layer[l].wOff) --l;
    return l;
}

// Scratch of mrirt_muon_step, in bytes from its start (every region 256-B aligned):
//   [norm partial sums (opt_scratch_bytes)][m^: nw][O: nw] | [denominators: kTrMaxLayers doubles][X ping: nw][X pong: nw][A][B]
// mrirt_muon_orthogonalize uses the part behind the bar, at offNs of the same buffer.
struct MuonLayout {
    uint64_t offMhat, offO, offNs, offDenom, offX0, offX1, offA, offB, bytes;
};
MRIRT_HD MuonLayout muon_layout(const MuonPlan& P) {
    MuonLayout L;
    const uint64_t mat = tr_align(P.nw * sizeof(float)), gram = tr_align(P.gramElems * sizeof(float));
    L.offMhat = opt_scratch_bytes((int64_t)(P.nw + P.nb));
    L.offO = L.offMhat + mat;
    L.offNs = L.offO + mat;
    L.offDenom = L.offNs;
    L.offX0 = L.offDenom + tr_align(kTrMaxLayers * sizeof(double));
    L.offX1 = L.offX0 + mat;
    L.offA = L.offX1 + mat;
    L.offB = L.offA + gram;
    L.bytes = L.offB + gram;
    return L;
}

// One Newton-Schulz product of one layer through the GEMM of inr_gemm.h: C[row cR + col cC] = epilogue(acc, D[same offset])
struct MuonGemm {
    TrView A, B;
    const float* D;
    float* C;
    int64_t cR, cC;
    uint32_t M, N;
    int64_t K;
};
// A = X X^T: both operands are X with k along its columns
MRIRT_HD MuonGemm muon_gram_args(const MuonLayer& y, const float* X, float* A) {
    MuonGemm g = {};
    g.A = TrView{ X + y.wOff, y.sR, y.sC, y.r, 0u };
    g.B = g.A;
    g.C = A + y.gOff; g.cR = y.r; g.cC = 1;
    g.M = y.r; g.N = y.r; g.K = y.c;
    return g;
}
// B = c1 A + c2 (A A)
MRIRT_HD MuonGemm muon_poly_args(const MuonLayer& y, const float* A, float* B) {
    MuonGemm g = {};
    g.A = TrView{ A + y.gOff, (int64_t)y.r, 1, y.r, 0u };
    g.B = TrView{ A + y.gOff, 1, (int64_t)y.r, y.r, 0u };
    g.D = A + y.gOff;
    g.C = B + y.gOff; g.cR = y.r; g.cC = 1;
    g.M = y.r; g.N = y.r; g.K = y.r;
    return g;
}
// X' = c0 X + B X, written in X's own layout
MRIRT_HD MuonGemm muon_update_args(const MuonLayer& y, const float* B, const float* X, float* Xn) {
    MuonGemm g = {};
    g.A = TrView{ B + y.gOff, (int64_t)y.r, 1, y.r, 0u };
    g.B = TrView{ X + y.wOff, y.sC, y.sR, y.c, 0u };
    g.D = X + y.wOff;
    g.C = Xn + y.wOff; g.cR = y.sR; g.cC = y.sC;
    g.M = y.r; g.N = y.c; g.K = y.r;
    return g;
}
// block tiles of the launch that serves every layer: x over rows, y over columns, z = layer; a block outside its layer's
// own tile range returns at once
MRIRT_HD uint32_t muon_tiles(uint32_t extent, uint32_t tile) { return (extent + tile - 1) / tile; }

}  // namespace mrirt
