// INR training step (csrc/inr_train.hip): the index arithmetic of its fp32-MFMA GEMMs, of the split-n slabs and of the
// scratch layout, written once for the device kernels and for the host (tests/native/inr_train_harness.hip walks it under
// AddressSanitizer + UBSan over buffers of exactly the real sizes).
//
// One GEMM template serves the three products of a layer.  Both operands are "views": an element is
// addressed by its non-k index (a row of the result for the A operand, a column for the B operand) and its k index,
//     H . W      A = h[n][in]   (non = point, k = input)    B = W[in][out] (non = output, k = input)
//     dZ . W^T   A = dz[n][out] (non = point, k = output)   B = W[in][out] (non = input,  k = output)
//     H^T . dZ   A = h[n][in]   (non = input, k = point)    B = dz[n][out] (non = output, k = point)
// and the last one carries one more A row of ones, so that db = sum_p dz is row `in` of the same product.
#pragma once
#include <stdint.h>

#include "mrirt_device.h"

namespace mrirt {

constexpr int kTrThreads = 256;               // 4 waves; wave w owns rows 16 w .. 16 w + 15 of the 64-row block tile
constexpr int kTrBM = 64;                     // block tile rows
constexpr int kTrBK = 16;                     // k depth of one staged tile: four 16x16x4 MFMA steps
constexpr int kTrMaxLayers = 8;
constexpr uint32_t kTrSlabMin = 256;          // points per slab of H^T . dZ; doubled until at most kTrMaxSlabs slabs cover n
constexpr uint32_t kTrMaxSlabs = 64;
constexpr uint32_t kLossThreads = 256;
constexpr uint32_t kLossMaxBlocks = 256;
constexpr uint32_t kLossMaxClasses = 16;
// per block (and once more for the totals): sum probs, sum probs y, count, sum ce y per class; then sum ce cw[label]
constexpr uint32_t kLossVals = 4 * kLossMaxClasses + 1;

MRIRT_HD uint64_t tr_align(uint64_t bytes) { return (bytes + 255u) & ~(uint64_t)255u; }

MRIRT_HD uint32_t tr_slab_len(int64_t n) {
    uint64_t len = kTrSlabMin;
    while (((uint64_t)n + len - 1) / len > kTrMaxSlabs) len *= 2;
    return (uint32_t)len;
}
MRIRT_HD uint32_t tr_slabs(int64_t n) { const uint64_t len = tr_slab_len(n); return (uint32_t)(((uint64_t)n + len - 1) / len); }

MRIRT_HD uint32_t loss_blocks(int64_t n) {
    const uint64_t b = ((uint64_t)n + kLossThreads - 1) / kLossThreads;
    return (uint32_t)(b < kLossMaxBlocks ? b : kLossMaxBlocks);
}
// doubles: [loss_blocks(n)][kLossVals] partial sums, then [kLossVals] totals
MRIRT_HD uint64_t loss_scratch_bytes(int64_t n) { return tr_align((uint64_t)(loss_blocks(n) + 1) * kLossVals * sizeof(double)); }

// Scratch of one training step, in bytes from its start (every region 256-B aligned):
//   [loss sums][x: n x inDim][h_0 .. h_{L-2}: n x hidden each][dz ping, dz pong: n x hidden each][slabs x slabElems]
struct TrainLayout {
    uint32_t numLayers, inDim, hidden, outDim;
    uint32_t in[kTrMaxLayers], out[kTrMaxLayers];
    uint32_t wOff[kTrMaxLayers], bOff[kTrMaxLayers];     // into the unpadded fp32 weight / bias arrays (and their gradients)
    uint32_t slabLen, slabs;
    uint64_t slabElems;                                  // floats of one slab: the largest (in + 1) x out of the network
    uint64_t offX, offH, offDz, offSlab, bytes;
};

MRIRT_HD TrainLayout train_layout(uint32_t numLayers, uint32_t inDim, uint32_t hidden, uint32_t outDim, int64_t n) {
    TrainLayout L;
    L.numLayers = numLayers; L.inDim = inDim; L.hidden = hidden; L.outDim = outDim;
    uint32_t w = 0, b = 0;
    L.slabElems = 0;
    for (uint32_t l = 0; l < (uint32_t)kTrMaxLayers; ++l) {
        L.in[l] = l == 0 ? inDim : hidden;
        L.out[l] = l + 1 >= numLayers ? outDim : hidden;
        L.wOff[l] = w; L.bOff[l] = b;
        if (l < numLayers) {
            w += L.in[l] * L.out[l];
            b += L.out[l];
            const uint64_t e = (uint64_t)(L.in[l] + 1) * L.out[l];
            if (e > L.slabElems) L.slabElems = e;
        }
    }
    L.slabLen = tr_slab_len(n);
    L.slabs = tr_slabs(n);
    const uint64_t act = tr_align((uint64_t)n * hidden * sizeof(float));
    L.offX = loss_scratch_bytes(n);
    L.offH = L.offX + tr_align((uint64_t)n * inDim * sizeof(float));
    L.offDz = L.offH + (uint64_t)(numLayers - 1) * act;
    L.offSlab = L.offDz + 2 * act;
    // room for the most slabs any smaller n uses (the count drops where the slab length doubles): the size is monotone in n
    const uint64_t most = ((uint64_t)n + kTrSlabMin - 1) / kTrSlabMin;
    L.bytes = L.offSlab + tr_align((most < kTrMaxSlabs ? most : kTrMaxSlabs) * L.slabElems * sizeof(float));
    return L;
}
MRIRT_HD uint64_t train_act_bytes(const TrainLayout& L, int64_t n) { return tr_align((uint64_t)n * L.hidden * sizeof(float)); }

// One GEMM operand: element (non, k) is p[non * sNon + k * sK] for non < nonDim and kBegin <= k < kEnd; with `ones`, row
// non == nonDim reads 1; everything else reads 0 (tile tails).
struct TrView {
    const float* p;
    int64_t sNon, sK;
    uint32_t nonDim, ones;
};

// What thread t stages for its i-th element of a (R non-k indices) x (kTrBK k indices) tile, R = 64 or 16: R / 16 elements
// per thread.  KFAST (k is the contiguous index in memory): 16 neighbouring threads read 16 neighbouring k; otherwise R
// neighbouring threads read R neighbouring non-k indices.
template <int R, bool KFAST>
MRIRT_HD void tr_stage_coord(uint32_t t, int i, uint32_t& r, uint32_t& k) {
    if (KFAST) { k = t & 15u; r = (t >> 4) + 16u * (uint32_t)i; }
    else       { r = t % (uint32_t)R; k = t / (uint32_t)R + (uint32_t)(kTrThreads / R) * (uint32_t)i; }
}

// Offset of element (non, k) inside the view, or -1: reads 0, -2: reads 1 (the ones row).
MRIRT_HD int64_t tr_view_offset(const TrView& v, uint32_t non, int64_t k, int64_t kEnd) {
    if (k >= kEnd) return -1;
    if (non < v.nonDim) return (int64_t)non * v.sNon + k * v.sK;
    return (non == v.nonDim && v.ones) ? -2 : -1;
}

// One launch of the GEMM template.  The epilogue is the kernel's template parameter: bias (+ ReLU), mask, or slab.
struct TrGemmArgs {
    TrView A, B;
    uint32_t M, N;               // result rows (A's non-k extent, the ones row included) and columns
    int64_t K;                   // k extent; slab form: the number of points, split into slabs of slabLen by blockIdx.z
    uint32_t slabLen;
    float* C;                    // bias / mask forms: [M][ldc]; slab form: [slab][M][N]
    int64_t ldc;
    uint64_t slabStride;
    const float* bias;           // bias form
    uint32_t relu;
    const float* mask;           // mask form: the saved activation of the layer below, [M][ldc]; gradient passes where it is > 0
                                 // cosine-scale form (SIREN): the saved cosine of the layer below, [M][ldc]; C = v * mask
    float* cosOut;               // sine form (SIREN): cos of the pre-activation, [M][ldc] beside C = sin
};

// Scratch offset of layer l's input: x for layer 0, else the saved h_{l-1} (which the forward of layer l - 1 writes)
MRIRT_HD uint64_t tr_in_offset(const TrainLayout& L, uint32_t l, int64_t n) {
    return l == 0 ? L.offX : L.offH + (uint64_t)(l - 1) * train_act_bytes(L, n);
}
// Scratch offset of dz_{l-1}, which the backward of layer l writes: the two buffers alternate down the layers
MRIRT_HD uint64_t tr_dz_offset(const TrainLayout& L, uint32_t l, int64_t n) {
    return L.offDz + (uint64_t)((L.numLayers - l) & 1u) * train_act_bytes(L, n);
}

// The three launches of layer l exactly as the library issues them; the sanitizer harness replays these same arguments.
// H . W + b (ReLU below the head): h is layer l's input, C its output (the logits for the head)
MRIRT_HD TrGemmArgs tr_forward_args(const TrainLayout& L, uint32_t l, int64_t n, const float* h, const float* w, const float* b, float* C) {
    TrGemmArgs a = {};
    a.A = TrView{ h, (int64_t)L.in[l], 1, (uint32_t)n, 0u };
    a.B = TrView{ w + L.wOff[l], 1, (int64_t)L.out[l], L.out[l], 0u };
    a.M = (uint32_t)n; a.N = L.out[l]; a.K = L.in[l];
    a.C = C; a.ldc = L.out[l];
    a.bias = b + L.bOff[l];
    a.relu = l + 1 == L.numLayers ? 0u : 1u;
    return a;
}
// H^T . dZ into slabs, db as the row of ones
MRIRT_HD TrGemmArgs tr_slab_args(const TrainLayout& L, uint32_t l, int64_t n, const float* hin, const float* dz, float* slab) {
    TrGemmArgs g = {};
    g.A = TrView{ hin, 1, (int64_t)L.in[l], L.in[l], 1u };
    g.B = TrView{ dz, 1, (int64_t)L.out[l], L.out[l], 0u };
    g.M = L.in[l] + 1; g.N = L.out[l]; g.K = n; g.slabLen = L.slabLen;
    g.C = slab; g.slabStride = L.slabElems;
    return g;
}
// dZ . W^T, masked by layer l's input
MRIRT_HD TrGemmArgs tr_mask_args(const TrainLayout& L, uint32_t l, int64_t n, const float* dz, const float* w, const float* hin, float* dzPrev) {
    TrGemmArgs d = {};
    d.A = TrView{ dz, (int64_t)L.out[l], 1, (uint32_t)n, 0u };
    d.B = TrView{ w + L.wOff[l], (int64_t)L.out[l], 1, L.in[l], 0u };
    d.M = (uint32_t)n; d.N = L.in[l]; d.K = L.out[l];
    d.C = dzPrev; d.ldc = L.in[l];
    d.mask = hin;
    return d;
}
// Element i of a reduced slab ((in + 1) x out): rows < in are dW, row in is db
MRIRT_HD float* tr_reduce_dst(uint32_t i, uint32_t in, uint32_t out, float* gw, float* gb) {
    return i < in * out ? gw + i : gb + (i - in * out);
}

// ---- SIREN ---------------------------------------------------------------------------------------------
// The step's scratch is the ReLU step's with one more region behind it: c_0 .. c_{L-2}, the cosines of the hidden
// pre-activations (n x hidden each), which the forward's sine epilogue stores beside h_l and the backward multiplies by.
struct SirenLayout {
    TrainLayout T;               // T.bytes: where the cosines start
    uint64_t offC, bytes;
};
MRIRT_HD SirenLayout siren_layout(uint32_t numLayers, uint32_t inDim, uint32_t hidden, uint32_t outDim, int64_t n) {
    SirenLayout S;
    S.T = train_layout(numLayers, inDim, hidden, outDim, n);
    S.offC = S.T.bytes;
    S.bytes = S.offC + (uint64_t)(numLayers - 1) * train_act_bytes(S.T, n);
    return S;
}
// Scratch offset of c_l, the cosine of hidden layer l's pre-activation (l < numLayers - 1)
MRIRT_HD uint64_t tr_cos_offset(const SirenLayout& S, uint32_t l, int64_t n) { return S.offC + (uint64_t)l * train_act_bytes(S.T, n); }
// H . W + b, then sin into C and cos into cosOut (hidden layers; the head is tr_forward_args, which is linear there)
MRIRT_HD TrGemmArgs tr_sine_args(const SirenLayout& S, uint32_t l, int64_t n, const float* h, const float* w, const float* b, float* C,
                                 float* cosOut) {
    TrGemmArgs a = tr_forward_args(S.T, l, n, h, w, b, C);
    a.relu = 0u;
    a.cosOut = cosOut;
    return a;
}
// dZ . W^T, times the cosine of the layer below (c_{l-1})
MRIRT_HD TrGemmArgs tr_cos_args(const SirenLayout& S, uint32_t l, int64_t n, const float* dz, const float* w, const float* cosPrev,
                                float* dzPrev) {
    return tr_mask_args(S.T, l, n, dz, w, cosPrev, dzPrev);
}
// Element i of x'[n][inDim] = w0 * x: where x comes from.  src 0: coords[off], 1: feats[off]
MRIRT_HD void tr_siren_feature_src(int64_t i, uint32_t inDim, uint32_t M, uint32_t raw, uint32_t& src, int64_t& off) {
    const int64_t p = i / inDim;
    const uint32_t f = (uint32_t)(i - p * inDim);
    if (raw) { src = 1; off = i; }
    else if (f < 3) { src = 0; off = 3 * p + f; }
    else { src = 1; off = p * M + (f - 3); }
}

// LDS image of a staged tile: [k][non] with a row pitch that spreads one MFMA operand read (4 k x 16 non) over 64 banks
template <int R> struct TrLds { static constexpr int pitch = R == 64 ? 80 : 16; };

// The MFMA tile (v_mfma_f32_16x16x4_f32): operand lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15];
// accumulator register r of lane l is C[row 4 (l >> 4) + r][col l & 15].
MRIRT_HD uint32_t tr_acc_row(uint32_t lane, int reg) { return 4u * (lane >> 4) + (uint32_t)reg; }
MRIRT_HD uint32_t tr_acc_col(uint32_t lane) { return lane & 15u; }

// k range of slab z of H^T . dZ
MRIRT_HD void tr_slab_range(int64_t n, uint32_t slabLen, uint32_t z, int64_t& k0, int64_t& k1) {
    k0 = (int64_t)z * slabLen;
    k1 = k0 + slabLen < n ? k0 + slabLen : n;
}

}  // namespace mrirt
