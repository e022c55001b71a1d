// Coordinate-injection INR (csrc/inr_inject.hip): the index arithmetic of its scratch, of the layer
// GEMM's A operand, of the dropout mask and of the chunk walk over a volume, written once for the device kernels and for the
// host (tests/native/inject_harness.hip walks it under AddressSanitizer + UBSan over buffers of exactly the real sizes).
//
// The A operand of hidden layer l is the row [h_{l-1} | coords | mods] of the notebook's jnp.concatenate, never copied
// together: a three-part view picks, per k, the previous activation (k < split), the point's coordinates (split <= k <
// splitM) or its modalities (splitM <= k < K).  Layer 0 is the same view with the Fourier features as `h` and no coords.
//
// The training step (csrc/inr_inject_train.hip) adds its scratch layout, the same view with the roles
// swapped (k = the point) for X^T . dZ, and the arguments of its launches (tests/native/inject_train_harness.hip replays them).
#pragma once
#include <stdint.h>

#include "inr_optim.h"

namespace mrirt {

constexpr uint32_t kInjMaxLayers = 8, kInjMaxWidth = 256, kInjMaxFourier = 256, kInjMaxMods = 8, kInjMaxClasses = 16;
constexpr uint32_t kInjMaxSamples = 64;
constexpr uint32_t kInjMaxSampleIndex = 1u << 24;        // 256 s + l stays a 32-bit counter word
constexpr uint32_t kInjThreads = 256;

// The network as the kernels see it: in[l] / out[l] / split[l] / splitM[l] per layer, offsets into the unpadded arrays
struct InjNet {
    uint32_t numLayers, F, M, C, maxHidden;
    uint32_t in[kInjMaxLayers], out[kInjMaxLayers];
    uint32_t split[kInjMaxLayers], splitM[kInjMaxLayers];      // k < split: h;  split <= k < splitM: coords;  splitM <= k: mods
    uint32_t wOff[kInjMaxLayers], bOff[kInjMaxLayers];
    uint32_t nw, nb;
};

// 0 when the shape is one the entry points take (include/mrirt.h), else -5 (MRIRT_ERR_ARG)
MRIRT_HD int inj_check_shape(uint32_t L, uint32_t F, uint32_t M, const uint32_t* width, uint32_t coordLayers, uint32_t modLayers) {
    if (L < 2 || L > kInjMaxLayers) return -5;
    if (F < 2 || F > kInjMaxFourier || (F & 1u) != 0 || M > kInjMaxMods) return -5;
    for (uint32_t l = 0; l < L; ++l)
        if (width[l] < 1 || width[l] > kInjMaxWidth) return -5;
    if (width[L - 1] > kInjMaxClasses) return -5;
    uint32_t allowed = 0;
    for (uint32_t l = 1; l + 1 < L; ++l) allowed |= 1u << l;
    if ((coordLayers & ~allowed) != 0 || (modLayers & ~allowed) != 0) return -5;
    return 0;
}

MRIRT_HD InjNet inj_net(uint32_t L, uint32_t F, uint32_t M, const uint32_t* width, uint32_t coordLayers, uint32_t modLayers) {
    InjNet N = {};
    N.numLayers = L; N.F = F; N.M = M; N.C = width[L - 1];
    uint32_t w = 0, b = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t prev = l == 0 ? F : width[l - 1];
        const bool cj = l > 0 && ((coordLayers >> l) & 1u), mj = l == 0 || ((modLayers >> l) & 1u);
        N.split[l] = prev;
        N.splitM[l] = prev + (cj ? 3u : 0u);
        N.in[l] = N.splitM[l] + (mj ? M : 0u);
        N.out[l] = width[l];
        N.wOff[l] = w; N.bOff[l] = b;
        w += N.in[l] * N.out[l];
        b += N.out[l];
        if (l + 1 < L && width[l] > N.maxHidden) N.maxHidden = width[l];
    }
    N.nw = w; N.nb = b;
    return N;
}

// Scratch of n points, in bytes from its start (every region 256-B aligned):
//   [coords n x 3][features n x F][act ping, act pong: n x maxHidden each][logits n x C][probability sums n x C]
struct InjLayout { uint64_t offCoords, offFeat, offAct, actBytes, offLogits, offMean, bytes; };

MRIRT_HD InjLayout inj_layout(const InjNet& N, int64_t n) {
    InjLayout L;
    L.offCoords = 0;
    L.offFeat = tr_align((uint64_t)n * 3 * sizeof(float));
    L.offAct = L.offFeat + tr_align((uint64_t)n * N.F * sizeof(float));
    L.actBytes = tr_align((uint64_t)n * N.maxHidden * sizeof(float));
    L.offLogits = L.offAct + 2 * L.actBytes;
    L.offMean = L.offLogits + tr_align((uint64_t)n * N.C * sizeof(float));
    L.bytes = L.offMean + tr_align((uint64_t)n * N.C * sizeof(float));
    return L;
}
// output of hidden layer l (l <= L - 2): the two buffers alternate
MRIRT_HD uint64_t inj_act_offset(const InjLayout& L, uint32_t l) { return L.offAct + (uint64_t)(l & 1u) * L.actBytes; }

// The A operand: three TrViews side by side along k
struct InjView {
    TrView h, c, m;
    uint32_t split, splitM;
};

// Which source holds element (row, k) of the view and where: 0 h, 1 coords, 2 mods; -1: reads 0 (tile tails)
MRIRT_HD int inj_view_src(const InjView& v, uint32_t row, int64_t k, int64_t K, int64_t& off) {
    off = -1;
    if (k >= K) return -1;
    if (k < (int64_t)v.split) { off = tr_view_offset(v.h, row, k, v.split); return off >= 0 ? 0 : -1; }
    if (k < (int64_t)v.splitM) { off = tr_view_offset(v.c, row, k - v.split, 3); return off >= 0 ? 1 : -1; }
    off = tr_view_offset(v.m, row, k - v.splitM, K - v.splitM);
    return off >= 0 ? 2 : -1;
}

// Layer l's A operand over n rows.  h: the layer's first part (features or the previous activation, [n][split]); coords:
// [n][3]; mods: element (row, m) at mods[row * modRow + m * modCol] ([n][M] for the point entry points, a window of
// [M][H][W][D] for a volume chunk)
MRIRT_HD InjView inj_layer_view(const InjNet& N, uint32_t l, int64_t n, const float* h, const float* coords, const float* mods,
                                int64_t modRow, int64_t modCol) {
    InjView v;
    v.split = N.split[l]; v.splitM = N.splitM[l];
    v.h = TrView{ h, (int64_t)N.split[l], 1, (uint32_t)n, 0u };
    v.c = TrView{ coords, 3, 1, (uint32_t)n, 0u };
    v.m = TrView{ mods, modRow, modCol, (uint32_t)n, 0u };
    return v;
}

// ---- dropout --------------------------------------------------------------------------------------------------------------------
// thr = floor(keep 2^32); keep == 1 (no mask at all) never comes here
MRIRT_HD uint32_t inj_threshold(float keep) { return (uint32_t)((double)keep * 4294967296.0); }

// the mask word of (global point i, layer l, unit j) of sample s
MRIRT_HD uint32_t inj_mask_word(uint64_t seed, uint64_t i, uint32_t s, uint32_t l, uint32_t j) {
    uint32_t c[4] = { (uint32_t)i, (uint32_t)(i >> 32), 256u * s + l, j >> 2 };
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return c[j & 3u];
}

// ---- training step (csrc/inr_inject_train.hip) -----------------------------------------------------------
// Scratch of one step over n points, in bytes from its start (every region 256-B aligned).  The first region is the loss
// prefix of mrirt_inr_loss, so forward, loss and backward share one buffer:
//   [loss sums][features n x F][h_0 .. h_{L-2} after dropout: n x width[l] each][dz ping, dz pong: n x maxHidden each]
//   [feature gradient n x F (g overwrites its first half row by row)][c01 n x 3][slabs x slabElems]
struct InjTrainLayout {
    uint64_t offFeat, offH[kInjMaxLayers], offDz, dzBytes, offDF, offC01, offSlab, bytes;
    uint64_t slabElems;                                  // floats of one slab: the largest (in + 1) x out, or F / 2 x 3 for dB
    uint32_t slabLen, slabs;
};

MRIRT_HD InjTrainLayout inj_train_layout(const InjNet& N, int64_t n) {
    InjTrainLayout T = {};
    T.slabElems = (uint64_t)(N.F / 2) * 3;
    for (uint32_t l = 0; l < N.numLayers; ++l) {
        const uint64_t e = (uint64_t)(N.in[l] + 1) * N.out[l];
        if (e > T.slabElems) T.slabElems = e;
    }
    T.slabLen = tr_slab_len(n);
    T.slabs = tr_slabs(n);
    T.offFeat = loss_scratch_bytes(n);
    uint64_t at = T.offFeat + tr_align((uint64_t)n * N.F * sizeof(float));
    for (uint32_t l = 0; l + 1 < N.numLayers; ++l) {
        T.offH[l] = at;
        at += tr_align((uint64_t)n * N.out[l] * sizeof(float));
    }
    T.dzBytes = tr_align((uint64_t)n * N.maxHidden * sizeof(float));
    T.offDz = at;
    T.offDF = T.offDz + 2 * T.dzBytes;
    T.offC01 = T.offDF + tr_align((uint64_t)n * N.F * sizeof(float));
    T.offSlab = T.offC01 + tr_align((uint64_t)n * 3 * sizeof(float));
    // room for the most slabs any smaller n uses (the count drops where the slab length doubles): the size is monotone in n
    const uint64_t most = ((uint64_t)n + kTrSlabMin - 1) / kTrSlabMin;
    T.bytes = T.offSlab + tr_align((most < kTrMaxSlabs ? most : kTrMaxSlabs) * T.slabElems * sizeof(float));
    return T;
}
// dz_{l-1}, which the backward of layer l >= 1 writes: the two buffers alternate down the layers
MRIRT_HD uint64_t inj_dz_offset(const InjNet& N, const InjTrainLayout& T, uint32_t l) {
    return T.offDz + (uint64_t)((N.numLayers - l) & 1u) * T.dzBytes;
}

// The A operand of X^T . dZ: the three-part view with the roles swapped.  k is the point, the non-k index runs over
// h | coords | mods and, with `ones`, one more row that reads 1 (db rides with dW).  g^T . c01 is the same view with h = g
// alone (rows of pitch hRow = F, split = splitM = in = F / 2, no ones).
struct InjViewT {
    const float *h, *c, *m;
    int64_t hRow, mRow;                                  // floats from one point's h / mods row to the next
    uint32_t split, splitM, in, ones;
};

// Which source holds element (non, k) and where: 0 h, 1 coords, 2 mods, 3: reads 1; -1: reads 0 (tile tails)
MRIRT_HD int inj_viewT_src(const InjViewT& v, uint32_t non, int64_t k, int64_t kEnd, int64_t& off) {
    off = -1;
    if (k >= kEnd) return -1;
    if (non < v.split) { off = k * v.hRow + non; return 0; }
    if (non < v.splitM) { off = k * 3 + (non - v.split); return 1; }
    if (non < v.in) { off = k * v.mRow + (non - v.splitM); return 2; }
    return (non == v.in && v.ones) ? 3 : -1;
}

struct InjSlabArgs {
    InjViewT A;
    TrView B;                    // dz [n][out] (non = unit, k = point), or c01 [n][3]
    uint32_t M, N;               // rows (A's non-k extent, the ones row included) and columns
    int64_t K;                   // the points, split into slabs of slabLen by blockIdx.z
    uint32_t slabLen;
    float* C;                    // [slab][M][N]
    uint64_t slabStride;
};

struct InjDzArgs {
    TrView A, B;                 // dz [n][out] (non = point, k = unit);  the first N rows of W [in][out] (non = input, k = unit)
    uint32_t M, N;
    int64_t K;
    float* C;                    // [M][N]
    const float* act;            // mask forms: the saved post-dropout activation [M][N]; the gradient passes where it is > 0
    float scale;                 // mask-and-scale form: 1.0f / keep
};

// The launches of layer l exactly as the library issues them; the sanitizer harness replays these same arguments.
// x_l^T . dz_l into slabs: x_l = [hin | coords | mods] with one more row of ones
MRIRT_HD InjSlabArgs inj_slab_args(const InjNet& N, const InjTrainLayout& T, uint32_t l, int64_t n, const float* hin, const float* coords,
                                   const float* mods, const float* dz, float* slab) {
    InjSlabArgs g = {};
    g.A = InjViewT{ hin, coords, mods, (int64_t)N.split[l], (int64_t)N.M, N.split[l], N.splitM[l], N.in[l], 1u };
    g.B = TrView{ dz, 1, (int64_t)N.out[l], N.out[l], 0u };
    g.M = N.in[l] + 1; g.N = N.out[l]; g.K = n; g.slabLen = T.slabLen;
    g.C = slab; g.slabStride = T.slabElems;
    return g;
}
// g^T . c01 into slabs: g lies in the first half of the feature gradient's rows
MRIRT_HD InjSlabArgs inj_slab_args_B(const InjNet& N, const InjTrainLayout& T, int64_t n, const float* g, const float* c01, float* slab) {
    InjSlabArgs s = {};
    s.A = InjViewT{ g, nullptr, nullptr, (int64_t)N.F, 0, N.F / 2, N.F / 2, N.F / 2, 0u };
    s.B = TrView{ c01, 1, 3, 3u, 0u };
    s.M = N.F / 2; s.N = 3; s.K = n; s.slabLen = T.slabLen;
    s.C = slab; s.slabStride = T.slabElems;
    return s;
}
// dz_l . W_l^T over the first split[l] rows of W_l (the injected rows get no gradient); act: h_{l-1} for l >= 1
MRIRT_HD InjDzArgs inj_dz_args(const InjNet& N, uint32_t l, int64_t n, const float* dz, const float* w, const float* act, float scale,
                               float* out) {
    InjDzArgs d = {};
    d.A = TrView{ dz, (int64_t)N.out[l], 1, (uint32_t)n, 0u };
    d.B = TrView{ w + N.wOff[l], (int64_t)N.out[l], 1, N.split[l], 0u };
    d.M = (uint32_t)n; d.N = N.split[l]; d.K = N.out[l];
    d.C = out; d.act = act; d.scale = scale;
    return d;
}

// ---- volume ---------------------------------------------------------------------------------------------------------------------
// pass p of a volume of `voxels` points, `chunk` per pass: its first voxel and its length
MRIRT_HD uint64_t inj_passes(int64_t voxels, int64_t chunk) { return ((uint64_t)voxels + (uint64_t)chunk - 1) / (uint64_t)chunk; }
MRIRT_HD void inj_pass_range(int64_t voxels, int64_t chunk, uint64_t p, int64_t& first, int64_t& len) {
    first = (int64_t)p * chunk;
    len = voxels - first < chunk ? voxels - first : chunk;
}
// voxel g of [H][W][D], C order -> (x, y, z)
MRIRT_HD void inj_voxel(int64_t g, uint32_t W, uint32_t D, uint32_t& x, uint32_t& y, uint32_t& z) {
    const int64_t xy = g / D;
    z = (uint32_t)(g - xy * D);
    x = (uint32_t)(xy / W);
    y = (uint32_t)(xy - (int64_t)x * W);
}

// argmax as np.argmax: the first index of the maximum, a NaN counting as the maximum
MRIRT_HD uint32_t inj_argmax(const float* z, uint32_t C) {
    uint32_t best = 0;
    for (uint32_t k = 1; k < C; ++k)
        if (!(z[best] != z[best]) && (z[k] > z[best] || z[k] != z[k])) best = k;
    return best;
}

}  // namespace mrirt
