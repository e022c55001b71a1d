// Coordinate-injection INR of notebooks/improved.ipynb (cells 6 - 10): learnable Gaussian Fourier projection, an MLP whose hidden
// layers take [h | coords | mods], dropout after every hidden ReLU, full-volume prediction, MC-dropout entropy, and the
// boundary weight map of the notebook's cache.  fp32 throughout, on v_mfma_f32_16x16x4_f32.  DESIGN.md section 23.
//   inj_features_kernel   coords (given, or generated from the voxel index) -> [sin | cos](2 pi c01 . B^T) with the STRICT
//                         sine / cosine of siren_sincos.h
//   inj_gemm_kernel       one layer: the GEMM staging of inr_gemm.h over the three-part A view of inr_inject.h; epilogues
//                         bias + ReLU, bias + ReLU + dropout (Philox word per element, no mask in memory), head
//   inj_point_kernel      per point over the logits: argmax, softmax added into the running sum, entropy of the mean
//   inj_boundary_kernel   max over classes of 1 / (1 + sqrt(d2)) on the squared-distance field of csrc/edt.hip
// No allocation, no host synchronisation, no float atomics, one writer per element: the same inputs give the same bits.
// The feature and layer launches (inj_run_features, inj_run_layers; csrc/inr_inject_host.h) take their output buffers as
// arguments: the training step of csrc/inr_inject_train.hip runs them into per-layer buffers.
#include "inr_device.h"
#include "inr_gemm.h"
#include "inr_inject_host.h"
#include "inr_inject_fused.h"
#include "edt_line.h"
#include "siren_sincos.h"

namespace mrirt {

enum { kInjRelu = 0, kInjDrop = 1, kInjHead = 2 };

struct InjFeatArgs {
    const float* B;              // [F / 2][3]
    const float* coordsIn;       // [n][3], or NULL: generated from voxel base + i of [H][W][D]
    float* coordsOut;            // generated coordinates, [n][3] (only without coordsIn)
    float* feat;                 // [n][F]
    int64_t n, base;
    uint32_t F, H, W, D;
};

// thread (i, j), j < F / 2: feat[i][j] = sin a, feat[i][F / 2 + j] = cos a
__global__ __launch_bounds__(kInjThreads) void inj_features_kernel(InjFeatArgs a) {
    const uint32_t half = a.F >> 1;
    const int64_t t = (int64_t)blockIdx.x * kInjThreads + threadIdx.x;
    if (t >= a.n * (int64_t)half) return;
    const int64_t i = t / half;
    const uint32_t j = (uint32_t)(t - i * half);
    float cx, cy, cz;
    if (a.coordsIn) {
        cx = a.coordsIn[3 * i]; cy = a.coordsIn[3 * i + 1]; cz = a.coordsIn[3 * i + 2];
    } else {
        uint32_t x, y, z;
        inj_voxel(a.base + i, a.W, a.D, x, y, z);
        cx = sample_coord(x, a.H); cy = sample_coord(y, a.W); cz = sample_coord(z, a.D);
        if (j == 0) { a.coordsOut[3 * i] = cx; a.coordsOut[3 * i + 1] = cy; a.coordsOut[3 * i + 2] = cz; }
    }
    float sn, cs;
    inj_feature(cx, cy, cz, a.B[3 * j], a.B[3 * j + 1], a.B[3 * j + 2], sn, cs);      // csrc/inr_inject_fused.h: shared with the fused forward
    a.feat[i * a.F + j] = sn;
    a.feat[i * a.F + half + j] = cs;
}

struct InjGemmArgs {
    InjView A;
    TrView B;
    uint32_t M, N;               // rows (points of this call) and columns (units of the layer)
    int64_t K;
    float* C;                    // [M][N]
    const float* bias;
    uint64_t seed, index0;       // dropout: Philox key, global index of row 0
    uint32_t ctr2, thr;          // 256 s + l;  kept iff word < thr
    float scale;
};

__device__ __forceinline__ void inj_fetch(const InjView& v, uint32_t m0, int64_t k0, int64_t K, float (&reg)[kTrBM / 16]) {
#pragma unroll
    for (int i = 0; i < kTrBM / 16; ++i) {
        uint32_t r, k;
        tr_stage_coord<kTrBM, true>(threadIdx.x, i, r, k);
        int64_t off;
        const int src = inj_view_src(v, m0 + r, k0 + k, K, off);
        reg[i] = src == 0 ? v.h.p[off] : src == 1 ? v.c.p[off] : src == 2 ? v.m.p[off] : 0.0f;
    }
}

template <int BN, int EPI>
__global__ __launch_bounds__(kTrThreads) void inj_gemm_kernel(InjGemmArgs a) {
    __shared__ float As[kTrBK * TrLds<kTrBM>::pitch];
    __shared__ float Bs[kTrBK * TrLds<BN>::pitch];
    constexpr int NT = BN / 16;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m0 = blockIdx.x * kTrBM, n0 = blockIdx.y * BN;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    float ra[kTrBM / 16], rb[BN / 16];
    inj_fetch(a.A, m0, 0, a.K, ra);
    gm_fetch<BN, false>(a.B, n0, 0, a.K, rb);
    for (int64_t k0 = 0; k0 < a.K; k0 += kTrBK) {
        __syncthreads();                                 // the previous tile's reads are done
        gm_stage<kTrBM, true>(As, ra);
        gm_stage<BN, false>(Bs, rb);
        __syncthreads();
        if (k0 + kTrBK < a.K) {                          // the next tile's loads fly under this tile's MFMAs
            inj_fetch(a.A, m0, k0 + kTrBK, a.K, ra);
            gm_fetch<BN, false>(a.B, n0, k0 + kTrBK, a.K, rb);
        }
#pragma unroll
        for (int s = 0; s < kTrBK / 4; ++s) {
            const uint32_t kk = 4u * s + (lane >> 4);
            const float av = As[kk * TrLds<kTrBM>::pitch + 16u * wave + (lane & 15u)];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float bv = Bs[kk * TrLds<BN>::pitch + 16u * j + (lane & 15u)];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const uint32_t col = n0 + 16u * j + tr_acc_col(lane);
        uint32_t word[4] = { 0u, 0u, 0u, 0u };           // the mask words of this lane's four rows (inj_mask_word of each)
        if (EPI == kInjDrop) {
            // One Philox call yields the words of units 4 g .. 4 g + 3 of a point, and the four lanes 4 g' .. 4 g' + 3 of the
            // MFMA tile hold exactly those units for the same four rows: lane q of the group draws row q's four words, and
            // four rounds of lane exchange hand every lane word (its unit & 3) of each row.  Every lane takes part.
            const uint32_t q = lane & 3u;
            const uint64_t i = a.index0 + (m0 + 16u * wave + tr_acc_row(lane, 0) + q);
            uint32_t c[4] = { (uint32_t)i, (uint32_t)(i >> 32), a.ctr2, col >> 2 };
            philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const uint32_t want = (q - t) & 3u, from = (q + t) & 3u;      // in round t lane q shows word q - t and reads row q + t
                const uint32_t send = want == 0 ? c[0] : want == 1 ? c[1] : want == 2 ? c[2] : c[3];
                const uint32_t got = (uint32_t)__shfl((int)send, (int)((lane & ~3u) | from), 64);
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r)
                    if (from == r) word[r] = got;
            }
        }
        if (col >= a.N) continue;
        const float bias = a.bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = m0 + 16u * wave + tr_acc_row(lane, r);
            if (row >= a.M) continue;
            float v = acc[j][r] + bias;
            if (EPI != kInjHead) v = !(v <= 0.0f) ? v : 0.0f;        // jnp.maximum(v, 0): -0 -> +0, a NaN stays
            if (EPI == kInjDrop) v = word[r] < a.thr ? v * a.scale : 0.0f;
            a.C[(int64_t)row * a.N + col] = v;
        }
    }
}

struct InjPointArgs {
    const float* logits;         // [n][C]
    int64_t n;
    uint32_t C;
    int16_t* argmax;             // NULL: not wanted
    float* sum;                  // NULL: no softmax job; else [n][C]: sample `first` stores, later samples add
    uint32_t first, last;
    float samples;               // (float)S
    uint32_t writeMean;          // after the last sample: sum <- mean
    float* entropy;              // after the last sample, [n]
};

__global__ __launch_bounds__(kInjThreads) void inj_point_kernel(InjPointArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kInjThreads + threadIdx.x;
    if (i >= a.n) return;
    const float* z = a.logits + i * a.C;
    if (a.argmax) a.argmax[i] = (int16_t)inj_argmax(z, a.C);
    if (!a.sum) return;
    float p[kLossMaxClasses], d[kLossMaxClasses];
    point_softmax(z, a.C, p, d);
    float* s = a.sum + i * a.C;
    float h = 0.0f;
    for (uint32_t k = 0; k < a.C; ++k) {
        const float t = a.first ? p[k] : s[k] + p[k];
        if (!a.last) { s[k] = t; continue; }
        const float m = t / a.samples;
        if (a.writeMean) s[k] = m;
        h = h + m * logf(m + 1e-10f);
    }
    if (a.last) a.entropy[i] = -h;
}

// out = (first ? v : max(out, v)) with v = float(1 / (1 + sqrt(d2))) in fp64, rounded once (the rounding is monotone: the
// maximum of the rounded values is the rounded maximum); d2 == NULL: v = 0
__global__ __launch_bounds__(kInjThreads) void inj_boundary_kernel(const double* d2, float* out, int64_t n, uint32_t first) {
    const int64_t i = (int64_t)blockIdx.x * kInjThreads + threadIdx.x;
    if (i >= n) return;
    const float v = d2 ? (float)(1.0 / (1.0 + sqrt(d2[i]))) : 0.0f;
    out[i] = first ? v : fmaxf(out[i], v);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

int inj_desc(const MrirtInjectDesc* d, InjNet& N) {
    if (!d) return MRIRT_ERR_NULL;
    if (d->numLayers < 2 || d->numLayers > kInjMaxLayers) return MRIRT_ERR_ARG;
    if (inj_check_shape(d->numLayers, d->fourierDim, d->numMods, d->width, d->coordLayers, d->modLayers) != 0) return MRIRT_ERR_ARG;
    N = inj_net(d->numLayers, d->fourierDim, d->numMods, d->width, d->coordLayers, d->modLayers);
    return MRIRT_OK;
}

// what every entry point refuses of a dropout struct; S: how many samples this call may take at most
int inj_check_dropout(const MrirtInjectDropout* p, uint32_t maxSamples) {
    if (!(p->keep > 0.0f && p->keep <= 1.0f) || !isfinite(1.0f / p->keep)) return MRIRT_ERR_ARG;
    if (p->samples < 1 || p->samples > maxSamples) return MRIRT_ERR_ARG;
    if (p->sample0 >= kInjMaxSampleIndex || p->sample0 + p->samples > kInjMaxSampleIndex) return MRIRT_ERR_ARG;
    if (p->reserved != 0) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

InjDrop inj_drop(const MrirtInjectDropout* p, uint32_t s) {
    InjDrop d = {};
    if (!p || p->keep == 1.0f) return d;                 // keep == 1 masks nothing: the evaluation forward
    d.on = true;
    d.seed = p->seed; d.index0 = p->index0; d.s = p->sample0 + s;
    d.thr = inj_threshold(p->keep);
    d.scale = 1.0f / p->keep;
    return d;
}

static uint32_t inj_blocks(int64_t items) { return (uint32_t)((items + kInjThreads - 1) / kInjThreads); }

int inj_run_features(const InjNet& N, const float* B, const float* coords, int64_t n, int64_t base, const uint32_t* hwd, float* coordsOut,
                     float* feat, hipStream_t s) {
    InjFeatArgs f = {};
    f.B = B; f.coordsIn = coords; f.coordsOut = coordsOut; f.feat = feat;
    f.n = n; f.base = base; f.F = N.F;
    if (hwd) { f.H = hwd[0]; f.W = hwd[1]; f.D = hwd[2]; }
    hipLaunchKernelGGL(inj_features_kernel, dim3(inj_blocks(n * (int64_t)(N.F / 2))), dim3(kInjThreads), 0, s, f);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

template <int EPI>
static int launch_layer(const InjGemmArgs& g, hipStream_t s) {
    const uint32_t mt = (g.M + kTrBM - 1) / kTrBM;
    if (g.N <= 16) hipLaunchKernelGGL((inj_gemm_kernel<16, EPI>), dim3(mt, 1), dim3(kTrThreads), 0, s, g);
    else hipLaunchKernelGGL((inj_gemm_kernel<64, EPI>), dim3(mt, (g.N + 63) / 64), dim3(kTrThreads), 0, s, g);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

// coords: [n][3]; mods as inj_layer_view takes them
int inj_run_layers(const InjNet& N, const float* feat, float* const* act, const float* w, const float* b, const float* coords,
                   const float* mods, int64_t modRow, int64_t modCol, int64_t n, const InjDrop& d, float* logits, hipStream_t s) {
    for (uint32_t l = 0; l < N.numLayers; ++l) {
        const bool head = l + 1 == N.numLayers;
        const float* h = l == 0 ? feat : act[l - 1];
        InjGemmArgs g = {};
        g.A = inj_layer_view(N, l, n, h, coords, mods, modRow, modCol);
        g.B = TrView{ w + N.wOff[l], 1, (int64_t)N.out[l], N.out[l], 0u };
        g.M = (uint32_t)n; g.N = N.out[l]; g.K = N.in[l];
        g.C = head ? logits : act[l];
        g.bias = b + N.bOff[l];
        g.seed = d.seed; g.index0 = d.index0; g.ctr2 = 256u * d.s + l; g.thr = d.thr; g.scale = d.scale;
        const int rc = head ? launch_layer<kInjHead>(g, s) : d.on ? launch_layer<kInjDrop>(g, s) : launch_layer<kInjRelu>(g, s);
        if (rc != MRIRT_OK) return rc;
    }
    return MRIRT_OK;
}

// the two over the inference scratch: features at offFeat, the activations in the two alternating buffers
static int run_features(const InjNet& N, const InjLayout& Y, const float* B, const float* coords, int64_t n, int64_t base,
                        const uint32_t* hwd, char* scratch, hipStream_t s) {
    return inj_run_features(N, B, coords, n, base, hwd, (float*)(scratch + Y.offCoords), (float*)(scratch + Y.offFeat), s);
}

static int run_layers(const InjNet& N, const InjLayout& Y, const float* w, const float* b, const float* coords, const float* mods,
                      int64_t modRow, int64_t modCol, int64_t n, const InjDrop& d, float* logits, char* scratch, hipStream_t s) {
    float* act[kInjMaxLayers];
    for (uint32_t l = 0; l < kInjMaxLayers; ++l) act[l] = (float*)(scratch + inj_act_offset(Y, l));
    return inj_run_layers(N, (const float*)(scratch + Y.offFeat), act, w, b, coords, mods, modRow, modCol, n, d, logits, s);
}

static int run_point(const InjPointArgs& p, hipStream_t s) {
    hipLaunchKernelGGL(inj_point_kernel, dim3(inj_blocks(p.n)), dim3(kInjThreads), 0, s, p);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

// S dropout passes over the features in the scratch -> entropy (and the mean in `sum` when writeMean)
static int run_uncertainty(const InjNet& N, const InjLayout& Y, const float* w, const float* b, const float* coords, const float* mods,
                           int64_t modRow, int64_t modCol, int64_t n, const MrirtInjectDropout* dp, uint64_t index0, float* sum,
                           uint32_t writeMean, float* entropy, char* scratch, hipStream_t s) {
    float* logits = (float*)(scratch + Y.offLogits);
    for (uint32_t k = 0; k < dp->samples; ++k) {
        InjDrop d = inj_drop(dp, k);
        d.index0 = index0;
        int rc = run_layers(N, Y, w, b, coords, mods, modRow, modCol, n, d, logits, scratch, s);
        if (rc != MRIRT_OK) return rc;
        InjPointArgs p = {};
        p.logits = logits; p.n = n; p.C = N.C; p.sum = sum;
        p.first = k == 0; p.last = k + 1 == dp->samples; p.samples = (float)dp->samples; p.writeMean = writeMean; p.entropy = entropy;
        if ((rc = run_point(p, s)) != MRIRT_OK) return rc;
    }
    return MRIRT_OK;
}

static int inj_check_points(const InjNet& N, const float* B, const float* w, const float* b, const float* coords, const float* mods, int64_t n) {
    if (!B || !w || !b || !coords || (N.M != 0 && !mods)) return MRIRT_ERR_NULL;
    if (n < 1 || n >= ((int64_t)1 << 31)) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_inject_scratch_bytes(const MrirtInjectDesc* desc, int64_t n) {
    InjNet N;
    if (inj_desc(desc, N) != MRIRT_OK || n < 1 || n >= ((int64_t)1 << 31)) return 0;
    return (int64_t)inj_layout(N, n).bytes;
}

extern "C" int mrirt_inject_forward(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                                    const float* mods, int64_t n, const MrirtInjectDropout* dropout, float* logits, int16_t* argmax,
                                    void* scratch, int64_t scratch_bytes, void* stream) {
    InjNet N;
    int rc = inj_desc(desc, N);
    if (rc != MRIRT_OK) return rc;
    if ((rc = inj_check_points(N, B, w, b, coords, mods, n)) != MRIRT_OK) return rc;
    if (!logits && !argmax) return MRIRT_ERR_NULL;
    if (dropout && ((rc = inj_check_dropout(dropout, 1)) != MRIRT_OK)) return rc;
    const InjLayout Y = inj_layout(N, n);
    if ((rc = check_scratch(scratch, scratch_bytes, Y.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    if (!logits) logits = (float*)(base + Y.offLogits);
    if ((rc = run_features(N, Y, B, coords, n, 0, nullptr, base, s)) != MRIRT_OK) return rc;
    if ((rc = run_layers(N, Y, w, b, coords, mods, (int64_t)N.M, 1, n, inj_drop(dropout, 0), logits, base, s)) != MRIRT_OK) return rc;
    if (argmax) {
        InjPointArgs p = {};
        p.logits = logits; p.n = n; p.C = N.C; p.argmax = argmax;
        if ((rc = run_point(p, s)) != MRIRT_OK) return rc;
    }
    return MRIRT_OK;
}

extern "C" int mrirt_inject_uncertainty(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                                        const float* mods, int64_t n, const MrirtInjectDropout* dropout, float* entropy,
                                        float* mean_probs, void* scratch, int64_t scratch_bytes, void* stream) {
    InjNet N;
    int rc = inj_desc(desc, N);
    if (rc != MRIRT_OK) return rc;
    if ((rc = inj_check_points(N, B, w, b, coords, mods, n)) != MRIRT_OK) return rc;
    if (!dropout || !entropy) return MRIRT_ERR_NULL;
    if ((rc = inj_check_dropout(dropout, kInjMaxSamples)) != MRIRT_OK) return rc;
    const InjLayout Y = inj_layout(N, n);
    if ((rc = check_scratch(scratch, scratch_bytes, Y.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    if ((rc = run_features(N, Y, B, coords, n, 0, nullptr, base, s)) != MRIRT_OK) return rc;
    float* sum = mean_probs ? mean_probs : (float*)(base + Y.offMean);
    return run_uncertainty(N, Y, w, b, coords, mods, (int64_t)N.M, 1, n, dropout, dropout->index0, sum, mean_probs ? 1u : 0u, entropy, base, s);
}

extern "C" int mrirt_inject_predict_volume(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* mods,
                                           const uint32_t hwd[3], int64_t chunk, const MrirtInjectDropout* dropout, int16_t* pred,
                                           float* entropy, void* scratch, int64_t scratch_bytes, void* stream) {
    InjNet N;
    int rc = inj_desc(desc, N);
    if (rc != MRIRT_OK) return rc;
    if (!B || !w || !b || (N.M != 0 && !mods) || !hwd || !pred) return MRIRT_ERR_NULL;
    if (entropy && !dropout) return MRIRT_ERR_NULL;
    if (dropout && !entropy) return MRIRT_ERR_ARG;
    uint64_t vox = 1;
    for (int k = 0; k < 3; ++k) {
        if (hwd[k] < 2) return MRIRT_ERR_ARG;
        vox *= hwd[k];
        if (vox >= (1ull << 31)) return MRIRT_ERR_ARG;
    }
    if (chunk < 1 || chunk >= ((int64_t)1 << 31)) return MRIRT_ERR_ARG;
    if (dropout && ((rc = inj_check_dropout(dropout, kInjMaxSamples)) != MRIRT_OK)) return rc;
    if (dropout && dropout->index0 != 0) return MRIRT_ERR_ARG;       // a volume's global index is the voxel index
    const InjLayout Y = inj_layout(N, chunk);
    if ((rc = check_scratch(scratch, scratch_bytes, Y.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    const float* coords = (const float*)(base + Y.offCoords);
    float* logits = (float*)(base + Y.offLogits);
    const uint64_t passes = inj_passes((int64_t)vox, chunk);
    for (uint64_t p = 0; p < passes; ++p) {
        int64_t first, len;
        inj_pass_range((int64_t)vox, chunk, p, first, len);
        const float* m = mods ? mods + first : nullptr;
        if ((rc = run_features(N, Y, B, nullptr, len, first, hwd, base, s)) != MRIRT_OK) return rc;
        if ((rc = run_layers(N, Y, w, b, coords, m, 1, (int64_t)vox, len, InjDrop{}, logits, base, s)) != MRIRT_OK) return rc;
        InjPointArgs a = {};
        a.logits = logits; a.n = len; a.C = N.C; a.argmax = pred + first;
        if ((rc = run_point(a, s)) != MRIRT_OK) return rc;
        if (entropy) {
            rc = run_uncertainty(N, Y, w, b, coords, m, 1, (int64_t)vox, len, dropout, (uint64_t)first, (float*)(base + Y.offMean), 0u,
                                 entropy + first, base, s);
            if (rc != MRIRT_OK) return rc;
        }
    }
    return MRIRT_OK;
}

extern "C" int64_t mrirt_boundary_weights_scratch_bytes(const uint32_t hwd[3]) {
    if (!hwd || edt_check_volume(hwd, nullptr) != 0) return 0;
    return (int64_t)tr_align((uint64_t)hwd[0] * hwd[1] * hwd[2] * sizeof(double)) + (int64_t)tr_align(kEdtSquaredScratch);
}

extern "C" int mrirt_boundary_weights(const int16_t* labels, const uint32_t hwd[3], uint32_t num_classes, float* out, void* scratch,
                                      int64_t scratch_bytes, void* stream) {
    if (!labels || !hwd || !out) return MRIRT_ERR_NULL;
    if (edt_check_volume(hwd, nullptr) != 0) return MRIRT_ERR_ARG;
    if (num_classes < 1 || num_classes > kEdtMaxClasses) return MRIRT_ERR_ARG;
    const int64_t vox = (int64_t)hwd[0] * hwd[1] * hwd[2];
    const uint64_t fieldBytes = tr_align((uint64_t)vox * sizeof(double));
    int rc = check_scratch(scratch, scratch_bytes, fieldBytes + tr_align(kEdtSquaredScratch));
    if (rc != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* field = (double*)scratch;
    const float one[3] = { 1.0f, 1.0f, 1.0f };
    if (num_classes == 1) {
        hipLaunchKernelGGL(inj_boundary_kernel, dim3(inj_blocks(vox)), dim3(kInjThreads), 0, s, (const double*)nullptr, out, vox, 1u);
        MRIRT_HIP(hipGetLastError());
    }
    for (uint32_t c = 1; c < num_classes; ++c) {
        // a class that is absent leaves d2 = +inf everywhere: 1 / (1 + inf) = 0, the map's floor
        rc = mrirt_edt_squared(labels, hwd, (int32_t)c, one, field, (char*)scratch + fieldBytes, (int64_t)tr_align(kEdtSquaredScratch), stream);
        if (rc != MRIRT_OK) return rc;
        hipLaunchKernelGGL(inj_boundary_kernel, dim3(inj_blocks(vox)), dim3(kInjThreads), 0, s, (const double*)field, out, vox, c == 1 ? 1u : 0u);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}
