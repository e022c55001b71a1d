// What the INR forward's translation units share: the packed-image layout and the launch arguments (inr_mlp.hip fills
// them), the device code that the three kernels have in common, and the kernels' launchers (inr_stream.hip, inr_ws.hip,
// inr_refine.hip).  The formulation and the precision notes are in inr_mlp.hip's header.
#pragma once
#include "mrirt_host.h"

namespace mrirt {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int N> struct IC { static constexpr int value = N; };   // compile-time int as a lambda argument

constexpr int kInrWaves = 8;      // waves per workgroup
constexpr int kMaxLayers = 8;
constexpr int kPackSlackFrags = 64;   // one full chunk
constexpr int kRefSlackFrags = 32;    // after the refine image: inr_refine_kernel's tile DMAs always move a full ring slot
constexpr int kRawStride = 12;        // floats per point in the LDS copy of the raw inputs: c0..c2, m0..m7, 0
constexpr int kMaxMods = 8;
constexpr int kFlagBit = 0x4000;      // near-tie mark in a stored class (see inr_mlp.hip): classes are < 16, bit 14 of the int16 is free

struct InrLayout {
    uint32_t numLayers, hidden, inDim, outDim, kt0;      // kt0: 32-wide k tiles of layer 0
    uint32_t in[kMaxLayers], out[kMaxLayers];            // true widths
    uint32_t fragOff[kMaxLayers];                        // first fragment (1 KiB units) of each layer's image
    uint32_t biasOff[kMaxLayers];                        // offset into the padded bias array
    uint32_t wOff[kMaxLayers];                           // offset into the unpadded fp32 weight array
    uint32_t totalFrags;
    uint32_t split0;                                     // layer 0 carries hi + lo fragments (SIREN kinds)
    uint32_t aug0;                                       // ... or, for <= 8 inputs, the split lives in the k axis (make_layout)
    // Folded into the packed weights and the LDS copy of the biases, so that the activation is one
    // instruction on the accumulator: SIREN layers are sin(2 pi . rev) with v_sin_f32 taking revolutions,
    // hence scale = w0 / 2 pi (layer 0), 1 / 2 pi (hidden), 1 (head); ReLU nets: 1 everywhere.
    float scale[kMaxLayers];
    float bscale[kMaxLayers];                            // the biases' share of it: 1 / 2 pi without the w0
    // The REFINE image (near-tie refinement, inr_refine_kernel): every layer as split bf16, fragments
    // [out tile][k step][hi, lo] (the augmented layer 0 keeps its k-folded form [out tile][k step]); it follows
    // the image above and its slack.  refFragOff is relative to the refine image's first fragment.
    uint32_t refFragOff[kMaxLayers];
    uint32_t refTotalFrags;
};
// one more fragment after the refine image: the calibration record (tail[0] = rms logit error of the bf16 pass)

// first fragment of the refine image / of the calibration record inside the packed buffer
__host__ __device__ __forceinline__ uint32_t ref_base_frag(const InrLayout& L) { return L.totalFrags + (uint32_t)kPackSlackFrags; }
static inline uint32_t tail_frag(const InrLayout& L) { return ref_base_frag(L) + L.refTotalFrags + (uint32_t)kRefSlackFrags; }

__device__ __forceinline__ uint16_t bf16_bits(float x) {     // round-to-nearest-even, NaN preserved by the cast
    return __builtin_bit_cast(uint16_t, (__bf16)x);
}

struct InrArgs {
    InrLayout L;
    uint32_t kind, K, M;
    float w0;
    const uint4* wpack;
    const float* bias;
    const float* coords;       // [n][3] or nullptr (volume mode / raw-x kinds)
    const float* feats;        // [n][M]  (points mode)  or mods[M][H*W*D] (volume mode)
    int64_t n;
    const uint32_t* nDev;      // optional: the point count lives on the device (<= n); lets a producer kernel size the batch
    uint32_t volume;           // 1: points are the voxels of an H x W x D grid in ij order
    uint32_t H, W, D;
    float* logits;
    int16_t* argmax;
    const float* tie;          // calibration record of the packed net (tail[0] = rms logit error); nullptr: no marking
    float tieScale;            // mark when (best - second) < tieScale * tie[0]
    uint32_t refineAll;        // inr_refine_kernel: every point, not only the marked ones (calibration, mrirt_inr_forward_refined)
    uint32_t* segTicket;       // inr_refine_kernel: optional zeroed device word — the 2048-point segments after each workgroup's first are
                               // dealt on demand instead of round-robin (the config-5 passes: a few batches per workgroup, where the
                               // spread of the mark counts costs a whole batch time)
    uint32_t flags;            // MrirtInrFlags of the descriptor (read by the launchers only)
    float tieSigmas;           // the descriptor's; 0 = kTieSigmas
};

// top-2 tracking for the near-tie mark: v joins (best, second); strict > keeps the first maximum (np.argmax)
__device__ __forceinline__ void top2_push(float v, uint32_t cls, float& best, float& second, uint32_t& bestc) {
    const bool take = v > best;
    second = take ? best : fmaxf(second, v);
    best = take ? v : best;
    bestc = take ? cls : bestc;
}

// point count: a launch argument, or (C5's chunked render) a device word written by the producer kernel
__device__ __forceinline__ int64_t inr_point_count(const InrArgs& a) {
    int64_t nPts = a.n;
    if (a.nDev != nullptr) { const int64_t nd = (int64_t)*a.nDev; nPts = nd < nPts ? nd : nPts; }
    return nPts;
}

// biases: global -> LDS once per workgroup, scaled like the packed weights (InrLayout::bscale: the fold minus layer 0's w0),
// so the batch loop's only vector-memory traffic is the weight stream
__device__ __forceinline__ void inr_stage_biases(const InrArgs& a, uint4* dst) {
    const uint32_t nq = (a.L.biasOff[a.L.numLayers - 1] + 32) / 4;
    for (uint32_t i = threadIdx.x; i < nq; i += blockDim.x) {
        uint32_t l = 0;
        while (l + 1 < a.L.numLayers && 4 * i >= a.L.biasOff[l + 1]) ++l;
        float4 b = reinterpret_cast<const float4*>(a.bias)[i];
        const float sc = a.L.bscale[l];
        b.x *= sc; b.y *= sc; b.z *= sc; b.w *= sc;
        dst[i] = __builtin_bit_cast(uint4, b);
    }
}

// Feature table (inr/inr/model.py:11-23 order: coords, per axis [sin k=1..K, cos k=1..K], modalities):
// feature f of a point is  trig == 1 ? sin(2 pi (raw[src] * mult + phase)) : raw[src]  (trig == 2: the bf16
// remainder raw[src] - bf16(raw[src]) of the augmented split)  with raw = (c0,c1,c2,
// m0..m7, 0).  sin(pi k c) / cos(pi k c) go through v_sin_f32, which takes revolutions: mult = k/2
// (|.| <= 8 at K = 16), phase 0 / 0.25; its ~1e-6 absolute error is far below the split-bf16
// resolution of the layer-0 operands.  Returns the entry of slot f: (mult, phase, src, trig).
template <bool AUG>
__device__ __forceinline__ float4 inr_feature_entry(const InrArgs& a, uint32_t f) {
    uint32_t src = kRawStride - 1, trig = 0;
    float mult = 0.0f, phase = 0.0f;
    if (f < 3) src = f;
    else if (f < a.L.inDim) {
        uint32_t g = f - 3;
        if (a.kind == MRIRT_INR_FOURIER_RELU && g < 6 * a.K) {
            const uint32_t axis = g / (2 * a.K), rem = g % (2 * a.K);
            const bool isSin = rem < a.K;
            src = axis; trig = 1;
            mult = (float)((isSin ? rem : rem - a.K) + 1) * 0.5f;
            phase = isSin ? 0.0f : 0.25f;
        } else {
            if (a.kind == MRIRT_INR_FOURIER_RELU) g -= 6 * a.K;
            src = 3 + g;
        }
    }
    if constexpr (AUG) {                             // slot f = 16 s + kk:  s = 0: [x_hi | x_lo],  s = 1: [x_hi]
        const uint32_t kk = f & 15u, in = a.L.inDim;
        src = kRawStride - 1; trig = 0;
        if (f < 16) { if (kk < in) src = kk; else if (kk < 2 * in) { src = kk - in; trig = 2; } }
        else if (f < 32 && kk < in) src = kk;
    }
    return make_float4(mult, phase, __builtin_bit_cast(float, src), __builtin_bit_cast(float, trig));
}

// The <KT0, SIREN, AUG> combination a network runs with, for the two kernel families that are templated on it:
// pick(IC<KT0>, IC<SIREN>, IC<AUG>) returns the family's kernel for the caller's HID (and RES).
typedef void (*InrKernel)(const InrArgs);
template <class Pick>
static inline InrKernel inr_select_kernel(const InrArgs& a, Pick pick) {
    const bool siren = a.kind == MRIRT_INR_SIREN || a.kind == 3u;
    if (a.L.kt0 == 1) {
        if (!siren) return pick(IC<1>{}, IC<0>{}, IC<0>{});
        return a.L.aug0 ? pick(IC<1>{}, IC<1>{}, IC<1>{}) : pick(IC<1>{}, IC<1>{}, IC<0>{});
    }
    return siren ? pick(IC<4>{}, IC<1>{}, IC<0>{}) : pick(IC<4>{}, IC<0>{}, IC<0>{});
}

// inr_stream.hip: the streaming kernel, every network the layout accepts
int launch_inr_stream(const InrArgs& a, hipStream_t s);
// inr_ws.hip: the weight-stationary kernel and the networks it takes
bool ws_eligible(const InrArgs& a);
int launch_inr_ws(const InrArgs& a, hipStream_t s);
// inr_refine.hip: the split-bf16 pass over the marked points of a.argmax (or over every point: a.refineAll)
int launch_refine(const InrArgs& a, hipStream_t s);

}  // namespace mrirt
