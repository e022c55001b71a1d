// INR forward on the CDNA4 matrix cores — replaces the per-voxel MLP evaluation of the reference
// (inr/inr/model.py:11-50 build_input + apply_mlp, :119-141 predict_volume; SIREN forward of
// notebooks/neumors_inr.ipynb:1165-1178), which the viewer runs as a prepass over every voxel
// (inr/viewer/brats_viewer.py:250-310).
//
// Formulation: every layer is computed TRANSPOSED,  Y^T[out, points] = W^T[out, in] . H^T[in, points],
// with v_mfma_f32_32x32x16_bf16.  The 32x32 accumulator tile then has the point on the lane and the
// output feature in the registers — exactly the B-operand shape of the next layer (k = feature), so
// activations go  accumulator -> bias + activation -> bf16 pack -> next MFMA  without leaving the
// register file (guide: "an accumulator tile as the next MFMA's operand").  The k order inside a
// 16-deep step is permuted by that reuse (element j of lane half h is feature 16s + 8(j>>2) + 4h + (j&3));
// the weights are pre-packed in the same permuted order (mrirt_inr_pack_weights), one 1-KiB fragment
// per (out tile, k step): an A fragment is one 16-byte read per lane.
//
// Precision: bf16 operands, fp32 accumulate.  A SIREN's FIRST layer scales its inputs by w0 = 30 before a
// sine, so its inputs and weights are split hi + lo in bf16 and three products are accumulated
// (hi*hi + hi*lo + lo*hi: ~16 mantissa bits).  A ReLU net's first layer (coordinates, sin(pi k c) features,
// z-scored intensities) and every hidden layer use plain bf16.
//
// This file is the host side and the ABI: the packed-image layout and the pack kernel, the dispatch between the kernels,
// calibration and the mrirt_inr_* entry points.  The kernels and their launchers: inr_stream.hip (every network),
// inr_ws.hip (the 4 x 256 SIREN, weights stationary in registers), inr_refine.hip (near-tie refinement in split bf16);
// what they share: inr_fwd.h.
#include <stdlib.h>

#include "inr_fwd.h"

namespace mrirt {

// Packed image, in fragment units:  layer 0 of a SIREN: [o][t][s][hi,lo]   every other layer: [o][t][s]
// Augmented split (a SIREN with <= 8 inputs, i.e. the 7-input net of the notebook): the three products
// x_hi W_hi + x_lo W_hi + x_hi W_lo are folded into the k axis of ONE 32-deep tile — k step 0 carries
// [x_hi | x_lo] against [W_hi ; W_hi], k step 1 carries [x_hi] against [W_lo] — two MFMAs per out tile
// instead of six.
static int make_layout(const MrirtInrDesc* d, InrLayout& L) {
    if (!d) return MRIRT_ERR_NULL;
    if (d->numLayers < 2 || d->numLayers > kMaxLayers || d->outDim < 1 || d->outDim > 16) return MRIRT_ERR_ARG;
    if (d->hidden != 32 && d->hidden != 64 && d->hidden != 128 && d->hidden != 256) return MRIRT_ERR_ARG;
    if (d->inDim < 1 || d->inDim > 128 || d->kind > 3) return MRIRT_ERR_ARG;
    if (d->kind == MRIRT_INR_FOURIER_RELU && d->inDim != 3 + 6 * d->fourierFreqs + d->numMods) return MRIRT_ERR_ARG;
    if (d->kind == MRIRT_INR_SIREN && d->inDim != 3 + d->numMods) return MRIRT_ERR_ARG;
    if (d->kind < 2 && d->numMods > (uint32_t)kMaxMods) return MRIRT_ERR_ARG;    // raw inputs are staged 12 floats per point
    L.numLayers = d->numLayers; L.hidden = d->hidden; L.inDim = d->inDim; L.outDim = d->outDim;
    L.kt0 = d->inDim <= 32 ? 1 : 4;                      // 33..128 inputs: zero-padded to 128 (layer 0 only)
    uint32_t frag = 0, bias = 0, w = 0;
    for (uint32_t l = 0; l < d->numLayers; ++l) {
        L.in[l] = l == 0 ? d->inDim : d->hidden;
        L.out[l] = l + 1 == d->numLayers ? d->outDim : d->hidden;
        const uint32_t kt = l == 0 ? L.kt0 : d->hidden / 32, ot = (L.out[l] + 31) / 32;
        L.fragOff[l] = frag; L.biasOff[l] = bias; L.wOff[l] = w;
        const bool sirenNet = d->kind == MRIRT_INR_SIREN || d->kind == 3u, head = l + 1 == d->numLayers;
        L.scale[l] = (!sirenNet || head) ? 1.0f : (float)((l == 0 ? (double)d->w0 : 1.0) / 6.283185307179586);
        L.bscale[l] = (!sirenNet || head) ? 1.0f : (float)(1.0 / 6.283185307179586);     // sin(w0 (xW) + b): b is not scaled by w0
        const bool aug = d->kind == MRIRT_INR_SIREN && d->inDim <= 8;
        frag += ot * kt * 2 * ((l == 0 && sirenNet && !aug) ? 2 : 1);     // split layer 0: hi and lo fragments side by side
        bias += ot * 32;
        w += L.in[l] * L.out[l];
    }
    L.totalFrags = frag;
    L.aug0 = (d->kind == MRIRT_INR_SIREN && d->inDim <= 8) ? 1u : 0u;
    L.split0 = ((d->kind == MRIRT_INR_SIREN || d->kind == 3u) && !L.aug0) ? 1u : 0u;
    uint32_t rf = 0;
    for (uint32_t l = 0; l < d->numLayers; ++l) {
        const uint32_t kt = l == 0 ? L.kt0 : d->hidden / 32, ot = (L.out[l] + 31) / 32;
        L.refFragOff[l] = rf;
        rf += ot * kt * 2 * ((l == 0 && L.aug0) ? 1 : 2);
    }
    L.refTotalFrags = rf;
    return MRIRT_OK;
}

// fp32 [in][out] row-major -> permuted bf16 fragments (see file header).  One thread per (fragment, lane) of one image:
// the main image (REF = false), or the refine image (REF = true) — same permuted k order and the same folded scale, but
// every layer split: fragment 2q holds the bf16 "hi" parts and 2q + 1 the "lo" parts (w - hi, rounded to bf16) of k step q.
template <bool REF>
__global__ __launch_bounds__(256) void inr_pack_kernel(const float* __restrict__ w, uint4* __restrict__ packed, InrLayout L) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t frag = gid >> 6, lane = gid & 63u;
    const uint32_t* fragOff = REF ? L.refFragOff : L.fragOff;
    if (frag >= (REF ? L.refTotalFrags : L.totalFrags)) return;
    uint32_t l = 0;
    while (l + 1 < L.numLayers && frag >= fragOff[l + 1]) ++l;
    const uint32_t kt = l == 0 ? L.kt0 : L.hidden / 32;
    uint32_t f = frag - fragOff[l];
    const bool aug = l == 0 && L.aug0;
    bool lo = false;
    if (REF ? !aug : (l == 0 && L.split0)) { lo = (f & 1u) != 0; f >>= 1; }    // this layer carries hi and lo fragments side by side
    const uint32_t s = f & 1u, t = (f >> 1) % kt, o = (f >> 1) / kt;
    const uint32_t r = lane & 31u, h = lane >> 5;
    uint16_t e[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        uint32_t k = 32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3u);
        const uint32_t oc = 32 * o + r;
        bool part_lo = lo;
        if (aug) {                                       // k step 0: [W_hi ; W_hi], k step 1: [W_lo]
            const uint32_t kk = k & 15u, in = L.in[0];
            part_lo = s == 1;
            k = s == 0 ? (kk < in ? kk : (kk < 2 * in ? kk - in : 0xffffu)) : (kk < in ? kk : 0xffffu);
        }
        const float v = (k < L.in[l] && oc < L.out[l]) ? w[L.wOff[l] + k * L.out[l] + oc] * L.scale[l] : 0.0f;
        const uint16_t hi = bf16_bits(v);
        const float hif = __builtin_bit_cast(float, (uint32_t)hi << 16);
        e[j] = part_lo ? bf16_bits(v - hif) : hi;
    }
    uint4 q;
    q.x = e[0] | ((uint32_t)e[1] << 16); q.y = e[2] | ((uint32_t)e[3] << 16);
    q.z = e[4] | ((uint32_t)e[5] << 16); q.w = e[6] | ((uint32_t)e[7] << 16);
    packed[(size_t)frag * 64 + lane] = q;
}

// Near-tie refinement.  bf16 hidden layers leave each logit with an error of a few 1e-3 of the logit
// range; where the two largest logits are closer than that, the argmax can differ from the fp32 reference's
// (0.3-0.5 % of the points of a random 4-class head).  The forward kernels therefore mark every point whose top-2 gap is
// below  tieScale x (rms logit error of this network's bf16 pass, measured once at pack time: tail[0])  by setting
// kFlagBit in the class they store, and inr_refine_kernel re-evaluates exactly those points with split-bf16 operands
// (hi + lo, three products, ~16 mantissa bits) in EVERY layer and stores the clean class.  The mark depends on the
// point's own logits only, so results stay independent of batch position.
constexpr float kTieSigmas = 3.0f;        // mark below this many standard deviations of the gap's error (MRIRT_INR_TIE_SIGMAS overrides)
constexpr int kCalPoints = 8192;          // calibration points (pack time)

static int launch_inr_main(const InrArgs& a, hipStream_t s) {
    if (ws_eligible(a) && !(a.flags & MRIRT_INR_NO_WEIGHT_STATIONARY) && !debug_env("MRIRT_INR_NO_WS")) return launch_inr_ws(a, s);
    return launch_inr_stream(a, s);
}

// near-tie marking + refinement can be switched off for A/B measurements (MrirtInrDesc.flags; the classes are then the bf16 pass's)
static int launch_inr(InrArgs a, hipStream_t s) {
    if (a.n <= 0) return MRIRT_OK;
    if (a.refineAll) return launch_refine(a, s);
    const bool off = (a.flags & MRIRT_INR_NO_REFINE) != 0 || debug_env("MRIRT_INR_NO_REFINE");
    const bool mark = a.argmax != nullptr && a.tie != nullptr && !off;
    if (!mark) a.tie = nullptr;
    else {
        float sig = a.tieSigmas > 0.0f ? a.tieSigmas : kTieSigmas;
#ifdef MRIRT_DEBUG_ENV
        if (const char* e = getenv("MRIRT_INR_TIE_SIGMAS")) { const float v = (float)atof(e); if (v > 0.0f) sig = v; }
#endif
        a.tieScale = sig * 1.41421356f;                  // the gap of two logits carries two errors
    }
    int rc = launch_inr_main(a, s);
    if (rc != MRIRT_OK || !mark || (a.flags & MRIRT_INR_MARK_ONLY) != 0) return rc;
    return launch_refine(a, s);
}

static int fill_args(const MrirtInrDesc* d, InrArgs& a) {
    int rc = make_layout(d, a.L);
    if (rc != MRIRT_OK) return rc;
    if (!d->weights || !d->biases) return MRIRT_ERR_NULL;
    a.kind = d->kind; a.K = d->fourierFreqs; a.M = d->numMods; a.w0 = d->w0;
    a.wpack = static_cast<const uint4*>(d->weights);
    a.bias = d->biases;
    a.coords = nullptr; a.feats = nullptr; a.n = 0; a.nDev = nullptr; a.volume = 0; a.H = a.W = a.D = 1;
    a.logits = nullptr; a.argmax = nullptr;
    a.tie = reinterpret_cast<const float*>(a.wpack + (size_t)tail_frag(a.L) * 64);     // written by mrirt_inr_pack_weights
    a.tieScale = 0.0f; a.refineAll = 0; a.segTicket = nullptr;
    a.flags = d->flags; a.tieSigmas = d->tieSigmas;
    return MRIRT_OK;
}

// Internal (brats_host.h): the forward pass with the point count read from device memory — used by the
// chunked C5 render (brats_c5.hip), whose producer kernel sizes each chunk's batch on the device.
int inr_forward_dev_n(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t nMax,
                      const uint32_t* nDev, int16_t* argmax, uint32_t* segTicket, hipStream_t s) {
    InrArgs a;
    int rc = fill_args(desc, a);
    if (rc != MRIRT_OK) return rc;
    if (desc->kind >= 2 || !coords || !feats || !argmax || !nDev) return MRIRT_ERR_ARG;
    a.coords = coords; a.feats = feats; a.n = nMax; a.nDev = nDev; a.argmax = argmax; a.segTicket = segTicket;
    return launch_inr(a, s);
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_inr_pack_bytes(const MrirtInrDesc* desc) {
    InrLayout L;
    if (make_layout(desc, L) != MRIRT_OK) return 0;
    // main image + slack (the last chunk's DMA over-fetch, never used) + refine image + calibration record
    return (int64_t)(tail_frag(L) + 1) * 1024;
}

namespace mrirt {

__device__ __forceinline__ uint32_t cal_hash(uint32_t x) {         // lowbias32
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float cal_uniform(uint32_t i) { return (float)(cal_hash(i) >> 8) * (1.0f / 16777216.0f); }

// calibration inputs: coords ~ U(-1, 1); modalities ~ the sum of four uniforms, centred and scaled to unit variance
// (z-scored intensities, brats_viewer.py:281-287); raw-x kinds: every input ~ U(-1, 1)
__global__ void inr_cal_inputs_kernel(float* __restrict__ coords, float* __restrict__ feats, uint32_t n, uint32_t featW, uint32_t raw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (uint32_t k = 0; k < 3; ++k) coords[i * 3 + k] = 2.0f * cal_uniform(i * 131u + k) - 1.0f;
    for (uint32_t k = 0; k < featW; ++k) {
        const uint32_t sd = 0x9e3779b9u + (i * 257u + k) * 4u;
        feats[(size_t)i * featW + k] = raw ? 2.0f * cal_uniform(sd) - 1.0f
                                           : (cal_uniform(sd) + cal_uniform(sd + 1) + cal_uniform(sd + 2) + cal_uniform(sd + 3) - 2.0f) * 1.7320508f;
    }
}

// tail[0] = rms over points and classes of (bf16 pass - split-bf16 pass), [1] = max |logit|, [2] = max |difference|, [3] = points
__global__ __launch_bounds__(256) void inr_cal_reduce_kernel(const float* __restrict__ la, const float* __restrict__ lb, uint32_t count,
                                                             float points, float* __restrict__ tail) {
    __shared__ double ssq[256];
    __shared__ float smx[256], sme[256];
    double q = 0.0;
    float mx = 0.0f, me = 0.0f;
    for (uint32_t i = threadIdx.x; i < count; i += 256) {
        const float d = la[i] - lb[i];
        q += (double)d * (double)d;
        mx = fmaxf(mx, fabsf(lb[i]));
        me = fmaxf(me, fabsf(d));
    }
    ssq[threadIdx.x] = q; smx[threadIdx.x] = mx; sme[threadIdx.x] = me;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ssq[threadIdx.x] += ssq[threadIdx.x + o];
            smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
            sme[threadIdx.x] = fmaxf(sme[threadIdx.x], sme[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tail[0] = (float)sqrt(ssq[0] / (double)count);
        tail[1] = smx[0]; tail[2] = sme[0]; tail[3] = points;
    }
}

// Measures, once per packed network, the error scale of its bf16 pass: kCalPoints pseudo-random inputs through the
// forward kernel and through the split-bf16 kernel, rms difference of the logits -> the calibration record.
static int calibrate(const MrirtInrDesc* d, hipStream_t s) {
    InrArgs a;
    int rc = fill_args(d, a);
    if (rc != MRIRT_OK) return rc;
    const bool raw = d->kind >= 2;
    const uint32_t featW = raw ? d->inDim : (d->numMods > 0 ? d->numMods : 1u), n = kCalPoints;
    const size_t fl = (size_t)n * (3 + featW + 2 * d->outDim);
    float* buf = nullptr;
    MRIRT_HIP(hipMalloc(reinterpret_cast<void**>(&buf), fl * sizeof(float)));
    float* coords = buf; float* feats = coords + (size_t)n * 3; float* la = feats + (size_t)n * featW; float* lb = la + (size_t)n * d->outDim;
    hipLaunchKernelGGL(inr_cal_inputs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, coords, feats, n, featW, raw ? 1u : 0u);
    if (raw) a.M = d->inDim;
    a.coords = raw ? nullptr : coords; a.feats = feats; a.n = n;
    a.logits = la; a.tie = nullptr;
    rc = launch_inr_main(a, s);                          // the bf16 pass (logits only)
    if (rc == MRIRT_OK) { a.logits = lb; a.refineAll = 1; rc = launch_refine(a, s); }
    if (rc == MRIRT_OK) {
        float* tail = const_cast<float*>(reinterpret_cast<const float*>(a.wpack + (size_t)tail_frag(a.L) * 64));
        hipLaunchKernelGGL(inr_cal_reduce_kernel, dim3(1), dim3(256), 0, s, la, lb, n * d->outDim, (float)n, tail);
        if (hipGetLastError() != hipSuccess) rc = MRIRT_ERR_LAUNCH;
    }
    const hipError_t e = hipStreamSynchronize(s);        // load time: the scratch is freed before returning
    (void)hipFree(buf);
    if (e != hipSuccess) return hip_fail(e);
    return rc;
}

}  // namespace mrirt

extern "C" int mrirt_inr_pack_weights(const MrirtInrDesc* desc, const float* w_f32, void* packed, void* stream) {
    InrLayout L;
    int rc = make_layout(desc, L);
    if (rc != MRIRT_OK) return rc;
    if (!w_f32 || !packed) return MRIRT_ERR_NULL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t threads = L.totalFrags * 64;
    hipLaunchKernelGGL(inr_pack_kernel<false>, dim3((threads + 255) / 256), dim3(256), 0, s, w_f32, static_cast<uint4*>(packed), L);
    MRIRT_HIP(hipGetLastError());
    uint4* ref = static_cast<uint4*>(packed) + (size_t)ref_base_frag(L) * 64;
    hipLaunchKernelGGL(inr_pack_kernel<true>, dim3((L.refTotalFrags * 64 + 255) / 256), dim3(256), 0, s, w_f32, ref, L);
    MRIRT_HIP(hipGetLastError());
    // the slack after the refine image (DMA'd into ring slots nobody reads) and the calibration record: zero (= nothing is
    // marked) until the biases are known
    MRIRT_HIP(hipMemsetAsync(ref + (size_t)L.refTotalFrags * 64, 0, ((size_t)kRefSlackFrags + 1) * 1024, s));
    if (desc->weights == packed && desc->biases != nullptr) return calibrate(desc, s);
    return MRIRT_OK;
}

extern "C" int mrirt_inr_calibrate(const MrirtInrDesc* desc, void* stream) {
    if (!desc || !desc->weights || !desc->biases) return MRIRT_ERR_NULL;
    return calibrate(desc, static_cast<hipStream_t>(stream));
}

// mrirt_inr_forward (refineAll = 0) and mrirt_inr_forward_refined (1: every point through the split-bf16 kernel)
static int forward_points(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t n,
                          float* logits, int16_t* argmax, uint32_t refineAll, void* stream) {
    InrArgs a;
    int rc = fill_args(desc, a);
    if (rc != MRIRT_OK) return rc;
    if (n < 0) return MRIRT_ERR_ARG;
    const bool needCoords = desc->kind < 2, needFeats = desc->kind >= 2 || desc->numMods > 0;
    if ((needCoords && !coords) || (needFeats && !feats)) return MRIRT_ERR_NULL;
    if (!logits && !argmax) return MRIRT_ERR_NULL;
    if (desc->kind >= 2) a.M = desc->inDim;              // raw-x kinds: feats IS the input matrix [n][inDim]
    a.coords = desc->kind < 2 ? coords : nullptr;
    a.feats = feats; a.n = n; a.logits = logits; a.argmax = argmax; a.refineAll = refineAll;
    return launch_inr(a, static_cast<hipStream_t>(stream));
}

extern "C" int mrirt_inr_forward_refined(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t n,
                                         float* logits, int16_t* argmax, void* stream) {
    return forward_points(desc, coords, feats, n, logits, argmax, 1u, stream);
}

extern "C" int mrirt_inr_forward(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t n,
                                 float* logits, int16_t* argmax, void* stream) {
    return forward_points(desc, coords, feats, n, logits, argmax, 0u, stream);
}

extern "C" int mrirt_inr_predict_volume(const MrirtInrDesc* desc, const float* mods, const uint32_t hwd[3],
                                        int16_t* pred, void* stream) {
    InrArgs a;
    int rc = fill_args(desc, a);
    if (rc != MRIRT_OK) return rc;
    if (!mods || !hwd || !pred) return MRIRT_ERR_NULL;
    if (desc->kind != MRIRT_INR_FOURIER_RELU && desc->kind != MRIRT_INR_SIREN) return MRIRT_ERR_ARG;
    for (int k = 0; k < 3; ++k) if (hwd[k] < 2) return MRIRT_ERR_DIMS;
    a.feats = mods; a.volume = 1; a.H = hwd[0]; a.W = hwd[1]; a.D = hwd[2];
    a.n = (int64_t)hwd[0] * hwd[1] * hwd[2];
    a.argmax = pred;
    return launch_inr(a, static_cast<hipStream_t>(stream));
}
