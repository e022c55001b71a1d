// INR training step: fp32 forward, the reference's loss (inr/inr/model.py:57-90) and the gradients to the weights and biases
// of a ReLU MLP, on the exact fp32-input MFMA of gfx950 (v_mfma_f32_16x16x4_f32).  The bf16 inference kernels
// (csrc/inr_mlp.hip) and their packed images are not involved: the operands here are the fp32 master weights, row-major
// [in][out] per layer.
//
// A step is a pipeline of launches, one layer at a time:
//   forward   inputs x (Fourier features as the inference path builds them) -> per layer H . W + b, ReLU -> saved h_l
//   loss      per-point softmax / CE and per-block fp64 class sums -> totals, loss, aux -> dlogits
//   backward  per layer: H^T . dZ over split-n slabs (db as the row of ones) -> fixed-order slab sum; dZ . W^T, masked
// The three products are one LDS-tiled GEMM template; its index arithmetic lives in inr_train.h, its staging in inr_gemm.h,
// the wave sum and the softmax it shares with the other training kernels in inr_device.h.  No float atomics: every sum
// over the batch has a fixed order, so two runs on the same inputs give the same bits.
//
// SIREN kinds run the same pipeline through entry points of their own (mrirt_siren_*): the inputs are
// scaled by w0, the hidden layers' epilogue takes the STRICT sine of siren_sincos.h and saves the cosine beside it, and the
// backward multiplies by that cosine where the ReLU step masks.
#include "inr_device.h"
#include "inr_gemm.h"
#include "siren_sincos.h"
#include "mrirt_host.h"

namespace mrirt {

enum { kEpiBias = 0, kEpiMask = 1, kEpiSlab = 2, kEpiSine = 3, kEpiCos = 4 };

template <int BN, bool AKFAST, bool BKFAST, int EPI>
__global__ __launch_bounds__(kTrThreads) void tr_gemm_kernel(TrGemmArgs a) {
    __shared__ float As[kTrBK * TrLds<kTrBM>::pitch];
    __shared__ float Bs[kTrBK * TrLds<BN>::pitch];
    constexpr int NT = BN / 16;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m0 = blockIdx.x * kTrBM, n0 = blockIdx.y * BN;
    int64_t kBegin = 0, kEnd = a.K;
    if (EPI == kEpiSlab) tr_slab_range(a.K, a.slabLen, blockIdx.z, kBegin, kEnd);

    f32x4 acc[NT];                                       // gm_accumulate's loop, kept here: see inr_gemm.h
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    float ra[kTrBM / 16], rb[BN / 16];
    gm_fetch<kTrBM, AKFAST>(a.A, m0, kBegin, kEnd, ra);
    gm_fetch<BN, BKFAST>(a.B, n0, kBegin, kEnd, rb);
    for (int64_t k0 = kBegin; k0 < kEnd; k0 += kTrBK) {
        __syncthreads();                                 // the previous tile's reads are done
        gm_stage<kTrBM, AKFAST>(As, ra);
        gm_stage<BN, BKFAST>(Bs, rb);
        __syncthreads();
        if (k0 + kTrBK < kEnd) {                         // the next tile's loads fly under this tile's MFMAs
            gm_fetch<kTrBM, AKFAST>(a.A, m0, k0 + kTrBK, kEnd, ra);
            gm_fetch<BN, BKFAST>(a.B, n0, k0 + kTrBK, kEnd, rb);
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
        if (col >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = m0 + 16u * wave + tr_acc_row(lane, r);
            if (row >= a.M) continue;
            float v = acc[j][r];
            if (EPI == kEpiBias) {
                v = v + a.bias[col];
                if (a.relu) v = v > 0.0f ? v : 0.0f;
                a.C[(int64_t)row * a.ldc + col] = v;
            } else if (EPI == kEpiMask) {
                const int64_t at = (int64_t)row * a.ldc + col;
                a.C[at] = a.mask[at] > 0.0f ? v : 0.0f;
            } else if (EPI == kEpiSlab) {
                a.C[(uint64_t)blockIdx.z * a.slabStride + (uint64_t)row * a.N + col] = v;
            } else if (EPI == kEpiSine) {                // one accumulator register at a time: the fp64 sincos keeps few live values
                const int64_t at = (int64_t)row * a.ldc + col;
                float sn, cs;
                siren_sincos(v + a.bias[col], sn, cs);
                a.C[at] = sn;
                a.cosOut[at] = cs;
            } else {
                const int64_t at = (int64_t)row * a.ldc + col;
                a.C[at] = v * a.mask[at];
            }
        }
    }
}

template <bool AKFAST, bool BKFAST, int EPI>
static int launch_gemm(const TrGemmArgs& a, uint32_t slabs, hipStream_t s) {
    const uint32_t mt = (a.M + kTrBM - 1) / kTrBM;
    if (a.N <= 16) {
        hipLaunchKernelGGL((tr_gemm_kernel<16, AKFAST, BKFAST, EPI>), dim3(mt, 1, slabs), dim3(kTrThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL((tr_gemm_kernel<64, AKFAST, BKFAST, EPI>), dim3(mt, (a.N + 63) / 64, slabs), dim3(kTrThreads), 0, s, a);
    }
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

// grad (+)= slab 0 + slab 1 + ... in that order; rows < in are dW, row in is db
__global__ __launch_bounds__(256) void tr_slab_reduce_kernel(const float* slab, uint64_t slabStride, uint32_t slabs, uint32_t in,
                                                             uint32_t out, float* gw, float* gb, uint32_t accumulate) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (in + 1u) * out) return;
    float* dst = tr_reduce_dst(i, in, out, gw, gb);
    float s = accumulate ? *dst : 0.0f;
    for (uint32_t z = 0; z < slabs; ++z) s += slab[(uint64_t)z * slabStride + i];
    *dst = s;
}

// x[n][inDim]: feature order of inr/inr/model.py:11-23 (coords, per axis [sin k = 1..K, cos k = 1..K], modalities) with the
// inference path's sine (v_sin_f32 takes revolutions: sin(pi k c) = sin(2 pi (c k / 2)), cos = the same a quarter turn on);
// the raw kind copies feats.
__global__ __launch_bounds__(256) void tr_features_kernel(const float* coords, const float* feats, int64_t n, uint32_t inDim,
                                                          uint32_t K, uint32_t M, uint32_t raw, float* x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * (int64_t)inDim) return;
    const int64_t p = i / inDim;
    const uint32_t f = (uint32_t)(i - p * inDim);
    float v;
    if (raw) v = feats[i];
    else if (f < 3) v = coords[3 * p + f];
    else if (f - 3 < 6 * K) {
        const uint32_t g = f - 3, axis = g / (2 * K), rem = g % (2 * K);
        const bool isSin = rem < K;
        const float mult = (float)((isSin ? rem : rem - K) + 1) * 0.5f;
        v = __builtin_amdgcn_sinf(__builtin_fmaf(coords[3 * p + axis], mult, isSin ? 0.0f : 0.25f));
    } else v = feats[p * M + (f - 3 - 6 * K)];
    x[i] = v;
}

// SIREN: x'[n][inDim] = w0 * (coords, modalities), or w0 * feats for the raw kind; one fp32 multiply per element
__global__ __launch_bounds__(256) void tr_siren_features_kernel(const float* coords, const float* feats, int64_t n, uint32_t inDim,
                                                                uint32_t M, uint32_t raw, float w0, float* x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * (int64_t)inDim) return;
    uint32_t src;
    int64_t off;
    tr_siren_feature_src(i, inDim, M, raw, src, off);
    x[i] = w0 * (src ? feats[off] : coords[off]);
}

// ---- loss ----------------------------------------------------------------------------------------------------------------------

struct LossArgs {
    const float* logits;
    const int32_t* labels;
    int64_t n;
    uint32_t C;
    float cw[kLossMaxClasses];
    float dw;
    double* sums;                // [blocks][kLossVals], then the totals
    uint32_t blocks;
    float* loss;
    float* aux;
    float* dlogits;
};

// the softmax of one point and its cross entropy -log p[label] (0 for a label outside 0..C-1)
__device__ __forceinline__ float point_ce(const float* z, uint32_t C, int32_t label, float (&p)[kLossMaxClasses]) {
    float d[kLossMaxClasses], dl;
    const float s = point_softmax<true>(z, C, label, p, d, dl);
    return (label >= 0 && (uint32_t)label < C) ? logf(s) - dl : 0.0f;
}

__global__ __launch_bounds__(kLossThreads) void loss_partial_kernel(LossArgs a) {
    __shared__ double part[kLossThreads / 64][kLossVals];
    double acc[kLossVals];
#pragma unroll
    for (uint32_t v = 0; v < kLossVals; ++v) acc[v] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < a.n; i += (int64_t)a.blocks * kLossThreads) {
        float p[kLossMaxClasses];
        const int32_t label = a.labels[i];
        const float ce = point_ce(a.logits + i * a.C, a.C, label, p);
        float w = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
            const bool hit = (int32_t)k == label && k < a.C;
            acc[k] += (double)p[k];
            acc[kLossMaxClasses + k] += hit ? (double)p[k] : 0.0;
            acc[2 * kLossMaxClasses + k] += hit ? 1.0 : 0.0;
            acc[3 * kLossMaxClasses + k] += hit ? (double)ce : 0.0;
            if (hit) w = a.cw[k];                        // the guarded class-weight lookup: no label indexes memory
        }
        acc[4 * kLossMaxClasses] += (double)(ce * w);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t v = 0; v < kLossVals; ++v) {
        const double s = wave_sum(acc[v]);
        if (lane == 0) part[wave][v] = s;
    }
    __syncthreads();
    if (threadIdx.x < kLossVals) {
        double s = 0.0;
        for (uint32_t w = 0; w < kLossThreads / 64; ++w) s += part[w][threadIdx.x];
        a.sums[(uint64_t)blockIdx.x * kLossVals + threadIdx.x] = s;
    }
}

// totals in block order, then loss and aux (model.py:74-88)
__global__ __launch_bounds__(128) void loss_final_kernel(LossArgs a) {
    __shared__ double tot[kLossVals];
    if (threadIdx.x < kLossVals) {
        double s = 0.0;
        for (uint32_t b = 0; b < a.blocks; ++b) s += a.sums[(uint64_t)b * kLossVals + threadIdx.x];
        tot[threadIdx.x] = s;
        a.sums[(uint64_t)a.blocks * kLossVals + threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double diceMean = 0.0;
        for (uint32_t k = 0; k < a.C; ++k) {
            const double dice = (2.0 * tot[kLossMaxClasses + k] + 1e-6) / (tot[k] + tot[2 * kLossMaxClasses + k] + 1e-6);
            const double cnt = tot[2 * kLossMaxClasses + k];
            diceMean += dice;
            a.aux[k] = (float)(tot[3 * kLossMaxClasses + k] / (cnt > 1.0 ? cnt : 1.0));
            a.aux[a.C + k] = (float)dice;
        }
        diceMean /= (double)a.C;
        const double ce = tot[4 * kLossMaxClasses] / (double)a.n;
        const double dw = (double)a.dw;
        a.loss[0] = (float)(a.dw > 0.0f ? (1.0 - dw) * ce + dw * (1.0 - diceMean) : ce);
    }
}

// dloss/dlogits = (1 - dw) cw[label] / n (p - y)  +  p (g - sum_k g_k p_k),  g_k = -(dw / C) (2 y_k - dice_k) / (S_k + eps)
__global__ __launch_bounds__(kLossThreads) void loss_grad_kernel(LossArgs a) {
    __shared__ float gA[kLossMaxClasses], gB[kLossMaxClasses];      // g_k = gB[k] - gA[k] y_k
    if (threadIdx.x < kLossMaxClasses) {
        const uint32_t k = threadIdx.x;
        float ga = 0.0f, gb = 0.0f;
        if (k < a.C && a.dw > 0.0f) {
            const double* tot = a.sums + (uint64_t)a.blocks * kLossVals;
            const double den = tot[k] + tot[2 * kLossMaxClasses + k] + 1e-6;
            const double dice = (2.0 * tot[kLossMaxClasses + k] + 1e-6) / den;
            const double c = (double)a.dw / (double)a.C / den;
            ga = (float)(2.0 * c);
            gb = (float)(c * dice);
        }
        gA[k] = ga; gB[k] = gb;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (i >= a.n) return;
    float p[kLossMaxClasses];
    const int32_t label = a.labels[i];
    point_ce(a.logits + i * a.C, a.C, label, p);
    float w = 0.0f, dot = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        const bool hit = (int32_t)k == label && k < a.C;
        if (hit) w = a.cw[k];
        dot += (gB[k] - (hit ? gA[k] : 0.0f)) * p[k];
    }
    const float ceScale = (a.dw > 0.0f ? 1.0f - a.dw : 1.0f) * w / (float)a.n;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        if (k >= a.C) continue;
        const bool hit = (int32_t)k == label;
        const float g = gB[k] - (hit ? gA[k] : 0.0f);
        a.dlogits[i * a.C + k] = ceScale * (p[k] - (hit ? 1.0f : 0.0f)) + p[k] * (g - dot);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

// The shapes one family of entry points takes: the ReLU kinds for mrirt_inr_*, the SIREN kinds (no Fourier features, a
// finite non-zero w0) for mrirt_siren_*.  L.bytes is the family's scratch size.
static int train_desc(const MrirtInrDesc* d, int64_t n, bool siren, TrainLayout& L, SirenLayout& S) {
    if (!d) return MRIRT_ERR_NULL;
    if (siren) {
        if (d->kind != MRIRT_INR_SIREN && d->kind != MRIRT_INR_RAW_SIREN) return MRIRT_ERR_ARG;
        if (d->fourierFreqs != 0 || !isfinite(d->w0) || d->w0 == 0.0f) return MRIRT_ERR_ARG;
    } else if (d->kind != MRIRT_INR_FOURIER_RELU && d->kind != MRIRT_INR_RAW_RELU) return MRIRT_ERR_ARG;
    if (mrirt_inr_pack_bytes(d) <= 0) return MRIRT_ERR_ARG;             // the shapes the packer accepts
    if (n < 1 || n >= (1ll << 31)) return MRIRT_ERR_ARG;
    S = siren_layout(d->numLayers, d->inDim, d->hidden, d->outDim, n);
    L = S.T;
    if (siren) L.bytes = S.bytes;
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

static int64_t scratch_bytes_of(const MrirtInrDesc* desc, int64_t n, bool siren) {
    TrainLayout L;
    SirenLayout S;
    return train_desc(desc, n, siren, L, S) == MRIRT_OK ? (int64_t)L.bytes : 0;
}

extern "C" int64_t mrirt_inr_train_scratch_bytes(const MrirtInrDesc* desc, int64_t n) { return scratch_bytes_of(desc, n, false); }
extern "C" int64_t mrirt_siren_train_scratch_bytes(const MrirtInrDesc* desc, int64_t n) { return scratch_bytes_of(desc, n, true); }

extern "C" int64_t mrirt_inr_loss_scratch_bytes(int64_t n) {
    return (n < 1 || n >= (1ll << 31)) ? 0 : (int64_t)loss_scratch_bytes(n);
}

static int forward_f32(const MrirtInrDesc* desc, bool siren, const float* w_f32, const float* b_f32, const float* coords,
                       const float* feats, int64_t n, float* logits, void* scratch, int64_t scratch_bytes, void* stream) {
    TrainLayout L;
    SirenLayout S;
    if (!desc || !w_f32 || !b_f32 || !logits) return MRIRT_ERR_NULL;
    int rc = train_desc(desc, n, siren, L, S);
    if (rc != MRIRT_OK) return rc;
    const bool raw = desc->kind == MRIRT_INR_RAW_RELU || desc->kind == MRIRT_INR_RAW_SIREN;
    if ((!raw && !coords) || ((raw || desc->numMods > 0) && !feats)) return MRIRT_ERR_NULL;
    if ((rc = check_scratch(scratch, scratch_bytes, L.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    float* x = (float*)(base + L.offX);
    const int64_t total = n * (int64_t)L.inDim;
    if (siren)
        hipLaunchKernelGGL(tr_siren_features_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, coords, feats, n, L.inDim,
                           desc->numMods, raw ? 1u : 0u, desc->w0, x);
    else
        hipLaunchKernelGGL(tr_features_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, coords, feats, n, L.inDim,
                           desc->fourierFreqs, desc->numMods, raw ? 1u : 0u, x);
    MRIRT_HIP(hipGetLastError());
    const float* h = x;
    for (uint32_t l = 0; l < L.numLayers; ++l) {
        const bool head = l + 1 == L.numLayers;
        float* out = head ? logits : (float*)(base + tr_in_offset(L, l + 1, n));
        if (siren && !head)
            rc = launch_gemm<true, false, kEpiSine>(tr_sine_args(S, l, n, h, w_f32, b_f32, out, (float*)(base + tr_cos_offset(S, l, n))), 1, s);
        else
            rc = launch_gemm<true, false, kEpiBias>(tr_forward_args(L, l, n, h, w_f32, b_f32, out), 1, s);
        if (rc != MRIRT_OK) return rc;
        h = out;
    }
    return MRIRT_OK;
}

extern "C" int mrirt_inr_forward_f32(const MrirtInrDesc* desc, const float* w_f32, const float* b_f32, const float* coords,
                                     const float* feats, int64_t n, float* logits, void* scratch, int64_t scratch_bytes,
                                     void* stream) {
    return forward_f32(desc, false, w_f32, b_f32, coords, feats, n, logits, scratch, scratch_bytes, stream);
}

extern "C" int mrirt_siren_forward_f32(const MrirtInrDesc* desc, const float* w_f32, const float* b_f32, const float* coords,
                                       const float* feats, int64_t n, float* logits, void* scratch, int64_t scratch_bytes,
                                       void* stream) {
    return forward_f32(desc, true, w_f32, b_f32, coords, feats, n, logits, scratch, scratch_bytes, stream);
}

extern "C" int mrirt_inr_loss(const float* logits, const int32_t* labels, int64_t n, uint32_t num_classes,
                              const float* class_weights, float dice_weight, float* loss, float* aux, float* dlogits,
                              void* scratch, int64_t scratch_bytes, void* stream) {
    if (!logits || !labels || !class_weights || !loss || !aux) return MRIRT_ERR_NULL;
    if (n < 1 || n >= (1ll << 31) || num_classes < 1 || num_classes > kLossMaxClasses || !isfinite(dice_weight)) return MRIRT_ERR_ARG;
    const int rc = check_scratch(scratch, scratch_bytes, loss_scratch_bytes(n));
    if (rc != MRIRT_OK) return rc;
    LossArgs a = {};
    a.logits = logits; a.labels = labels; a.n = n; a.C = num_classes; a.dw = dice_weight;
    for (uint32_t k = 0; k < num_classes; ++k) a.cw[k] = class_weights[k];
    a.sums = (double*)scratch; a.blocks = loss_blocks(n);
    a.loss = loss; a.aux = aux; a.dlogits = dlogits;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_partial_kernel, dim3(a.blocks), dim3(kLossThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(128), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    if (dlogits) {
        hipLaunchKernelGGL(loss_grad_kernel, dim3((uint32_t)((n + kLossThreads - 1) / kLossThreads)), dim3(kLossThreads), 0, s, a);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}

static int backward_f32(const MrirtInrDesc* desc, bool siren, const float* w_f32, int64_t n, const float* dlogits, float* grad_w,
                        float* grad_b, uint32_t flags, void* scratch, int64_t scratch_bytes, void* stream) {
    TrainLayout L;
    SirenLayout S;
    if (!desc || !w_f32 || !dlogits || !grad_w || !grad_b) return MRIRT_ERR_NULL;
    int rc = train_desc(desc, n, siren, L, S);
    if (rc != MRIRT_OK) return rc;
    if (flags > 1u) return MRIRT_ERR_ARG;
    if ((rc = check_scratch(scratch, scratch_bytes, L.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    float* slab = (float*)(base + L.offSlab);
    const float* dz = dlogits;
    for (uint32_t l = L.numLayers; l-- > 0;) {
        const float* hin = (const float*)(base + tr_in_offset(L, l, n));
        if ((rc = launch_gemm<false, false, kEpiSlab>(tr_slab_args(L, l, n, hin, dz, slab), L.slabs, s)) != MRIRT_OK) return rc;
        const uint32_t elems = (L.in[l] + 1) * L.out[l];
        hipLaunchKernelGGL(tr_slab_reduce_kernel, dim3((elems + 255) / 256), dim3(256), 0, s, slab, L.slabElems, L.slabs, L.in[l],
                           L.out[l], grad_w + L.wOff[l], grad_b + L.bOff[l], flags & 1u);
        MRIRT_HIP(hipGetLastError());
        if (l == 0) break;
        float* dzPrev = (float*)(base + tr_dz_offset(L, l, n));
        if (siren)
            rc = launch_gemm<true, true, kEpiCos>(tr_cos_args(S, l, n, dz, w_f32, (const float*)(base + tr_cos_offset(S, l - 1, n)), dzPrev), 1, s);
        else
            rc = launch_gemm<true, true, kEpiMask>(tr_mask_args(L, l, n, dz, w_f32, hin, dzPrev), 1, s);
        if (rc != MRIRT_OK) return rc;
        dz = dzPrev;
    }
    return MRIRT_OK;
}

extern "C" int mrirt_inr_backward(const MrirtInrDesc* desc, const float* w_f32, int64_t n, const float* dlogits, float* grad_w,
                                  float* grad_b, uint32_t flags, void* scratch, int64_t scratch_bytes, void* stream) {
    return backward_f32(desc, false, w_f32, n, dlogits, grad_w, grad_b, flags, scratch, scratch_bytes, stream);
}

extern "C" int mrirt_siren_backward(const MrirtInrDesc* desc, const float* w_f32, int64_t n, const float* dlogits, float* grad_w,
                                    float* grad_b, uint32_t flags, void* scratch, int64_t scratch_bytes, void* stream) {
    return backward_f32(desc, true, w_f32, n, dlogits, grad_w, grad_b, flags, scratch, scratch_bytes, stream);
}
