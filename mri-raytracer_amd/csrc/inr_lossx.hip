// The loss and the sampling mix of the reference's richest trainer (scripts/jax_inr_brats.py:179-257, 466-528; DESIGN.md
// section 18), beside the plain ones of csrc/inr_train.hip / csrc/inr_optim.hip, which stay as they are.
//   lossx_partial_kernel   per-point softmax, smoothed targets, CE / focal CE, the edema sums -> per-block fp64 sums
//   lossx_final_kernel     totals in block order -> loss, aux, terms
//   lossx_grad_kernel      the exact derivative through the softmax Jacobian
//   tum_count_kernel       tumour voxels (seg > 0) per case
//   tum_chunk_kernel / tum_scan_kernel / tum_emit_kernel   the ascending tumour index: count per chunk, scan per case, emit
//   sample_mix_kernel      mrirt_inr_sample_batch with the first nTumour points drawn from the tumour index
// The focal CE is the PRODUCT OF TWO MEANS, [(1/n) sum m ce] [(1/n) sum w]: the reference's focal_ce_loss returns a scalar,
// which lines 230-233 then multiply by the class-weight vector and average.  It is reproduced, not repaired.
// No float atomics, no label indexes memory, every sum over the batch is fp64 in a fixed order.  The softmax, the wave sum
// and the sampler's write-out are inr_device.h's, shared with csrc/inr_train.hip and csrc/inr_optim.hip.
#include "inr_device.h"
#include "inr_lossx.h"
#include "mrirt_host.h"

namespace mrirt {

struct LossXArgs {
    const float* logits;
    const int32_t* labels;
    int64_t n;
    uint32_t C;
    float cw[kLossMaxClasses];
    float alpha[kLossMaxClasses];    // 1 without flags bit 1
    float dw, gamma, eps;
    float fpW, tvA, tvB, tvW, regW;
    uint32_t e;                      // edema class; >= C: no edema sums
    uint32_t perClassDice, focal, useAlpha;
    double* sums;                    // [blocks][kLossXVals], then the totals
    uint32_t blocks;
    float* loss;
    float* aux;
    float* terms;
    float* dlogits;
};

// What both passes need of one point.  y[k] = yh (1 - eps) + eps / C (exactly yh for eps == 0); ce = sum_k y_k (ls - d_k):
// for eps == 0 the one non-zero term, logf(s) - d_label, as mrirt_inr_loss forms it.
struct LxPoint {
    float ce, w, sumY, pt, a;
};
__device__ __forceinline__ LxPoint lossx_point(const LossXArgs& a, int32_t label, float ls, const float (&p)[kLossMaxClasses],
                                               const float (&d)[kLossMaxClasses], float (&y)[kLossMaxClasses]) {
    LxPoint r = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    const float on = 1.0f - a.eps, off = a.eps / (float)a.C;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        const bool hit = (int32_t)k == label && k < a.C;
        y[k] = 0.0f;
        if (k < a.C) {
            y[k] = a.eps > 0.0f ? (hit ? 1.0f : 0.0f) * on + off : (hit ? 1.0f : 0.0f);
            if (y[k] != 0.0f) {
                r.ce += y[k] * (ls - d[k]);
                r.pt += y[k] * p[k];
                r.a += y[k] * a.alpha[k];
                r.sumY += y[k];
            }
        }
        if (hit) r.w = a.cw[k];                          // the guarded class-weight lookup: no label indexes memory
    }
    if (!a.useAlpha) r.a = 1.0f;
    return r;
}

__device__ __forceinline__ float lx_softplus(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float lx_sigmoid(float z) {
    const float t = expf(-fabsf(z));
    return z >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
}

__global__ __launch_bounds__(kLossThreads) void lossx_partial_kernel(LossXArgs a) {
    __shared__ double part[kLossThreads / 64][kLossXVals];
    double acc[kLossXVals];
#pragma unroll
    for (uint32_t v = 0; v < kLossXVals; ++v) acc[v] = 0.0;
    for (int64_t i = lossx_first(blockIdx.x, threadIdx.x); i < a.n; i += lossx_stride(a.blocks)) {
        float p[kLossMaxClasses], d[kLossMaxClasses], y[kLossMaxClasses];
        const int32_t label = a.labels[i];
        const float* z = a.logits + i * a.C;
        const float ls = logf(point_softmax(z, a.C, p, d));
        const LxPoint r = lossx_point(a, label, ls, p, d, y);
        float q = 0.0f, ze = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
            const bool hit = (int32_t)k == label && k < a.C;
            acc[k] += (double)p[k];
            acc[kLossMaxClasses + k] += (double)p[k] * (double)y[k];
            acc[2 * kLossMaxClasses + k] += hit ? 1.0 : 0.0;
            acc[3 * kLossMaxClasses + k] += hit ? (double)r.ce : 0.0;
            if (k == a.e && k < a.C) { q = p[k]; ze = z[k]; }
        }
        acc[4 * kLossMaxClasses] += (double)(r.ce * r.w);
        acc[kLxW] += (double)r.w;
        if (a.focal) {
            const float u = fmaxf(1.0f - r.pt, 0.0f);
            acc[kLxFocal] += (double)((powf(u, a.gamma) * r.a) * r.ce);
        }
        if (a.e < a.C) {
            const bool g = label == (int32_t)a.e;
            acc[kLxTp] += g ? (double)q : 0.0;
            acc[kLxFp] += g ? 0.0 : (double)q;
            acc[kLxFn] += g ? (double)(1.0f - q) : 0.0;
            acc[kLxReg] += g ? 0.0 : (double)lx_softplus(ze);
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t v = 0; v < kLossXVals; ++v) {
        const double s = wave_sum(acc[v]);
        if (lane == 0) part[wave][v] = s;
    }
    __syncthreads();
    if (threadIdx.x < kLossXVals) {
        double s = 0.0;
        for (uint32_t w = 0; w < kLossThreads / 64; ++w) s += part[w][threadIdx.x];
        a.sums[lossx_sum_index(blockIdx.x, threadIdx.x)] = s;
    }
}

// the Dice weight of class k: 1 / C, or the prevalence v_k = Y_k / (sum_j Y_j + 1e-6) with Y_k = (1 - eps) count_k + n eps / C
__device__ __forceinline__ double lx_prevalence(const LossXArgs& a, const double* tot, uint32_t k) {
    const double on = 1.0 - (double)a.eps, off = (double)a.n * ((double)a.eps / (double)a.C);
    double all = 0.0;
    for (uint32_t j = 0; j < a.C; ++j) all += on * tot[2 * kLossMaxClasses + j] + off;
    return (on * tot[2 * kLossMaxClasses + k] + off) / (all + 1e-6);
}
__device__ __forceinline__ double lx_dice_den(const LossXArgs& a, const double* tot, uint32_t k) {
    const double on = 1.0 - (double)a.eps, off = (double)a.n * ((double)a.eps / (double)a.C);
    const double Y = a.eps > 0.0f ? on * tot[2 * kLossMaxClasses + k] + off : tot[2 * kLossMaxClasses + k];
    return tot[k] + Y + 1e-6;
}

// totals in block order, then loss, aux and terms
__global__ __launch_bounds__(kLossXFinalThreads) void lossx_final_kernel(LossXArgs a) {
    __shared__ double tot[kLossXVals];
    if (threadIdx.x < kLossXVals) {
        double s = 0.0;
        for (uint32_t b = 0; b < a.blocks; ++b) s += a.sums[lossx_sum_index(b, threadIdx.x)];
        tot[threadIdx.x] = s;
        a.sums[lossx_sum_index(a.blocks, threadIdx.x)] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double diceMean = 0.0, diceWeighted = 0.0;
        for (uint32_t k = 0; k < a.C; ++k) {
            const double dice = (2.0 * tot[kLossMaxClasses + k] + 1e-6) / lx_dice_den(a, tot, k);
            const double cnt = tot[2 * kLossMaxClasses + k];
            diceMean += dice;
            if (!a.perClassDice) diceWeighted += dice * lx_prevalence(a, tot, k);
            a.aux[k] = (float)(tot[3 * kLossMaxClasses + k] / (cnt > 1.0 ? cnt : 1.0));
            a.aux[a.C + k] = (float)dice;
        }
        diceMean /= (double)a.C;
        const double n = (double)a.n;
        const double ce = a.focal ? (tot[kLxFocal] / n) * (tot[kLxW] / n) : tot[4 * kLossMaxClasses] / n;
        const double dw = (double)a.dw;
        const double dl = a.perClassDice ? 1.0 - diceMean : 1.0 - diceWeighted;
        double loss = a.dw > 0.0f ? (1.0 - dw) * ce + dw * dl : ce;
        const double fp = tot[kLxFp] / n, reg = tot[kLxReg] / n;
        const double tv = tot[kLxTp] / (tot[kLxTp] + (double)a.tvA * tot[kLxFp] + (double)a.tvB * tot[kLxFn] + 1e-6);
        if (a.fpW > 0.0f) loss += (double)a.fpW * fp;
        if (a.tvW > 0.0f) loss += (double)a.tvW * (1.0 - tv);
        if (a.regW > 0.0f) loss += (double)a.regW * reg;
        a.loss[0] = (float)loss;
        if (a.terms) {
            a.terms[0] = (float)ce;
            a.terms[1] = a.dw > 0.0f ? (float)dl : 0.0f;
            a.terms[2] = (float)fp;
            a.terms[3] = (float)tv;
            a.terms[4] = (float)reg;
        }
    }
}

// dloss/dz_j = sum_k dL/dlogp_k (delta_jk - p_j) + p_j (G_j - sum_k G_k p_k) (+ the softplus' own term at j = e), with
//   dL/dlogp_k = -s m y_k                        s = (1 - dw) w / n, m = 1 (plain) or s = (1 - dw) wbar / n, m the focal factor
//   G_k = gB[k] - gA[k] y_k                      Dice: gA = 2 dw c_k / den_k, gB = dw c_k dice_k / den_k
//       - s ce a gamma u^(gamma - 1) y_k         focal, u = max(1 - pt, 0)
//       + [k == e] (edema: fpW (1 - g) / n - tvW dT/dq)
__global__ __launch_bounds__(kLossThreads) void lossx_grad_kernel(LossXArgs a) {
    __shared__ float gA[kLossMaxClasses], gB[kLossMaxClasses];
    __shared__ float sh[4];                              // [0] wbar, [1] edema G for g = 1, [2] for g = 0, [3] regW / n
    const double* tot = a.sums + lossx_sum_index(a.blocks, 0);
    if (threadIdx.x < kLossMaxClasses) {
        const uint32_t k = threadIdx.x;
        float ga = 0.0f, gb = 0.0f;
        if (k < a.C && a.dw > 0.0f) {
            const double den = lx_dice_den(a, tot, k);
            const double dice = (2.0 * tot[kLossMaxClasses + k] + 1e-6) / den;
            const double c = a.perClassDice ? (double)a.dw / (double)a.C / den : (double)a.dw * lx_prevalence(a, tot, k) / den;
            ga = (float)(2.0 * c);
            gb = (float)(c * dice);
        }
        gA[k] = ga; gB[k] = gb;
    }
    if (threadIdx.x == kLossMaxClasses) {
        const double n = (double)a.n;
        const double TP = tot[kLxTp], D = TP + (double)a.tvA * tot[kLxFp] + (double)a.tvB * tot[kLxFn] + 1e-6;
        double ge1 = 0.0, ge0 = 0.0;
        if (a.fpW > 0.0f) ge0 += (double)a.fpW / n;
        if (a.tvW > 0.0f) {                              // T = TP / D: dT/dq = (D - TP (1 - beta)) / D^2 on edema, -TP alpha / D^2 off it
            ge1 -= (double)a.tvW * (D - TP * (1.0 - (double)a.tvB)) / (D * D);
            ge0 += (double)a.tvW * TP * (double)a.tvA / (D * D);
        }
        sh[0] = (float)(tot[kLxW] / n);
        sh[1] = (float)ge1;
        sh[2] = (float)ge0;
        sh[3] = a.regW > 0.0f ? (float)((double)a.regW / n) : 0.0f;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (i >= a.n) return;
    float p[kLossMaxClasses], d[kLossMaxClasses], y[kLossMaxClasses];
    const int32_t label = a.labels[i];
    const float* z = a.logits + i * a.C;
    const float ls = logf(point_softmax(z, a.C, p, d));
    const LxPoint r = lossx_point(a, label, ls, p, d, y);
    const float ceScale = (a.dw > 0.0f ? 1.0f - a.dw : 1.0f) * (a.focal ? sh[0] : r.w) / (float)a.n;
    float m = 1.0f, fg = 0.0f;                           // the focal factor and its p-path coefficient
    if (a.focal) {
        const float u = fmaxf(1.0f - r.pt, 0.0f);
        m = powf(u, a.gamma) * r.a;
        fg = ((ceScale * r.ce) * r.a) * (a.gamma * powf(u, a.gamma - 1.0f));
    }
    const bool edema = a.e < a.C && (a.fpW > 0.0f || a.tvW > 0.0f);
    const bool isE = label == (int32_t)a.e;
    float G[kLossMaxClasses], dot = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        float g = gB[k] - gA[k] * y[k];
        if (a.focal) g -= fg * y[k];
        if (edema && k == a.e) g += isE ? sh[1] : sh[2];
        G[k] = g;
        dot += g * p[k];
    }
    const float lp = a.focal ? ceScale * m : ceScale;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        if (k >= a.C) continue;
        float v = lp * (p[k] * r.sumY - y[k]) + p[k] * (G[k] - dot);
        if (k == a.e && a.regW > 0.0f && !isE) v += sh[3] * lx_sigmoid(z[k]);
        a.dlogits[i * a.C + k] = v;
    }
}

static bool lx_weight(float v) { return isfinite(v) && v >= 0.0f; }

int lossx_check(const MrirtInrLossExt* x, uint32_t C) {
    if (!x) return MRIRT_ERR_NULL;
    if (C < 1 || C > kLossMaxClasses) return MRIRT_ERR_ARG;
    if (!(x->focalGamma == 0.0f || (x->focalGamma >= 1.0f && x->focalGamma <= 8.0f))) return MRIRT_ERR_ARG;      // NaN fails both
    if (!(x->labelSmoothing >= 0.0f && x->labelSmoothing < 1.0f) || !isfinite(x->diceWeight) || x->flags > 3u) return MRIRT_ERR_ARG;
    if (!lx_weight(x->edemaFpWeight) || !lx_weight(x->tverskyAlpha) || !lx_weight(x->tverskyBeta) || !lx_weight(x->tverskyWeight) ||
        !lx_weight(x->edemaLogitReg)) return MRIRT_ERR_ARG;
    for (uint32_t k = 0; k < C; ++k)
        if (!isfinite(x->classWeights[k]) || ((x->flags & 2u) && !isfinite(x->focalAlpha[k]))) return MRIRT_ERR_ARG;
    if (x->edemaClass >= C && (x->edemaFpWeight > 0.0f || x->tverskyWeight > 0.0f || x->edemaLogitReg > 0.0f)) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

// ---- tumour index --------------------------------------------------------------------------------------------------------------

struct TumArgs {
    const int16_t* const* seg;
    uint64_t hwd;
    uint32_t ncases, chunks;     // chunks per case
    unsigned long long* counts;  // tum_count_kernel
    uint32_t* chunkSums;         // [ncases][chunks]
    const int64_t* offsets;
    uint32_t* index;
};

__device__ __forceinline__ uint32_t tum_thread_count(const int16_t* seg, uint64_t first, uint64_t hwd) {
    uint32_t c = 0;
    for (uint32_t j = 0; j < kTumPerThread; ++j) {
        const uint64_t v = first + j;
        if (v < hwd && seg[v] > 0) ++c;
    }
    return c;
}

// the block's total in every thread (integer sums: any order gives the same value)
__device__ __forceinline__ uint32_t tum_block_sum(uint32_t c, uint32_t* lds) {
    lds[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t s = kTumThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    const uint32_t t = lds[0];
    __syncthreads();
    return t;
}

// grid (x, ncases): block x of a case strides over its chunks; one integer atomic per block (an integer sum has no order)
__global__ __launch_bounds__(kTumThreads) void tum_count_kernel(TumArgs a) {
    __shared__ uint32_t lds[kTumThreads];
    const int16_t* seg = a.seg[blockIdx.y];
    unsigned long long total = 0;
    for (uint32_t chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) total += tum_block_sum(tum_thread_count(seg, tum_first(chunk, threadIdx.x), a.hwd), lds);
    if (threadIdx.x == 0 && total) atomicAdd(a.counts + blockIdx.y, total);
}

// grid (chunks, ncases)
__global__ __launch_bounds__(kTumThreads) void tum_chunk_kernel(TumArgs a) {
    __shared__ uint32_t lds[kTumThreads];
    const uint32_t t = tum_block_sum(tum_thread_count(a.seg[blockIdx.y], tum_first(blockIdx.x, threadIdx.x), a.hwd), lds);
    if (threadIdx.x == 0) a.chunkSums[tum_chunk_slot(blockIdx.y, blockIdx.x, a.chunks)] = t;
}

// grid (ncases): the chunk sums of a case -> their exclusive prefix, in place
__global__ __launch_bounds__(kTumThreads) void tum_scan_kernel(TumArgs a) {
    __shared__ uint32_t lds[kTumThreads];
    const uint32_t len = tum_scan_len(a.chunks), first = threadIdx.x * len;
    uint32_t* s = a.chunkSums + tum_chunk_slot(blockIdx.x, 0, a.chunks);
    uint32_t mine = 0;
    for (uint32_t j = first; j < first + len && j < a.chunks; ++j) mine += s[j];
    lds[threadIdx.x] = mine;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) before += lds[t];
    for (uint32_t j = first; j < first + len && j < a.chunks; ++j) {
        const uint32_t c = s[j];
        s[j] = before;
        before += c;
    }
}

// grid (chunks, ncases): thread t's voxels land behind those of threads < t of its chunk, behind the chunks before it
__global__ __launch_bounds__(kTumThreads) void tum_emit_kernel(TumArgs a) {
    __shared__ uint32_t lds[kTumThreads];
    const int16_t* seg = a.seg[blockIdx.y];
    const uint64_t first = tum_first(blockIdx.x, threadIdx.x);
    lds[threadIdx.x] = tum_thread_count(seg, first, a.hwd);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) before += lds[t];
    const int64_t lo = a.offsets[blockIdx.y], hi = a.offsets[blockIdx.y + 1];
    int64_t at = lo + (int64_t)a.chunkSums[tum_chunk_slot(blockIdx.y, blockIdx.x, a.chunks)] + before;
    for (uint32_t j = 0; j < kTumPerThread; ++j) {
        const uint64_t v = first + j;
        if (v < a.hwd && seg[v] > 0) {
            if (at >= lo && at < hi) a.index[at] = (uint32_t)v;      // offsets that do not match the counts write nothing outside a case's range
            ++at;
        }
    }
}

// ---- mixed sampler ---------------------------------------------------------------------------------------------------------------

struct MixArgs {
    const float* const* mods;
    const int16_t* const* seg;
    uint32_t ncases, M, H, W, D;
    int64_t hwd;
    uint64_t seed, batch;
    int64_t n, nTumour;
    const uint32_t* index;
    const int64_t* offsets;
    float* coords;
    float* feats;
    int32_t* labels;
};

__global__ __launch_bounds__(kOptThreads) void sample_mix_kernel(MixArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (i >= a.n) return;
    const MixDraw dr = mix_words(a.seed, a.batch, (uint32_t)i);
    SamplePoint p = mix_uniform(dr, a.ncases, a.H, a.W, a.D);
    if (i < a.nTumour) {
        const int64_t first = a.offsets[p.cs], cnt = a.offsets[p.cs + 1] - first;
        if (cnt > 0) {
            const uint32_t v = a.index[mix_slot(dr.r[1], first, cnt)];
            if ((int64_t)v < a.hwd) tum_decode(v, a.W, a.D, p.x, p.y, p.z);      // a foreign index cannot point outside the volume
        }
    }
    sample_write(i, p, a.mods, a.seg, a.M, a.H, a.W, a.D, a.hwd, a.coords, a.feats, a.labels);
}

static int tum_check_cache(const MrirtInrCache* c) {
    if (!c) return MRIRT_ERR_NULL;
    const uint64_t hw = (uint64_t)c->hwd[0] * c->hwd[1];                // < 2^64; hw < 2^32 keeps hw * D there too
    if (hw >= (1ull << 32) || hw * c->hwd[2] >= (1ull << 32)) return MRIRT_ERR_ARG;
    return opt_check_cache(c);
}

static TumArgs tum_args(const MrirtInrCache* c) {
    TumArgs a = {};
    a.seg = c->seg;
    a.hwd = (uint64_t)c->hwd[0] * c->hwd[1] * c->hwd[2];
    a.ncases = c->ncases;
    a.chunks = tum_chunks(a.hwd);
    return a;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_inr_loss_ext_scratch_bytes(int64_t n) {
    return (n < 1 || n >= (1ll << 31)) ? 0 : (int64_t)lossx_scratch_bytes(n);
}

extern "C" int mrirt_inr_loss_ext(const float* logits, const int32_t* labels, int64_t n, uint32_t num_classes, const MrirtInrLossExt* ext,
                                  float* loss, float* aux, float* terms, float* dlogits, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!logits || !labels || !ext || !loss || !aux) return MRIRT_ERR_NULL;
    if (n < 1 || n >= (1ll << 31)) return MRIRT_ERR_ARG;
    int rc = lossx_check(ext, num_classes);
    if (rc != MRIRT_OK) return rc;
    if ((rc = check_scratch(scratch, scratch_bytes, lossx_scratch_bytes(n))) != MRIRT_OK) return rc;
    LossXArgs a = {};
    a.logits = logits; a.labels = labels; a.n = n; a.C = num_classes;
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) a.alpha[k] = 1.0f;
    for (uint32_t k = 0; k < num_classes; ++k) {
        a.cw[k] = ext->classWeights[k];
        if (ext->flags & 2u) a.alpha[k] = ext->focalAlpha[k];
    }
    a.dw = ext->diceWeight; a.gamma = ext->focalGamma; a.eps = ext->labelSmoothing;
    a.fpW = ext->edemaFpWeight; a.tvA = ext->tverskyAlpha; a.tvB = ext->tverskyBeta; a.tvW = ext->tverskyWeight; a.regW = ext->edemaLogitReg;
    a.e = ext->edemaClass;
    a.perClassDice = ext->flags & 1u; a.focal = ext->focalGamma > 0.0f ? 1u : 0u; a.useAlpha = (ext->flags >> 1) & 1u;
    a.sums = (double*)scratch; a.blocks = loss_blocks(n);
    a.loss = loss; a.aux = aux; a.terms = terms; a.dlogits = dlogits;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lossx_partial_kernel, dim3(a.blocks), dim3(kLossThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(lossx_final_kernel, dim3(1), dim3(kLossXFinalThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    if (dlogits) {
        hipLaunchKernelGGL(lossx_grad_kernel, dim3((uint32_t)((n + kLossThreads - 1) / kLossThreads)), dim3(kLossThreads), 0, s, a);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}

extern "C" int mrirt_inr_tumour_count(const MrirtInrCache* cache, int64_t* counts, void* stream) {
    if (!cache || !counts) return MRIRT_ERR_NULL;
    const int rc = tum_check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    TumArgs a = tum_args(cache);
    a.counts = (unsigned long long*)counts;
    hipStream_t s = (hipStream_t)stream;
    MRIRT_HIP(hipMemsetAsync(counts, 0, (size_t)cache->ncases * sizeof(int64_t), s));
    hipLaunchKernelGGL(tum_count_kernel, dim3(a.chunks < 64u ? a.chunks : 64u, a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int64_t mrirt_inr_tumour_index_scratch_bytes(const MrirtInrCache* cache) {
    if (tum_check_cache(cache) != MRIRT_OK) return 0;
    return (int64_t)tum_scratch_bytes(cache->ncases, (uint64_t)cache->hwd[0] * cache->hwd[1] * cache->hwd[2]);
}

extern "C" int mrirt_inr_tumour_index(const MrirtInrCache* cache, const int64_t* offsets, uint32_t* index, void* scratch,
                                      int64_t scratch_bytes, void* stream) {
    if (!cache || !offsets || !index) return MRIRT_ERR_NULL;
    int rc = tum_check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    TumArgs a = tum_args(cache);
    if ((rc = check_scratch(scratch, scratch_bytes, tum_scratch_bytes(a.ncases, a.hwd))) != MRIRT_OK) return rc;
    a.chunkSums = (uint32_t*)scratch; a.offsets = offsets; a.index = index;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tum_chunk_kernel, dim3(a.chunks, a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(tum_scan_kernel, dim3(a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(tum_emit_kernel, dim3(a.chunks, a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_inr_sample_batch_mix(const MrirtInrCache* cache, const MrirtInrTumourIndex* tumour, uint64_t seed, uint64_t batch_index,
                                          int64_t n, int64_t n_tumour, float* coords, float* feats, int32_t* labels, void* stream) {
    if (!cache || !coords || !labels) return MRIRT_ERR_NULL;
    const int rc = opt_check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    if (cache->numMods > 0 && !feats) return MRIRT_ERR_NULL;
    if (n < 1 || n >= (1ll << 31) || n_tumour < 0 || n_tumour > n) return MRIRT_ERR_ARG;
    if (n_tumour > 0 && (!tumour || !tumour->index || !tumour->offsets)) return MRIRT_ERR_NULL;
    MixArgs a = {};
    a.mods = cache->mods; a.seg = cache->seg; a.ncases = cache->ncases; a.M = cache->numMods;
    a.H = cache->hwd[0]; a.W = cache->hwd[1]; a.D = cache->hwd[2];
    a.hwd = (int64_t)a.H * a.W * a.D;
    a.seed = seed; a.batch = batch_index; a.n = n; a.nTumour = n_tumour;
    if (n_tumour > 0) { a.index = tumour->index; a.offsets = tumour->offsets; }
    a.coords = coords; a.feats = feats; a.labels = labels;
    hipLaunchKernelGGL(sample_mix_kernel, dim3((uint32_t)((n + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, (hipStream_t)stream, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
