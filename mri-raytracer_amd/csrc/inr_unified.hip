// The loss of the reference's coordinate-injection notebook (notebooks/improved.ipynb, cell 8): unified
// focal (focal Tversky + focal CE) + weighted Dice + the batch variance of the softmax ("TV") + the boundary-weighted label
// distance, as a map logits, labels, boundary weights -> loss, aux, dlogits beside mrirt_inr_loss / mrirt_inr_loss_ext.
//   unified_partial_kernel   per-point clipped and plain softmax, argmax -> per-block fp64 sums
//   unified_final_kernel     totals in block order -> loss, aux, the gradient's coefficient row
//   unified_grad_kernel      the exact derivative: the pc paths through the Jacobian over the clipped logits, TV through the plain one
//   field_gather_kernel      mrirt_inr_sample_field: a per-voxel field at the voxels the samplers draw
// No float atomics, no label indexes memory, every sum over the batch is fp64 in a fixed order.  A row that holds a logit
// which is not finite takes no part: it adds nothing to any sum and its gradient row is +0 (n stays the divisor).
#include "inr_device.h"
#include "inr_unified.h"
#include "mrirt_host.h"

namespace mrirt {

struct UnifiedArgs {
    const float* logits;
    const int32_t* labels;
    const float* bw;                 // NULL: no boundary term
    int64_t n;
    uint32_t C;
    float cw[kLossMaxClasses];
    float gamma, lambda, alpha, beta;
    float uflW, diceW, tvW, bdW;
    double* sums;                    // [blocks][kUnVals], the totals, the coefficients
    uint32_t blocks;
    float* loss;
    float* aux;
    float* dlogits;
};

// What both passes need of one point: pc (clipped softmax of the clipped logits), ps (that softmax before its clip), pu
// (softmax of the logits as they are), the first index of the largest logit; false for a row with a non-finite logit.
struct UnPoint {
    float ps[kLossMaxClasses], pc[kLossMaxClasses], pu[kLossMaxClasses];
    uint32_t am;
};
__device__ __forceinline__ bool unified_point(const float* z, uint32_t C, UnPoint& r) {
    float zc[kLossMaxClasses], d[kLossMaxClasses];
    bool fin = true;
    float best = z[0];
    r.am = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        zc[k] = 0.0f;
        if (k < C) {
            const float v = z[k];
            fin = fin && isfinite(v);
            if (v > best) { best = v; r.am = k; }
            zc[k] = fminf(fmaxf(v, -kUnLogitClip), kUnLogitClip);
        }
    }
    if (!fin) return false;
    point_softmax(zc, C, r.ps, d);
    point_softmax(z, C, r.pu, d);
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) r.pc[k] = k < C ? fminf(fmaxf(r.ps[k], kUnProbLo), kUnProbHi) : 0.0f;
    return true;
}

__global__ __launch_bounds__(kLossThreads) void unified_partial_kernel(UnifiedArgs a) {
    __shared__ double part[kLossThreads / 64][kUnVals];
    double acc[kUnVals];
#pragma unroll
    for (uint32_t v = 0; v < kUnVals; ++v) acc[v] = 0.0;
    for (int64_t i = unified_first(blockIdx.x, threadIdx.x); i < a.n; i += unified_stride(a.blocks)) {
        UnPoint r;
        if (!unified_point(a.logits + unified_logit_index(i, a.C, 0), a.C, r)) continue;
        const int32_t label = a.labels[i];
        const int32_t y = label >= 0 && label < (int32_t)a.C ? label : -1;      // pc and pu are 0 from class C on: only the hit needs the range
        float q = 0.0f;
        bool in = false;
#pragma unroll
        for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
            const bool hit = (int32_t)k == y;
            acc[kUnP + k] += (double)r.pc[k];
            acc[kUnA + k] += hit ? (double)r.pc[k] : 0.0;
            acc[kUnT + k] += hit ? 1.0 : 0.0;
            acc[kUnS + k] += (double)r.pu[k];
            acc[kUnQ + k] += (double)r.pu[k] * (double)r.pu[k];
            if (hit) { q = r.pc[k]; in = true; }
        }
        if (in) acc[kUnFL] += (double)(powf((1.0f - q) + 1e-7f, a.gamma) * -logf(q + 1e-10f));
        const int64_t dist = (int64_t)r.am - (int64_t)label;
        if (a.bw) acc[kUnBd] += (double)a.bw[i] * (double)(dist < 0 ? -dist : dist);
        acc[kUnAcc] += dist == 0 ? 1.0 : 0.0;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t v = 0; v < kUnVals; ++v) {
        const double s = wave_sum(acc[v]);
        if (lane == 0) part[wave][v] = s;
    }
    __syncthreads();
    if (threadIdx.x < kUnVals) {
        double s = 0.0;
        for (uint32_t w = 0; w < kLossThreads / 64; ++w) s += part[w][threadIdx.x];
        a.sums[unified_sum_index(blockIdx.x, threadIdx.x)] = s;
    }
}

// totals in block order; thread k < C then forms class k's Tversky and Dice terms, thread 0 the loss, aux and the scalar coefficients
__global__ __launch_bounds__(kUnFinalThreads) void unified_final_kernel(UnifiedArgs a) {
    __shared__ double tot[kUnVals];
    __shared__ double ftl[kLossMaxClasses], dftl[kLossMaxClasses], dice[kLossMaxClasses];
    __shared__ double gates[2];                          // the two scalar clips: ufl, dl
    if (threadIdx.x < kUnVals) {
        double s = 0.0;
        for (uint32_t b = 0; b < a.blocks; ++b) s += a.sums[unified_sum_index(b, threadIdx.x)];
        tot[threadIdx.x] = s;
        a.sums[unified_sum_index(a.blocks, threadIdx.x)] = s;
    }
    __syncthreads();
    const uint32_t k = threadIdx.x;
    const double al = (double)a.alpha, be = (double)a.beta, ig = 1.0 / (double)a.gamma;
    double tiA = 0.0, tiP = 0.0, den = 1.0;
    if (k < a.C) {
        const double A = tot[kUnA + k], P = tot[kUnP + k], T = tot[kUnT + k];
        const double D = A + al * (P - A) + be * (T - A) + 1e-7;
        const double ti = A / D;
        const bool open = ti >= 0.0 && ti <= 1.0;
        const double base = 1.0 - (ti < 0.0 ? 0.0 : ti > 1.0 ? 1.0 : ti) + 1e-7;
        ftl[k] = pow(base, ig);
        dftl[k] = open ? -ig * pow(base, ig - 1.0) : 0.0;
        tiA = (D - A * (1.0 - al - be)) / (D * D);      // dTI/dA and dTI/dP with fp = P - A, fn = T - A
        tiP = -A * al / (D * D);
        den = P + T + 1.0;
        dice[k] = (2.0 * A + 1.0) / den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)a.n, lam = (double)a.lambda;
        double mftl = 0.0, wd = 0.0, ws = 0.0, tv = 0.0, tum = 0.0;
        for (uint32_t c = 0; c < a.C; ++c) {
            mftl += ftl[c];
            wd += dice[c] * (double)a.cw[c];
            ws += (double)a.cw[c];
            const double m = tot[kUnS + c] / n;
            tv += tot[kUnQ + c] / n - m * m;
            if (c >= 1) tum += dice[c];
            a.aux[kUnAux + c] = (float)dice[c];
        }
        mftl /= (double)a.C;
        const double mfl = tot[kUnFL] / n;
        const double uflRaw = lam * mftl + (1.0 - lam) * mfl, dlRaw = 1.0 - wd / (ws + 1e-10);
        const double ufl = uflRaw < 0.0 ? 0.0 : uflRaw > 1e6 ? 1e6 : uflRaw;
        const double dl = dlRaw < 0.0 ? 0.0 : dlRaw > 10.0 ? 10.0 : dlRaw;
        const double bl = tot[kUnBd] / n;
        gates[0] = uflRaw >= 0.0 && uflRaw <= 1e6 ? 1.0 : 0.0;
        gates[1] = dlRaw >= 0.0 && dlRaw <= 10.0 ? 1.0 / (ws + 1e-10) : 0.0;
        a.loss[0] = (float)((double)a.uflW * ufl + (double)a.diceW * dl + (double)a.tvW * tv + (double)a.bdW * bl);
        a.aux[0] = (float)ufl; a.aux[1] = (float)mftl; a.aux[2] = (float)mfl; a.aux[3] = (float)dl; a.aux[4] = (float)tv;
        a.aux[5] = (float)bl;
        a.aux[6] = a.C > 1 ? (float)(tum / (double)(a.C - 1)) : 0.0f;
        a.aux[7] = (float)(tot[kUnAcc] / n);
        a.sums[unified_sum_index(a.blocks + 1, kUnFocal)] = (double)(float)((double)a.uflW * gates[0] * (1.0 - lam) / n);
        a.sums[unified_sum_index(a.blocks + 1, kUnTv)] = (double)(float)(2.0 * (double)a.tvW / n);
    }
    __syncthreads();
    if (k < a.C) {
        const double cT = (double)a.uflW * gates[0] * (double)a.lambda / (double)a.C * dftl[k];
        const double cD = -(double)a.diceW * gates[1] * (double)a.cw[k];
        a.sums[unified_sum_index(a.blocks + 1, kUnGP + k)] = (double)(float)(cT * tiP - cD * dice[k] / den);
        a.sums[unified_sum_index(a.blocks + 1, kUnGA + k)] = (double)(float)(cT * tiA + cD * 2.0 / den);
        a.sums[unified_sum_index(a.blocks + 1, kUnMean + k)] = (double)(float)(tot[kUnS + k] / (double)a.n);
    }
}

// dloss/dz_j = [|z_j| <= 10] ps_j (G_j - sum_k G_k ps_k) + pu_j (V_j - sum_k V_k pu_k), with
//   G_k = [1e-7 <= ps_k <= 1 - 1e-7] (GP_k + t_k (GA_k + focal df/dq))      the pc paths: Tversky, Dice, focal CE
//   V_k = (2 tvWeight / n) (pu_k - S_k / n)                                 the batch variance
__global__ __launch_bounds__(kLossThreads) void unified_grad_kernel(UnifiedArgs a) {
    __shared__ float co[kUnCoefs];
    if (threadIdx.x < kUnCoefs) co[threadIdx.x] = (float)a.sums[unified_sum_index(a.blocks + 1, threadIdx.x)];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (i >= a.n) return;
    const float* z = a.logits + unified_logit_index(i, a.C, 0);
    float* out = a.dlogits + unified_logit_index(i, a.C, 0);
    UnPoint r;
    if (!unified_point(z, a.C, r)) {
        for (uint32_t k = 0; k < a.C; ++k) out[k] = 0.0f;
        return;
    }
    const int32_t label = a.labels[i];
    float G[kLossMaxClasses], V[kLossMaxClasses], gdot = 0.0f, vdot = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        G[k] = 0.0f; V[k] = 0.0f;
        if (k >= a.C) continue;
        const bool hit = (int32_t)k == label;
        float g = co[kUnGP + k];
        if (hit) {
            const float q = r.pc[k], base = (1.0f - q) + 1e-7f, nl = -logf(q + 1e-10f);
            const float df = -(a.gamma * powf(base, a.gamma - 1.0f)) * nl - powf(base, a.gamma) / (q + 1e-10f);
            g += co[kUnGA + k] + co[kUnFocal] * df;
        }
        G[k] = (r.ps[k] >= kUnProbLo && r.ps[k] <= kUnProbHi) ? g : 0.0f;
        V[k] = co[kUnTv] * (r.pu[k] - co[kUnMean + k]);
        gdot += G[k] * r.ps[k];
        vdot += V[k] * r.pu[k];
    }
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        if (k >= a.C) continue;
        const bool open = z[k] >= -kUnLogitClip && z[k] <= kUnLogitClip;
        const float viaC = open ? r.ps[k] * (G[k] - gdot) : 0.0f;
        out[k] = viaC + r.pu[k] * (V[k] - vdot);
    }
}

struct FieldArgs {
    const float* const* fields;
    uint32_t ncases, H, W, D;
    int64_t hwd;
    uint64_t seed, batch;
    int64_t n, nTumour;
    const uint32_t* index;
    const int64_t* offsets;
    float* out;
};

__global__ __launch_bounds__(kOptThreads) void field_gather_kernel(FieldArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (i >= a.n) return;
    const FieldVoxel f = field_voxel(a.seed, a.batch, (uint32_t)i, a.nTumour, a.ncases, a.H, a.W, a.D, a.hwd, a.index, a.offsets);
    a.out[i] = a.fields[f.cs][f.voxel];
}

static bool un_weight(float v) { return isfinite(v) && v >= 0.0f; }

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_unified_loss_scratch_bytes(int64_t n) {
    return (n < 1 || n >= (1ll << 31)) ? 0 : (int64_t)unified_scratch_bytes(n);
}

extern "C" int mrirt_unified_loss(const float* logits, const int32_t* labels, const float* boundary_w, int64_t n, uint32_t num_classes,
                                  const MrirtUnifiedLoss* cfg, float* loss, float* aux, float* dlogits, void* scratch, int64_t scratch_bytes,
                                  void* stream) {
    if (!logits || !labels || !cfg || !loss || !aux || !scratch) return MRIRT_ERR_NULL;
    if (n < 1 || n >= (1ll << 31)) return MRIRT_ERR_ARG;
    if (num_classes < 1 || num_classes > kLossMaxClasses) return MRIRT_ERR_ARG;
    if (!(cfg->gamma >= 0.25f && cfg->gamma <= 1.0f) || !(cfg->lambda >= 0.0f && cfg->lambda <= 1.0f)) return MRIRT_ERR_ARG;      // NaN fails both
    if (!un_weight(cfg->tverskyAlpha) || !un_weight(cfg->tverskyBeta) || !un_weight(cfg->uflWeight) || !un_weight(cfg->diceWeight) ||
        !un_weight(cfg->tvWeight) || !un_weight(cfg->boundaryWeight)) return MRIRT_ERR_ARG;
    for (uint32_t k = 0; k < num_classes; ++k)
        if (!un_weight(cfg->classWeights[k])) return MRIRT_ERR_ARG;
    if (cfg->flags != 0u) return MRIRT_ERR_ARG;
    const int rc = check_scratch(scratch, scratch_bytes, unified_scratch_bytes(n));
    if (rc != MRIRT_OK) return rc;
    UnifiedArgs a = {};
    a.logits = logits; a.labels = labels; a.bw = boundary_w; a.n = n; a.C = num_classes;
    for (uint32_t k = 0; k < num_classes; ++k) a.cw[k] = cfg->classWeights[k];
    a.gamma = cfg->gamma; a.lambda = cfg->lambda; a.alpha = cfg->tverskyAlpha; a.beta = cfg->tverskyBeta;
    a.uflW = cfg->uflWeight; a.diceW = cfg->diceWeight; a.tvW = cfg->tvWeight; a.bdW = cfg->boundaryWeight;
    a.sums = (double*)scratch; a.blocks = loss_blocks(n);
    a.loss = loss; a.aux = aux; a.dlogits = dlogits;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(unified_partial_kernel, dim3(a.blocks), dim3(kLossThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(unified_final_kernel, dim3(1), dim3(kUnFinalThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    if (dlogits) {
        hipLaunchKernelGGL(unified_grad_kernel, dim3(unified_grad_blocks(n)), dim3(kLossThreads), 0, s, a);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}

extern "C" int mrirt_inr_sample_field(const MrirtInrCache* cache, const MrirtInrTumourIndex* tumour, const float* const* fields, uint64_t seed,
                                      uint64_t batch_index, int64_t n, int64_t n_tumour, float* out, void* stream) {
    if (!cache || !fields || !out) return MRIRT_ERR_NULL;
    const int rc = opt_check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    if (n < 1 || n >= (1ll << 31) || n_tumour < 0 || n_tumour > n) return MRIRT_ERR_ARG;
    if (n_tumour > 0 && (!tumour || !tumour->index || !tumour->offsets)) return MRIRT_ERR_NULL;
    FieldArgs a = {};
    a.fields = fields; a.ncases = cache->ncases;
    a.H = cache->hwd[0]; a.W = cache->hwd[1]; a.D = cache->hwd[2];
    a.hwd = (int64_t)a.H * a.W * a.D;
    a.seed = seed; a.batch = batch_index; a.n = n; a.nTumour = n_tumour;
    if (n_tumour > 0) { a.index = tumour->index; a.offsets = tumour->offsets; }
    a.out = out;
    hipLaunchKernelGGL(field_gather_kernel, dim3((uint32_t)((n + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, (hipStream_t)stream, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
