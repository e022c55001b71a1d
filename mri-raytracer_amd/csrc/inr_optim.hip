// INR training loop (inr/inr/train.py:18-259): what surrounds the training step of csrc/inr_train.hip.
//   sample_kernel          one micro-batch of voxels from a device-resident multi-case cache, drawn with Philox4x32-10 from
//                          (seed, micro-batch index, point index) alone: no generator state lives anywhere
//   sqnorm_partial_kernel  the global gradient norm in fp64: per-block sums in a fixed grid-stride assignment ...
//   sqnorm_final_kernel    ... added in block order; writes the norm and the clip factor s next to it
//   adamw_kernel           clip + AdamW on weights and biases in one launch; reads s from the device
//   mrirt_inr_train_run    enqueues whole optimiser steps (accum x (sample, forward, loss, backward), one update) through the
//                          same entry points a caller would use one by one: no host synchronisation, no allocation
//   mrirt_inr_train_run_muon  the same run with mrirt_muon_step (csrc/inr_muon.hip) as the update; that step borrows the norm
//                          pass and the bias update from here (opt_norm_and_bias_step)
// No float atomics and no data-dependent order anywhere: the same inputs give the same bits.
#include "inr_device.h"
#include "mrirt_host.h"

namespace mrirt {

struct SampleArgs {
    const float* const* mods;
    const int16_t* const* seg;
    uint32_t ncases, M, H, W, D;
    int64_t hwd;
    uint64_t seed, batch;
    int64_t n;
    float* coords;
    float* feats;
    int32_t* labels;
};

// One thread per point: the draw stays in registers, then M + 1 dependent gathers.  Neighbouring threads write neighbouring
// rows of coords / feats / labels.
__global__ __launch_bounds__(kOptThreads) void sample_kernel(SampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (i >= a.n) return;
    const SamplePoint p = sample_point(a.seed, a.batch, (uint32_t)i, a.ncases, a.H, a.W, a.D);
    sample_write(i, p, a.mods, a.seg, a.M, a.H, a.W, a.D, a.hwd, a.coords, a.feats, a.labels);
}

struct OptArgs {
    float *w, *b, *muW, *muB, *nuW, *nuB;
    const float *gw, *gb;
    int64_t nw, nb;
    OptUnits units;
    float gscale, lr, b1, b2, omb1, omb2, c1, c2, eps, wd;
    double clip;                 // <= 0: no clipping
    double* partial;             // [blocks]
    uint32_t blocks;
    double* gnorm;               // [0] norm, [1] s
};

__global__ __launch_bounds__(kOptThreads) void sqnorm_partial_kernel(OptArgs a) {
    __shared__ double part[kOptThreads / 64];
    const int64_t n = a.nw + a.nb;
    double acc = 0.0;
    for (int64_t i = opt_first(blockIdx.x, threadIdx.x); i < n; i += opt_stride(a.blocks)) {
        const float g = (i < a.nw ? a.gw[i] : a.gb[i - a.nw]) * a.gscale;
        acc += (double)g * (double)g;
    }
    const double s = wave_sum(acc);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (uint32_t w = 0; w < kOptThreads / 64; ++w) t += part[w];
        a.partial[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void sqnorm_final_kernel(OptArgs a) {
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (uint32_t b = 0; b < a.blocks; ++b) t += a.partial[b];
    const double norm = sqrt(t);
    double s = 1.0;
    if (a.clip > 0.0) s = isfinite(norm) ? (norm < a.clip ? 1.0 : a.clip / norm) : __builtin_nan("");
    a.gnorm[0] = norm;
    a.gnorm[1] = (double)(float)s;
}

__device__ __forceinline__ void adamw_one(const OptArgs& a, float s, float g, float& p, float& mu, float& nu) {
    const float gc = (g * a.gscale) * s;
    mu = a.b1 * mu + a.omb1 * gc;
    nu = a.b2 * nu + (a.omb2 * gc) * gc;
    const float mh = mu / a.c1, nh = nu / a.c2;
    const float upd = mh / (sqrtf(nh) + a.eps) + a.wd * p;
    p = p - a.lr * upd;
}

__global__ __launch_bounds__(kOptThreads) void adamw_kernel(OptArgs a) {
    const int64_t u = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (u >= opt_unit_count(a.units)) return;
    const float s = (float)a.gnorm[1];
    uint32_t seg, width;
    int64_t first;
    opt_unit(a.units, u, seg, first, width);
    float* p = (seg ? a.b : a.w) + first;
    float* mu = (seg ? a.muB : a.muW) + first;
    float* nu = (seg ? a.nuB : a.nuW) + first;
    const float* g = (seg ? a.gb : a.gw) + first;
    if (width == 4) {
        float4 pv = *(float4*)p, mv = *(float4*)mu, nv = *(float4*)nu;
        const float4 gv = *(const float4*)g;
        adamw_one(a, s, gv.x, pv.x, mv.x, nv.x);
        adamw_one(a, s, gv.y, pv.y, mv.y, nv.y);
        adamw_one(a, s, gv.z, pv.z, mv.z, nv.z);
        adamw_one(a, s, gv.w, pv.w, mv.w, nv.w);
        *(float4*)p = pv; *(float4*)mu = mv; *(float4*)nu = nv;
    } else {
        float pv = *p, mv = *mu, nv = *nu;
        adamw_one(a, s, *g, pv, mv, nv);
        *p = pv; *mu = mv; *nu = nv;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

static int check_cache(const MrirtInrCache* c) {
    if (!c || !c->seg || (c->numMods > 0 && !c->mods)) return MRIRT_ERR_NULL;
    if (c->hwd[0] < 2 || c->hwd[1] < 2 || c->hwd[2] < 2) return MRIRT_ERR_DIMS;
    if ((uint64_t)c->hwd[0] * c->hwd[1] >= (1ull << 31) || (uint64_t)c->hwd[0] * c->hwd[1] * c->hwd[2] >= (1ull << 31)) return MRIRT_ERR_DIMS;
    if (c->ncases < 1 || c->ncases > kCacheMaxCases || c->numMods > kCacheMaxMods) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

static bool finite_f(float v) { return isfinite(v); }

static int check_adamw(const MrirtAdamW* hp, bool needLr) {
    if (!hp) return MRIRT_ERR_NULL;
    if ((needLr && !finite_f(hp->lr)) || !finite_f(hp->b1) || !finite_f(hp->b2) || !finite_f(hp->eps) || !finite_f(hp->weightDecay)) return MRIRT_ERR_ARG;
    if (hp->b1 < 0.0f || hp->b1 >= 1.0f || hp->b2 < 0.0f || hp->b2 >= 1.0f || !(hp->eps > 0.0f)) return MRIRT_ERR_ARG;
    if (hp->clipNorm != hp->clipNorm || hp->clipNorm == -INFINITY) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the arguments of one update: the norm runs over [gw | gb] (nw + nb elements), the update over the first nwUpdate weights
// (all of them, or none) and every bias
static OptArgs opt_args(float* w, float* b, const float* gw, const float* gb, float* mu_w, float* mu_b, float* nu_w, float* nu_b,
                        int64_t nw, int64_t nb, int64_t nwUpdate, const MrirtAdamW* hp, uint64_t t, float gscale, double* gnorm, void* scratch) {
    OptArgs a = {};
    a.w = w; a.b = b; a.muW = mu_w; a.muB = mu_b; a.nuW = nu_w; a.nuB = nu_b; a.gw = gw; a.gb = gb;
    a.nw = nw; a.nb = nb;
    a.units = opt_units(nwUpdate, nb, aligned16(w) && aligned16(gw) && aligned16(mu_w) && aligned16(nu_w),
                        aligned16(b) && aligned16(gb) && aligned16(mu_b) && aligned16(nu_b));
    const double b1 = (double)hp->b1, b2 = (double)hp->b2, tp = (double)t + 1.0;
    a.gscale = gscale; a.lr = hp->lr; a.b1 = hp->b1; a.b2 = hp->b2; a.eps = hp->eps; a.wd = hp->weightDecay;
    a.omb1 = (float)(1.0 - b1); a.omb2 = (float)(1.0 - b2);
    a.c1 = (float)(1.0 - pow(b1, tp)); a.c2 = (float)(1.0 - pow(b2, tp));
    a.clip = (hp->clipNorm > 0.0f && isfinite(hp->clipNorm)) ? (double)hp->clipNorm : 0.0;
    a.partial = (double*)scratch; a.blocks = opt_blocks(nw + nb);
    a.gnorm = gnorm;
    return a;
}

static int launch_norm(const OptArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(a.blocks), dim3(kOptThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(64), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

static int launch_adamw(const OptArgs& a, hipStream_t s) {
    const int64_t units = opt_unit_count(a.units);
    if (units < 1) return MRIRT_OK;
    hipLaunchKernelGGL(adamw_kernel, dim3((uint32_t)((units + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

int opt_check_adamw(const MrirtAdamW* hp, bool needLr) { return check_adamw(hp, needLr); }
int opt_check_cache(const MrirtInrCache* cache) { return check_cache(cache); }

int opt_norm_and_bias_step(const float* gw, int64_t nw, float* b, const float* gb, float* mu_b, float* nu_b, int64_t nb,
                           const MrirtAdamW* hp, uint64_t t, float gscale, double* gnorm, void* scratch, hipStream_t stream) {
    const OptArgs a = opt_args(nullptr, b, gw, gb, nullptr, mu_b, nullptr, nu_b, nw, nb, 0, hp, t, gscale, gnorm, scratch);
    const int rc = launch_norm(a, stream);
    return rc != MRIRT_OK ? rc : launch_adamw(a, stream);
}

// the shapes, the cache and the configuration of a run; fills the layouts
static int check_run(const MrirtInrDesc* desc, bool siren, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg, TrainLayout& L, RunLayout& R) {
    if (!desc || !cache || !cfg) return MRIRT_ERR_NULL;
    int rc = check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    if (desc->kind != (siren ? MRIRT_INR_SIREN : MRIRT_INR_FOURIER_RELU) || desc->numMods != cache->numMods) return MRIRT_ERR_ARG;
    if (cfg->microBatch < 1 || cfg->microBatch >= (1ll << 31) || cfg->accum < 1) return MRIRT_ERR_ARG;
    const int64_t stepBytes = siren ? mrirt_siren_train_scratch_bytes(desc, cfg->microBatch) : mrirt_inr_train_scratch_bytes(desc, cfg->microBatch);
    if (stepBytes <= 0) return MRIRT_ERR_ARG;
    if (desc->outDim < 1 || desc->outDim > kLossMaxClasses || !isfinite(cfg->diceWeight)) return MRIRT_ERR_ARG;
    for (uint32_t k = 0; k < desc->outDim; ++k)
        if (!isfinite(cfg->classWeights[k])) return MRIRT_ERR_ARG;
    if ((rc = check_adamw(&cfg->adamw, false)) != MRIRT_OK) return rc;
    double lr;
    if ((rc = mrirt_inr_lr_schedule(cfg->peakLr, cfg->minLr, cfg->warmupSteps, cfg->decaySteps, 0, &lr)) != MRIRT_OK) return rc;
    L = train_layout(desc->numLayers, desc->inDim, desc->hidden, desc->outDim, cfg->microBatch);
    L.bytes = (uint64_t)stepBytes;                       // the SIREN step's scratch carries the cosines behind the ReLU step's
    R = run_layout(L, cfg->microBatch, cache->numMods);
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_inr_sample_batch(const MrirtInrCache* cache, uint64_t seed, uint64_t batch_index, int64_t n, float* coords,
                                      float* feats, int32_t* labels, void* stream) {
    if (!cache || !coords || !labels) return MRIRT_ERR_NULL;
    const int rc = check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    if (cache->numMods > 0 && !feats) return MRIRT_ERR_NULL;
    if (n < 1 || n >= (1ll << 31)) return MRIRT_ERR_ARG;
    SampleArgs a = {};
    a.mods = cache->mods; a.seg = cache->seg; a.ncases = cache->ncases; a.M = cache->numMods;
    a.H = cache->hwd[0]; a.W = cache->hwd[1]; a.D = cache->hwd[2];
    a.hwd = (int64_t)a.H * a.W * a.D;
    a.seed = seed; a.batch = batch_index; a.n = n;
    a.coords = coords; a.feats = feats; a.labels = labels;
    hipLaunchKernelGGL(sample_kernel, dim3((uint32_t)((n + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, (hipStream_t)stream, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int64_t mrirt_inr_adamw_scratch_bytes(int64_t n) {
    return (n < 1 || n >= (1ll << 31)) ? 0 : (int64_t)opt_scratch_bytes(n);
}

extern "C" int mrirt_inr_adamw_step(float* w, float* b, const float* gw, const float* gb, float* mu_w, float* mu_b, float* nu_w,
                                    float* nu_b, int64_t nw, int64_t nb, const MrirtAdamW* hp, uint64_t t, float gscale,
                                    double* gnorm, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!w || !gw || !mu_w || !nu_w || !hp || !gnorm) return MRIRT_ERR_NULL;
    if (nw < 1 || nb < 0 || nw >= (1ll << 31) || nb >= (1ll << 31) || nw + nb >= (1ll << 31)) return MRIRT_ERR_ARG;
    if (nb > 0 && (!b || !gb || !mu_b || !nu_b)) return MRIRT_ERR_NULL;
    int rc = check_adamw(hp, true);
    if (rc != MRIRT_OK) return rc;
    if (!isfinite(gscale) || ((uintptr_t)gnorm & 7u) != 0) return MRIRT_ERR_ARG;
    if ((rc = check_scratch(scratch, scratch_bytes, opt_scratch_bytes(nw + nb))) != MRIRT_OK) return rc;
    const OptArgs a = opt_args(w, b, gw, gb, mu_w, mu_b, nu_w, nu_b, nw, nb, nw, hp, t, gscale, gnorm, scratch);
    if ((rc = launch_norm(a, (hipStream_t)stream)) != MRIRT_OK) return rc;
    return launch_adamw(a, (hipStream_t)stream);
}

extern "C" int mrirt_inr_lr_schedule(double peak, double end, uint32_t warmup, uint32_t decay_steps, uint64_t t, double* lr) {
    if (!lr) return MRIRT_ERR_NULL;
    if (!isfinite(peak) || !isfinite(end) || !(peak > 0.0) || end < 0.0) return MRIRT_ERR_ARG;
    const int64_t T = (int64_t)decay_steps - (int64_t)warmup;
    if (T <= 0) return MRIRT_ERR_ARG;
    if (t < warmup) { *lr = peak * (double)t / (double)warmup; return MRIRT_OK; }
    const uint64_t past = t - warmup;
    const double u = (double)(past < (uint64_t)T ? past : (uint64_t)T) / (double)T;
    const double alpha = end / peak;
    *lr = peak * ((1.0 - alpha) * (0.5 * (1.0 + cos(3.141592653589793 * u))) + alpha);
    return MRIRT_OK;
}

static int64_t run_scratch_bytes(const MrirtInrDesc* desc, bool siren, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg) {
    TrainLayout L;
    RunLayout R;
    return check_run(desc, siren, cache, cfg, L, R) == MRIRT_OK ? (int64_t)R.bytes : 0;
}

// a Muon run's scratch: the AdamW run's, then mrirt_muon_step's
extern "C" int64_t mrirt_inr_train_run_muon_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg) {
    if (!desc) return 0;
    const int64_t run = run_scratch_bytes(desc, desc->kind == MRIRT_INR_SIREN, cache, cfg), step = mrirt_muon_scratch_bytes(desc);
    return run > 0 && step > 0 ? run + step : 0;
}

extern "C" int64_t mrirt_inr_train_run_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg) {
    return run_scratch_bytes(desc, false, cache, cfg);
}
extern "C" int64_t mrirt_siren_train_run_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg) {
    return run_scratch_bytes(desc, true, cache, cfg);
}

// mrirt_inr_train_run_ext's extras: the loss and the sampler of csrc/inr_lossx.hip.  All NULL / 0: the plain run.
struct RunExtras {
    const MrirtInrLossExt* loss;
    MrirtInrTumourIndex tumour;
    int64_t nTumour;
};

// what mrirt_inr_loss_ext / mrirt_inr_sample_batch_mix would refuse of the extras, before any launch
static int check_extras(const RunExtras& x, const MrirtInrDesc* desc, const MrirtInrTrainCfg* cfg) {
    if (x.loss) {
        const int rc = lossx_check(x.loss, desc->outDim);
        if (rc != MRIRT_OK) return rc;
    }
    if (x.nTumour < 0 || x.nTumour > cfg->microBatch) return MRIRT_ERR_ARG;
    if (x.nTumour > 0 && (!x.tumour.index || !x.tumour.offsets)) return MRIRT_ERR_NULL;
    return MRIRT_OK;
}

// One loop for both families: the kind picks the public forward / backward pair, everything else is shared.
// muon: NULL for AdamW; else the update is mrirt_muon_step, whose scratch lies behind the AdamW run's.
// extras: NULL for the plain run; else its loss (whose scratch lies behind Muon's) and / or its sampler replace the plain ones.
static int train_run(const MrirtInrDesc* desc, bool siren, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                     const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history,
                     void* scratch, int64_t scratch_bytes, void* stream, const MrirtMuon* muon = nullptr,
                     const RunExtras* extras = nullptr) {
    TrainLayout L;
    RunLayout R;
    if (!desc || !cache || !cfg || !state || !history) return MRIRT_ERR_NULL;
    if (!state->w || !state->b || !state->mu_w || !state->mu_b || !state->nu_w || !state->nu_b) return MRIRT_ERR_NULL;
    int rc = check_run(desc, siren, cache, cfg, L, R);
    if (rc != MRIRT_OK) return rc;
    if (steps < 1) return MRIRT_ERR_ARG;
    const int64_t muonBytes = muon ? mrirt_muon_scratch_bytes(desc) : 0;
    if (muon) {                                          // what mrirt_muon_step would refuse, before any launch
        if ((rc = muon_check_hp(muon)) != MRIRT_OK) return rc;
        if (muonBytes <= 0) return MRIRT_ERR_ARG;
    }
    if (extras && (rc = check_extras(*extras, desc, cfg)) != MRIRT_OK) return rc;
    const MrirtInrLossExt* lossExt = extras ? extras->loss : nullptr;
    const bool mix = extras && extras->nTumour > 0;
    const int64_t lossBytes = lossExt ? mrirt_inr_loss_ext_scratch_bytes(cfg->microBatch) : 0;
    if ((rc = check_scratch(scratch, scratch_bytes, R.bytes + (uint64_t)muonBytes + (uint64_t)lossBytes)) != MRIRT_OK) return rc;
    const int64_t n = cfg->microBatch;
    const uint32_t C = desc->outDim;
    char* base = (char*)scratch;
    float* coords = (float*)(base + R.offCoords);
    float* feats = cache->numMods ? (float*)(base + R.offFeats) : nullptr;
    int32_t* labels = (int32_t*)(base + R.offLabels);
    float* logits = (float*)(base + R.offLogits);
    float* dlogits = (float*)(base + R.offDlogits);
    float* gw = (float*)(base + R.offGw);
    float* gb = (float*)(base + R.offGb);
    double* gnorm = (double*)(base + R.offGnorm);
    MrirtAdamW hp = cfg->adamw;
    const float gscale = 1.0f / (float)cfg->accum;
    for (uint32_t k = 0; k < steps; ++k) {
        const uint64_t t = first_step + k;
        for (uint32_t a = 0; a < cfg->accum; ++a) {
            float* h = history + ((uint64_t)k * cfg->accum + a) * (1u + 2u * C);
            if (mix) rc = mrirt_inr_sample_batch_mix(cache, &extras->tumour, cfg->seed, t * cfg->accum + a, n, extras->nTumour, coords, feats, labels, stream);
            else rc = mrirt_inr_sample_batch(cache, cfg->seed, t * cfg->accum + a, n, coords, feats, labels, stream);
            if (rc != MRIRT_OK) return rc;
            if ((rc = (siren ? mrirt_siren_forward_f32 : mrirt_inr_forward_f32)(desc, state->w, state->b, coords, feats, n, logits, base, (int64_t)R.stepBytes, stream)) != MRIRT_OK) return rc;
            if (lossExt) rc = mrirt_inr_loss_ext(logits, labels, n, C, lossExt, h, h + 1, nullptr, dlogits, base + R.bytes + muonBytes, lossBytes, stream);
            else rc = mrirt_inr_loss(logits, labels, n, C, cfg->classWeights, cfg->diceWeight, h, h + 1, dlogits, base, (int64_t)R.stepBytes, stream);
            if (rc != MRIRT_OK) return rc;
            if ((rc = (siren ? mrirt_siren_backward : mrirt_inr_backward)(desc, state->w, n, dlogits, gw, gb, a ? 1u : 0u, base, (int64_t)R.stepBytes, stream)) != MRIRT_OK) return rc;
        }
        double lr;
        if ((rc = mrirt_inr_lr_schedule(cfg->peakLr, cfg->minLr, cfg->warmupSteps, cfg->decaySteps, t, &lr)) != MRIRT_OK) return rc;
        hp.lr = (float)lr;
        if (muon)
            rc = mrirt_muon_step(desc, state->w, state->b, gw, gb, state->mu_w, state->mu_b, state->nu_b, muon, &hp, t, gscale, gnorm,
                                 base + R.bytes, muonBytes, stream);
        else
            rc = mrirt_inr_adamw_step(state->w, state->b, gw, gb, state->mu_w, state->mu_b, state->nu_w, state->nu_b, (int64_t)R.nw,
                                      (int64_t)R.nb, &hp, t, gscale, gnorm, base + R.offOpt, (int64_t)R.optBytes, stream);
        if (rc != MRIRT_OK) return rc;
    }
    return MRIRT_OK;
}

extern "C" int mrirt_inr_train_run(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                                   const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history,
                                   void* scratch, int64_t scratch_bytes, void* stream) {
    return train_run(desc, false, cache, cfg, state, first_step, steps, history, scratch, scratch_bytes, stream);
}

extern "C" int mrirt_siren_train_run(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                                     const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history,
                                     void* scratch, int64_t scratch_bytes, void* stream) {
    return train_run(desc, true, cache, cfg, state, first_step, steps, history, scratch, scratch_bytes, stream);
}

extern "C" int mrirt_inr_train_run_muon(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg, const MrirtMuon* hp,
                                        const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history,
                                        void* scratch, int64_t scratch_bytes, void* stream) {
    if (!desc || !hp) return MRIRT_ERR_NULL;
    return train_run(desc, desc->kind == MRIRT_INR_SIREN, cache, cfg, state, first_step, steps, history, scratch, scratch_bytes, stream, hp);
}

static bool run_ext_kind(const MrirtInrDesc* desc, const MrirtInrTrainExt* ext, bool& siren, RunExtras& x) {
    if (!desc || !ext) return false;
    siren = desc->kind == MRIRT_INR_SIREN;
    x.loss = ext->loss; x.tumour = ext->tumour; x.nTumour = ext->nTumour;
    return true;
}

// the plain run's scratch, then mrirt_muon_step's (with muon), then mrirt_inr_loss_ext's (with loss)
extern "C" int64_t mrirt_inr_train_run_ext_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                                                         const MrirtInrTrainExt* ext) {
    bool siren;
    RunExtras x;
    if (!run_ext_kind(desc, ext, siren, x) || !cfg) return 0;
    const int64_t run = run_scratch_bytes(desc, siren, cache, cfg);
    if (run <= 0 || check_extras(x, desc, cfg) != MRIRT_OK) return 0;
    const int64_t step = ext->muon ? mrirt_muon_scratch_bytes(desc) : 0, loss = ext->loss ? mrirt_inr_loss_ext_scratch_bytes(cfg->microBatch) : 0;
    if ((ext->muon && (step <= 0 || muon_check_hp(ext->muon) != MRIRT_OK)) || (ext->loss && loss <= 0)) return 0;
    return run + step + loss;
}

extern "C" int mrirt_inr_train_run_ext(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                                       const MrirtInrTrainExt* ext, const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps,
                                       float* history, void* scratch, int64_t scratch_bytes, void* stream) {
    bool siren;
    RunExtras x;
    if (!run_ext_kind(desc, ext, siren, x)) return MRIRT_ERR_NULL;
    return train_run(desc, siren, cache, cfg, state, first_step, steps, history, scratch, scratch_bytes, stream, ext->muon, &x);
}
