// Muon for the INR training loop (Jordan et al. 2024; optax.contrib.muon's scale_by_muon with its defaults): momentum on every
// weight matrix, five Newton-Schulz iterations to orthogonalise it, AdamW on the biases.  DESIGN.md section 17.
//   muon_momentum_kernel   mu <- beta mu + (1 - beta) g';  m^ = the bias-corrected (Nesterov) momentum, element-wise
//   muon_norm_kernel       per layer, one block: the fp64 sum of squares of m^ in a fixed order -> ||m^||_F + eps
//   muon_scale_kernel      X = m^ / (||m^||_F + eps): fp64 divide, one rounding
//   muon_gemm_kernel       the three products of an iteration (A = X X^T;  B = c1 A + c2 A A;  X <- c0 X + B X) on the fp32 MFMA
//                          GEMM of inr_gemm.h, each launched once for ALL layers: blockIdx.z picks the layer from the table
//   muon_apply_kernel      W <- W - lr (scale O + wd W)
// The global-norm clip factor and the biases' AdamW are csrc/inr_optim.hip's own kernels (opt_norm_and_bias_step).
// No allocation, no host synchronisation, no float atomics, no workgroup waits for another: the same inputs give the same bits.
#include "inr_device.h"
#include "inr_gemm.h"
#include "inr_muon.h"
#include "mrirt_host.h"

namespace mrirt {

enum { kNsGram = 0, kNsPoly = 1, kNsUpdate = 2 };

struct MuonNsArgs {
    MuonPlan plan;
    const float* X;              // gram, update: the current iterate
    float* A;                    // gram writes it, poly reads it
    float* B;                    // poly writes it, update reads it
    float* Xn;                   // update: the next iterate
    float c0, c1, c2;
};

template <int WHICH, bool AKFAST, bool BKFAST>
__global__ __launch_bounds__(kTrThreads) void muon_gemm_kernel(MuonNsArgs a) {
    __shared__ float As[kTrBK * TrLds<kTrBM>::pitch];
    __shared__ float Bs[kTrBK * TrLds<kMuonBN>::pitch];
    constexpr int NT = kMuonBN / 16;
    const MuonLayer& y = a.plan.layer[blockIdx.z];
    const MuonGemm g = WHICH == kNsGram ? muon_gram_args(y, a.X, a.A) : WHICH == kNsPoly ? muon_poly_args(y, a.A, a.B)
                                                                                         : muon_update_args(y, a.B, a.X, a.Xn);
    const uint32_t m0 = blockIdx.x * kTrBM, n0 = blockIdx.y * kMuonBN;
    if (m0 >= g.M || n0 >= g.N) return;                  // the whole block: this layer has fewer tiles than the largest one
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    f32x4 acc[NT];
    gm_accumulate<kMuonBN, AKFAST, BKFAST>(g.A, g.B, m0, n0, 0, g.K, As, Bs, acc);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const uint32_t col = n0 + 16u * j + tr_acc_col(lane);
        if (col >= g.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = m0 + 16u * wave + tr_acc_row(lane, r);
            if (row >= g.M) continue;
            const int64_t at = (int64_t)row * g.cR + (int64_t)col * g.cC;
            const float v = acc[j][r];
            if (WHICH == kNsGram) g.C[at] = v;
            else if (WHICH == kNsPoly) g.C[at] = a.c1 * g.D[at] + a.c2 * v;
            else g.C[at] = a.c0 * g.D[at] + v;
        }
    }
}

// block l: thread t adds the squares of elements t, t + kMuonThreads, ... of layer l; the 64 lanes of a wave fold by halves,
// the four wave sums add in wave order
__global__ __launch_bounds__(kMuonThreads) void muon_norm_kernel(MuonPlan plan, const float* m, double eps, double* denom) {
    __shared__ double part[kMuonThreads / 64];
    const MuonLayer& y = plan.layer[blockIdx.x];
    const float* p = m + y.wOff;
    const int64_t n = (int64_t)y.in * y.out;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kMuonThreads) acc += (double)p[i] * (double)p[i];
    const double s = wave_sum(acc);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (uint32_t w = 0; w < kMuonThreads / 64; ++w) t += part[w];
        denom[blockIdx.x] = sqrt(t) + eps;
    }
}

__global__ __launch_bounds__(kMuonThreads) void muon_scale_kernel(MuonPlan plan, const float* m, const double* denom, float* X) {
    const int64_t i = (int64_t)blockIdx.x * kMuonThreads + threadIdx.x;
    if (i >= (int64_t)plan.nw) return;
    X[i] = (float)((double)m[i] / denom[muon_layer_of(plan, i)]);
}

struct MuonMomentumArgs {
    const float* gw;
    float *mu, *mhat;
    int64_t nw;
    const double* gnorm;         // [1]: the clip factor s
    float gscale, beta, omb, c1, c2;      // omb = 1 - beta;  c1 = 1 - beta^(t+1), c2 = 1 - beta^(t+2)
    uint32_t nesterov;
};

__global__ __launch_bounds__(kMuonThreads) void muon_momentum_kernel(MuonMomentumArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMuonThreads + threadIdx.x;
    if (i >= a.nw) return;
    const float s = (float)a.gnorm[1];
    const float gc = (a.gw[i] * a.gscale) * s;
    const float mu = a.beta * a.mu[i] + a.omb * gc;
    a.mu[i] = mu;
    a.mhat[i] = a.nesterov ? a.beta * (mu / a.c2) + a.omb * (gc / a.c1) : mu / a.c1;
}

__global__ __launch_bounds__(kMuonThreads) void muon_apply_kernel(MuonPlan plan, float* w, const float* O, float lr, float wd) {
    const int64_t i = (int64_t)blockIdx.x * kMuonThreads + threadIdx.x;
    if (i >= (int64_t)plan.nw) return;
    const float p = w[i];
    w[i] = p - lr * (plan.layer[muon_layer_of(plan, i)].scale * O[i] + wd * p);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

static int check_muon(const MrirtMuon* hp) {
    if (!hp) return MRIRT_ERR_NULL;
    if (!(hp->beta >= 0.0f && hp->beta < 1.0f)) return MRIRT_ERR_ARG;
    if (!(hp->eps > 0.0f) || !isfinite(hp->eps) || !isfinite(hp->weightDecay)) return MRIRT_ERR_ARG;
    for (int k = 0; k < 3; ++k)
        if (!isfinite(hp->nsCoeffs[k])) return MRIRT_ERR_ARG;
    if (hp->nsSteps < 1 || hp->nsSteps > kMuonMaxSteps || hp->nesterov > 1u) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

int muon_check_hp(const MrirtMuon* hp) { return check_muon(hp); }

// the network shapes either family of training entry points takes
static int muon_desc(const MrirtInrDesc* d, MuonPlan& P, MuonLayout& L) {
    if (!d) return MRIRT_ERR_NULL;
    if (mrirt_inr_train_scratch_bytes(d, 1) <= 0 && mrirt_siren_train_scratch_bytes(d, 1) <= 0) return MRIRT_ERR_ARG;
    if (d->numLayers < 1 || d->numLayers > (uint32_t)kTrMaxLayers) return MRIRT_ERR_ARG;
    P = muon_plan(d->numLayers, d->inDim, d->hidden, d->outDim);
    if (P.nw + P.nb >= (1ull << 31)) return MRIRT_ERR_ARG;
    L = muon_layout(P);
    return MRIRT_OK;
}

static uint32_t elem_blocks(uint64_t n) { return (uint32_t)((n + kMuonThreads - 1) / kMuonThreads); }

// m -> out through the Newton-Schulz part of the scratch; every argument has been checked
static int newton_schulz(const MuonPlan& P, const MuonLayout& L, const float* m, float* out, const MrirtMuon* hp, char* base, hipStream_t s) {
    double* denom = (double*)(base + L.offDenom);
    float* X[2] = { (float*)(base + L.offX0), (float*)(base + L.offX1) };
    hipLaunchKernelGGL(muon_norm_kernel, dim3(P.numLayers), dim3(kMuonThreads), 0, s, P, m, (double)hp->eps, denom);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(muon_scale_kernel, dim3(elem_blocks(P.nw)), dim3(kMuonThreads), 0, s, P, m, (const double*)denom, X[0]);
    MRIRT_HIP(hipGetLastError());
    MuonNsArgs a = {};
    a.plan = P;
    a.A = (float*)(base + L.offA); a.B = (float*)(base + L.offB);
    a.c0 = hp->nsCoeffs[0]; a.c1 = hp->nsCoeffs[1]; a.c2 = hp->nsCoeffs[2];
    const dim3 sq(muon_tiles(P.maxR, kTrBM), muon_tiles(P.maxR, kMuonBN), P.numLayers);
    const dim3 wide(muon_tiles(P.maxR, kTrBM), muon_tiles(P.maxC, kMuonBN), P.numLayers);
    for (uint32_t k = 0; k < hp->nsSteps; ++k) {
        a.X = X[k & 1u];
        a.Xn = k + 1 == hp->nsSteps ? out : X[(k + 1) & 1u];
        hipLaunchKernelGGL((muon_gemm_kernel<kNsGram, true, true>), sq, dim3(kTrThreads), 0, s, a);
        MRIRT_HIP(hipGetLastError());
        hipLaunchKernelGGL((muon_gemm_kernel<kNsPoly, true, false>), sq, dim3(kTrThreads), 0, s, a);
        MRIRT_HIP(hipGetLastError());
        hipLaunchKernelGGL((muon_gemm_kernel<kNsUpdate, true, false>), wide, dim3(kTrThreads), 0, s, a);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_muon_scratch_bytes(const MrirtInrDesc* desc) {
    MuonPlan P;
    MuonLayout L;
    return muon_desc(desc, P, L) == MRIRT_OK ? (int64_t)L.bytes : 0;
}

extern "C" int mrirt_muon_orthogonalize(const MrirtInrDesc* desc, const float* m_flat, float* out_flat, const MrirtMuon* hp,
                                        void* scratch, int64_t scratch_bytes, void* stream) {
    MuonPlan P;
    MuonLayout L;
    if (!desc || !m_flat || !out_flat || !hp) return MRIRT_ERR_NULL;
    int rc = muon_desc(desc, P, L);
    if (rc != MRIRT_OK) return rc;
    if ((rc = check_muon(hp)) != MRIRT_OK) return rc;
    if ((rc = check_scratch(scratch, scratch_bytes, L.bytes)) != MRIRT_OK) return rc;
    return newton_schulz(P, L, m_flat, out_flat, hp, (char*)scratch, (hipStream_t)stream);
}

extern "C" int mrirt_muon_step(const MrirtInrDesc* desc, float* w, float* b, const float* gw, const float* gb, float* mu_w,
                               float* mu_b, float* nu_b, const MrirtMuon* hp, const MrirtAdamW* adamw, uint64_t t, float gscale,
                               double* gnorm, void* scratch, int64_t scratch_bytes, void* stream) {
    MuonPlan P;
    MuonLayout L;
    if (!desc || !w || !b || !gw || !gb || !mu_w || !mu_b || !nu_b || !hp || !adamw || !gnorm) return MRIRT_ERR_NULL;
    int rc = muon_desc(desc, P, L);
    if (rc != MRIRT_OK) return rc;
    if ((rc = check_muon(hp)) != MRIRT_OK) return rc;
    if ((rc = opt_check_adamw(adamw, true)) != MRIRT_OK) return rc;
    if (!isfinite(gscale) || ((uintptr_t)gnorm & 7u) != 0) return MRIRT_ERR_ARG;
    if ((rc = check_scratch(scratch, scratch_bytes, L.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    // the clip factor over all gradients and the biases' AdamW: mrirt_inr_adamw_step's own kernels
    if ((rc = opt_norm_and_bias_step(gw, (int64_t)P.nw, b, gb, mu_b, nu_b, (int64_t)P.nb, adamw, t, gscale, gnorm, base, s)) != MRIRT_OK) return rc;
    MuonMomentumArgs m = {};
    const double beta = (double)hp->beta;
    m.gw = gw; m.mu = mu_w; m.mhat = (float*)(base + L.offMhat); m.nw = (int64_t)P.nw; m.gnorm = gnorm;
    m.gscale = gscale; m.beta = hp->beta; m.omb = (float)(1.0 - beta);
    m.c1 = (float)(1.0 - pow(beta, (double)t + 1.0)); m.c2 = (float)(1.0 - pow(beta, (double)t + 2.0));
    m.nesterov = hp->nesterov;
    hipLaunchKernelGGL(muon_momentum_kernel, dim3(elem_blocks(P.nw)), dim3(kMuonThreads), 0, s, m);
    MRIRT_HIP(hipGetLastError());
    float* O = (float*)(base + L.offO);
    if ((rc = newton_schulz(P, L, m.mhat, O, hp, base, s)) != MRIRT_OK) return rc;
    hipLaunchKernelGGL(muon_apply_kernel, dim3(elem_blocks(P.nw)), dim3(kMuonThreads), 0, s, P, w, (const float*)O, adamw->lr, hp->weightDecay);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
