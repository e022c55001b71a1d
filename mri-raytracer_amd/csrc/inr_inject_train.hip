// Coordinate-injection INR, training step: a forward that keeps what the backward needs, and the
// backward from dlogits to every W_l, b_l and the learnable projection B, through the injected inputs and the dropout masks.
// fp32 on v_mfma_f32_16x16x4_f32, through the staging of inr_gemm.h.
//   forward   the feature and layer kernels of csrc/inr_inject.hip, writing every hidden activation to a buffer of its own
//   inj_xt_slab_kernel   X^T . dZ over split-n slabs: the A operand is the three-part view with the roles swapped (k = the
//                        point) plus one row of ones, so db rides with dW; the same kernel forms g^T . c01 for dB
//   inj_dz_kernel        dZ . W^T over the first width[l - 1] (or F) rows of W_l; epilogues: mask, mask-and-scale (both read
//                        the saved post-dropout activation: kept and z > 0  <=>  saved value > 0), plain (layer 0)
//   inj_g_kernel         g = dF_s k - dF_c s, +0 outside the sine's domain; writes c01 beside it
//   inj_slab_reduce_kernel   slab 0 + slab 1 + ... in that order; dB: 2 pi times the finished sum
// No allocation, no host synchronisation, no float atomics, one writer per element: the same inputs give the same bits.
#include "inr_device.h"
#include "inr_gemm.h"
#include "inr_inject_host.h"

namespace mrirt {

enum { kInjDzMask = 0, kInjDzMaskScale = 1, kInjDzPlain = 2 };

__device__ __forceinline__ void inj_fetch_t(const InjViewT& v, uint32_t m0, int64_t k0, int64_t kEnd, float (&reg)[kTrBM / 16]) {
#pragma unroll
    for (int i = 0; i < kTrBM / 16; ++i) {
        uint32_t r, k;
        tr_stage_coord<kTrBM, false>(threadIdx.x, i, r, k);
        int64_t off;
        const int src = inj_viewT_src(v, m0 + r, k0 + k, kEnd, off);
        reg[i] = src == 0 ? v.h[off] : src == 1 ? v.c[off] : src == 2 ? v.m[off] : src == 3 ? 1.0f : 0.0f;
    }
}

template <int BN>
__global__ __launch_bounds__(kTrThreads) void inj_xt_slab_kernel(InjSlabArgs a) {
    __shared__ float As[kTrBK * TrLds<kTrBM>::pitch];
    __shared__ float Bs[kTrBK * TrLds<BN>::pitch];
    constexpr int NT = BN / 16;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m0 = blockIdx.x * kTrBM, n0 = blockIdx.y * BN;
    int64_t kBegin, kEnd;
    tr_slab_range(a.K, a.slabLen, blockIdx.z, kBegin, kEnd);
    f32x4 acc[NT];                                       // gm_accumulate's loop over the three-part A operand
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    float ra[kTrBM / 16], rb[BN / 16];
    inj_fetch_t(a.A, m0, kBegin, kEnd, ra);
    gm_fetch<BN, false>(a.B, n0, kBegin, kEnd, rb);
    for (int64_t k0 = kBegin; k0 < kEnd; k0 += kTrBK) {
        __syncthreads();                                 // the previous tile's reads are done
        gm_stage<kTrBM, false>(As, ra);
        gm_stage<BN, false>(Bs, rb);
        __syncthreads();
        if (k0 + kTrBK < kEnd) {                         // the next tile's loads fly under this tile's MFMAs
            inj_fetch_t(a.A, m0, k0 + kTrBK, kEnd, ra);
            gm_fetch<BN, false>(a.B, n0, k0 + kTrBK, kEnd, rb);
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
            a.C[(uint64_t)blockIdx.z * a.slabStride + (uint64_t)row * a.N + col] = acc[j][r];
        }
    }
}

template <int BN, int EPI>
__global__ __launch_bounds__(kTrThreads) void inj_dz_kernel(InjDzArgs a) {
    __shared__ float As[kTrBK * TrLds<kTrBM>::pitch];
    __shared__ float Bs[kTrBK * TrLds<BN>::pitch];
    constexpr int NT = BN / 16;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m0 = blockIdx.x * kTrBM, n0 = blockIdx.y * BN;
    f32x4 acc[NT];
    gm_accumulate<BN, true, true>(a.A, a.B, m0, n0, 0, a.K, As, Bs, acc);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const uint32_t col = n0 + 16u * j + tr_acc_col(lane);
        if (col >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = m0 + 16u * wave + tr_acc_row(lane, r);
            if (row >= a.M) continue;
            const int64_t at = (int64_t)row * a.N + col;
            float v = acc[j][r];
            if (EPI == kInjDzMaskScale) v = v * a.scale;
            if (EPI != kInjDzPlain) v = a.act[at] > 0.0f ? v : 0.0f;       // a NaN activation passes no gradient
            a.C[at] = v;
        }
    }
}

struct InjGArgs {
    const float* B;              // [F / 2][3]
    const float* coords;         // [n][3]
    const float* feat;           // [n][F]: s | k as the forward saved them
    float* dF;                   // [n][F]: dF on entry; g[p][j] replaces dF[p][j], j < F / 2
    float* c01;                  // [n][3]
    int64_t n;
    uint32_t F;
};

// thread (p, j), j < F / 2: the only reader of dF[p][j] and dF[p][F / 2 + j] and the only writer of g[p][j]
__global__ __launch_bounds__(kInjThreads) void inj_g_kernel(InjGArgs a) {
    const uint32_t half = a.F >> 1;
    const int64_t t = (int64_t)blockIdx.x * kInjThreads + threadIdx.x;
    if (t >= a.n * (int64_t)half) return;
    const int64_t p = t / half;
    const uint32_t j = (uint32_t)(t - p * half);
    const float ux = (a.coords[3 * p] + 1.0f) * 0.5f, uy = (a.coords[3 * p + 1] + 1.0f) * 0.5f, uz = (a.coords[3 * p + 2] + 1.0f) * 0.5f;
    if (j == 0) { a.c01[3 * p] = ux; a.c01[3 * p + 1] = uy; a.c01[3 * p + 2] = uz; }
    const float q = ((ux * a.B[3 * j]) + (uy * a.B[3 * j + 1])) + (uz * a.B[3 * j + 2]);
    const float ang = 6.2831855f * q;
    const float sn = a.feat[p * a.F + j], cs = a.feat[p * a.F + half + j];
    const float ds = a.dF[p * a.F + j], dc = a.dF[p * a.F + half + j];
    const float g = (ds * cs) - (dc * sn);
    a.dF[p * a.F + j] = __builtin_fabsf(ang) <= 1048576.0f ? g : 0.0f;      // outside the domain (a NaN too) the feature is a constant
}

// W / b: grad (+)= slab 0 + slab 1 + ... in that order, rows < in are dW, row in is db.  B (scaleB): the finished sum times
// 2 pi once, then added to the old value when accumulating.
__global__ __launch_bounds__(256) void inj_slab_reduce_kernel(const float* slab, uint64_t slabStride, uint32_t slabs, uint32_t in,
                                                              uint32_t out, float* gw, float* gb, uint32_t accumulate, uint32_t scaleB) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (in + (scaleB ? 0u : 1u)) * out) return;
    float* dst = scaleB ? gw + i : tr_reduce_dst(i, in, out, gw, gb);
    float s = (accumulate && !scaleB) ? *dst : 0.0f;
    for (uint32_t z = 0; z < slabs; ++z) s += slab[(uint64_t)z * slabStride + i];
    if (scaleB) {
        s = 6.2831855f * s;
        if (accumulate) s = *dst + s;
    }
    *dst = s;
}

static int launch_slab(const InjSlabArgs& g, uint32_t slabs, hipStream_t s) {
    const uint32_t mt = (g.M + kTrBM - 1) / kTrBM;
    if (g.N <= 16) hipLaunchKernelGGL((inj_xt_slab_kernel<16>), dim3(mt, 1, slabs), dim3(kTrThreads), 0, s, g);
    else hipLaunchKernelGGL((inj_xt_slab_kernel<64>), dim3(mt, (g.N + 63) / 64, slabs), dim3(kTrThreads), 0, s, g);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

template <int EPI>
static int launch_dz(const InjDzArgs& d, hipStream_t s) {
    const uint32_t mt = (d.M + kTrBM - 1) / kTrBM;
    if (d.N <= 16) hipLaunchKernelGGL((inj_dz_kernel<16, EPI>), dim3(mt, 1), dim3(kTrThreads), 0, s, d);
    else hipLaunchKernelGGL((inj_dz_kernel<64, EPI>), dim3(mt, (d.N + 63) / 64), dim3(kTrThreads), 0, s, d);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

// what both entry points check before anything else, in the order of mrirt_inject_forward
static int train_check(const MrirtInjectDesc* desc, const float* B, const float* w, const float* coords, const float* mods, int64_t n,
                       InjNet& N) {
    const int rc = inj_desc(desc, N);
    if (rc != MRIRT_OK) return rc;
    if (!B || !w || !coords || (N.M != 0 && !mods)) return MRIRT_ERR_NULL;
    if (n < 1 || n >= ((int64_t)1 << 31)) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_inject_train_scratch_bytes(const MrirtInjectDesc* desc, int64_t n) {
    InjNet N;
    if (inj_desc(desc, N) != MRIRT_OK || n < 1 || n >= ((int64_t)1 << 31)) return 0;
    return (int64_t)inj_train_layout(N, n).bytes;
}

extern "C" int mrirt_inject_forward_train(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                                          const float* mods, int64_t n, const MrirtInjectDropout* dropout, float* logits, void* scratch,
                                          int64_t scratch_bytes, void* stream) {
    InjNet N;
    int rc = train_check(desc, B, w, coords, mods, n, N);
    if (rc != MRIRT_OK) return rc;
    if (!b || !logits) return MRIRT_ERR_NULL;
    if (dropout && ((rc = inj_check_dropout(dropout, 1)) != MRIRT_OK)) return rc;
    const InjTrainLayout T = inj_train_layout(N, n);
    if ((rc = check_scratch(scratch, scratch_bytes, T.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    float* feat = (float*)(base + T.offFeat);
    float* act[kInjMaxLayers] = {};
    for (uint32_t l = 0; l + 1 < N.numLayers; ++l) act[l] = (float*)(base + T.offH[l]);
    if ((rc = inj_run_features(N, B, coords, n, 0, nullptr, nullptr, feat, s)) != MRIRT_OK) return rc;
    return inj_run_layers(N, feat, act, w, b, coords, mods, (int64_t)N.M, 1, n, inj_drop(dropout, 0), logits, s);
}

extern "C" int mrirt_inject_backward(const MrirtInjectDesc* desc, const float* B, const float* w, const float* coords, const float* mods,
                                     int64_t n, const MrirtInjectDropout* dropout, const float* dlogits, float* grad_B, float* grad_w,
                                     float* grad_b, uint32_t flags, void* scratch, int64_t scratch_bytes, void* stream) {
    InjNet N;
    int rc = train_check(desc, B, w, coords, mods, n, N);
    if (rc != MRIRT_OK) return rc;
    if (!dlogits || !grad_B || !grad_w || !grad_b) return MRIRT_ERR_NULL;
    if (dropout && ((rc = inj_check_dropout(dropout, 1)) != MRIRT_OK)) return rc;
    if (flags > 1u) return MRIRT_ERR_ARG;
    const InjTrainLayout T = inj_train_layout(N, n);
    if ((rc = check_scratch(scratch, scratch_bytes, T.bytes)) != MRIRT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    const InjDrop d = inj_drop(dropout, 0);
    const float* feat = (const float*)(base + T.offFeat);
    float* slab = (float*)(base + T.offSlab);
    float* dF = (float*)(base + T.offDF);
    float* c01 = (float*)(base + T.offC01);
    const uint32_t acc = flags & 1u;
    const float* dz = dlogits;
    for (uint32_t l = N.numLayers; l-- > 0;) {
        const float* hin = l == 0 ? feat : (const float*)(base + T.offH[l - 1]);
        if ((rc = launch_slab(inj_slab_args(N, T, l, n, hin, coords, mods, dz, slab), T.slabs, s)) != MRIRT_OK) return rc;
        const uint32_t elems = (N.in[l] + 1) * N.out[l];
        hipLaunchKernelGGL(inj_slab_reduce_kernel, dim3((elems + 255) / 256), dim3(256), 0, s, slab, T.slabElems, T.slabs, N.in[l], N.out[l],
                           grad_w + N.wOff[l], grad_b + N.bOff[l], acc, 0u);
        MRIRT_HIP(hipGetLastError());
        if (l == 0) {
            rc = launch_dz<kInjDzPlain>(inj_dz_args(N, 0, n, dz, w, nullptr, 1.0f, dF), s);
        } else {
            float* dzPrev = (float*)(base + inj_dz_offset(N, T, l));
            const InjDzArgs a = inj_dz_args(N, l, n, dz, w, hin, d.on ? d.scale : 1.0f, dzPrev);
            rc = d.on ? launch_dz<kInjDzMaskScale>(a, s) : launch_dz<kInjDzMask>(a, s);
            dz = dzPrev;
        }
        if (rc != MRIRT_OK) return rc;
    }
    InjGArgs g = {};
    g.B = B; g.coords = coords; g.feat = feat; g.dF = dF; g.c01 = c01; g.n = n; g.F = N.F;
    hipLaunchKernelGGL(inj_g_kernel, dim3((uint32_t)((n * (int64_t)(N.F / 2) + kInjThreads - 1) / kInjThreads)), dim3(kInjThreads), 0, s, g);
    MRIRT_HIP(hipGetLastError());
    if ((rc = launch_slab(inj_slab_args_B(N, T, n, dF, c01, slab), T.slabs, s)) != MRIRT_OK) return rc;
    const uint32_t elemsB = (N.F / 2) * 3;
    hipLaunchKernelGGL(inj_slab_reduce_kernel, dim3((elemsB + 255) / 256), dim3(256), 0, s, slab, T.slabElems, T.slabs, N.F / 2, 3u, grad_B,
                       (float*)nullptr, acc, 1u);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
