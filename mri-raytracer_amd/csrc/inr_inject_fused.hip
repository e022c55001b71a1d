// Fused forward of the coordinate-injection INR: one launch from coords / mods to classes.
//   inj_fused_kernel   a workgroup stages the whole network into LDS once (one barrier), then walks 64-row tiles in a
//                      grid-stride loop; a wave owns 16 rows: features straight into its A-buffer, every layer on
//                      v_mfma_f32_16x16x4_f32 from LDS to LDS, the head's argmax from LDS.  The row count comes from device
//                      memory (count_dev) or from the host (n_max); rows at or beyond it are neither read nor written.
// The per-element feature code, the order of every layer's products (k in increasing groups of four from +0, then + bias,
// then the ReLU) and the argmax are the chain's (csrc/inr_inject.hip), so logits and classes are mrirt_inject_forward's bits.
// The layout and every index are csrc/inr_inject_fused.h's.  No dropout, no atomics, one writer per output.
#include <atomic>

#include "inr_device.h"
#include "inr_gemm.h"
#include "inr_inject_fused.h"
#include "inr_inject_host.h"
#include "brats_host.h"

namespace mrirt {

struct InjFusedArgs {
    InjNet N;
    InjFusedLayout Y;
    const float *B, *w, *b, *coords, *mods;
    const uint32_t* countDev;    // NULL: nMax rows
    uint32_t nMax;
    int16_t* argmax;             // NULL: not wanted
    float* logits;               // NULL: not wanted
};

// Between two phases of a wave that exchange data through its LDS buffers: the LDS executes one wave's instructions in
// order, so all that is needed is that the compiler keeps them in order.
__device__ __forceinline__ void fused_phase() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// NT column tiles (from tile j0) of layer l over all of its k: NT accumulators in flight cover the MFMA's dependent latency
template <int NT>
__device__ __forceinline__ void fused_tiles(const InjFusedArgs& a, const float* lds, const float* in, float* out, uint32_t l, uint32_t j0,
                                            uint32_t lane, bool head, uint32_t row0, uint32_t n) {
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const uint32_t steps = a.Y.kPad[l] >> 2;
    const float* ap = in + fused_frag_a(0, lane);
    const float* bp = lds + fused_frag_b(a.Y, l, 0, j0, lane);
    const uint32_t bStep = 4u * a.Y.pitch[l];
    uint32_t s = 0;
    do {                                                 // kPad >= 4: at least one step, and no zero-trip path joins behind the loop
        const float av = ap[s * (4u * kFusedWaveRows)];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float bv = bp[s * bStep + 16u * j];
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
        }
        // hipcc leaves 10 wait states between the loop's last MFMA and the copies of its result behind the loop's exit; the
        // build's scan of matrix-core results (tools/check_async_loads.py) holds every kernel to 11.  One idle cycle per
        // step, against NT MFMAs of 32
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 0");
    } while (++s < steps);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const uint32_t col = 16u * (j0 + j) + tr_acc_col(lane);
        if (col >= a.N.out[l]) continue;
        const float bias = lds[a.Y.bOff[l] + col];
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t = acc[j][r] + bias;
            if (!head) t = !(t <= 0.0f) ? t : 0.0f;              // jnp.maximum(t, 0): -0 -> +0, a NaN stays
            v[r] = t;
        }
        *reinterpret_cast<f32x4*>(out + fused_epi_index(j0 + j, lane)) = v;
        if (head && a.logits) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t row = row0 + tr_acc_row(lane, r);
                if (row < n) a.logits[(size_t)row * a.N.C + col] = v[r];
            }
        }
    }
}

__global__ __launch_bounds__(kFusedThreads) void inj_fused_kernel(const InjFusedArgs a) {
    extern __shared__ f32x4 fusedLds[];
    float* lds = reinterpret_cast<float*>(fusedLds);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, r16 = lane & 15u, g = lane >> 4;
    const uint32_t L = a.N.numLayers;
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t elems = a.Y.kPad[l] * a.Y.pitch[l];
        for (uint32_t e = threadIdx.x; e < elems; e += kFusedThreads) {
            const int64_t src = fused_stage_src(a.N, a.Y, l, e);
            lds[a.Y.wOff[l] + e] = src >= 0 ? a.w[src] : 0.0f;
        }
        for (uint32_t c = threadIdx.x; c < a.Y.outPad[l]; c += kFusedThreads) lds[a.Y.bOff[l] + c] = c < a.N.out[l] ? a.b[a.N.bOff[l] + c] : 0.0f;
    }
    const uint32_t half = a.N.F >> 1;
    for (uint32_t e = threadIdx.x; e < half * 3u; e += kFusedThreads) lds[a.Y.offB + e] = a.B[e];
    __syncthreads();                                     // the only workgroup barrier: from here on a wave works alone

    const uint32_t n = fused_rows(a.nMax, a.countDev != nullptr, a.countDev ? *a.countDev : 0u);
    const uint32_t buf0 = a.Y.offWave + wave * a.Y.waveFloats, buf1 = buf0 + a.Y.bufFloats[0];
    const float* Bs = lds + a.Y.offB;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kFusedTileRows - 1) / kFusedTileRows);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row0 = tile * kFusedTileRows + wave * kFusedWaveRows;
        if (row0 >= n) continue;                         // wave-uniform
        const uint32_t row = row0 + r16;
        const bool valid = row < n;
        float c3[3] = { 0.0f, 0.0f, 0.0f }, ext[kFusedExt];
        if (valid) { c3[0] = a.coords[3 * (size_t)row]; c3[1] = a.coords[3 * (size_t)row + 1]; c3[2] = a.coords[3 * (size_t)row + 2]; }
#pragma unroll
        for (uint32_t i = 0; i < kFusedExt; ++i) {
            const uint32_t e = g + 4u * i;
            ext[i] = e < 3u ? (g == 0 ? c3[0] : g == 1 ? c3[1] : c3[2]) : (valid && e - 3u < a.N.M) ? a.mods[(size_t)row * a.N.M + (e - 3u)] : 0.0f;
        }
        // features of the wave's 16 rows: lane (row r16, j = g, g + 4, ..)
        for (uint32_t j = g; j < half; j += 4u) {
            float sn, cs;
            inj_feature(c3[0], c3[1], c3[2], Bs[3 * j], Bs[3 * j + 1], Bs[3 * j + 2], sn, cs);
            lds[buf0 + fused_a_index(j, r16)] = sn;
            lds[buf0 + fused_a_index(half + j, r16)] = cs;
        }
        for (uint32_t l = 0; l < L; ++l) {
            float* in = lds + ((l & 1u) ? buf1 : buf0);
            float* out = lds + ((l & 1u) ? buf0 : buf1);
            // the rest of layer l's operand: its injected columns, then zeros up to kPad
#pragma unroll
            for (uint32_t i = 0; i < kFusedExt; ++i) {
                const int k = fused_ext_k(a.N, l, g + 4u * i);
                if (k >= 0) in[fused_a_index((uint32_t)k, r16)] = ext[i];
            }
            if (lane < (a.Y.kPad[l] - a.N.in[l]) * kFusedWaveRows) in[fused_a_index(a.N.in[l], 0) + lane] = 0.0f;
            fused_phase();
            const bool head = l + 1u == L;
            const uint32_t nt = a.Y.outPad[l] >> 4;
            for (uint32_t j0 = 0; j0 < nt; j0 += kFusedGroup) {
                const uint32_t left = nt - j0;
                if (left >= 4u) fused_tiles<4>(a, lds, in, out, l, j0, lane, head, row0, n);
                else if (left == 3u) fused_tiles<3>(a, lds, in, out, l, j0, lane, head, row0, n);
                else if (left == 2u) fused_tiles<2>(a, lds, in, out, l, j0, lane, head, row0, n);
                else fused_tiles<1>(a, lds, in, out, l, j0, lane, head, row0, n);
            }
            fused_phase();
        }
        if (a.argmax && lane < kFusedWaveRows && valid)
            a.argmax[row] = (int16_t)inj_argmax_strided(lds + ((L & 1u) ? buf1 : buf0) + fused_a_index(0, r16), a.N.C, kFusedWaveRows);
        fused_phase();                                   // the next tile's features overwrite what the argmax read
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

static int fused_net(const MrirtInjectDesc* desc, InjNet& N, InjFusedLayout& Y) {
    const int rc = inj_desc(desc, N);
    if (rc != MRIRT_OK) return rc;
    Y = inj_fused_layout(N);
    return inj_fused_fits(Y) ? MRIRT_OK : MRIRT_ERR_ARG;
}

int inj_fused_check(const MrirtInjectDesc* desc) {
    InjNet N;
    InjFusedLayout Y;
    return fused_net(desc, N, Y);
}

// the dynamic-LDS limit of the kernel is raised once per device, its result checked before the first launch
static int fused_prepare(int& cus) {
    constexpr int kMaxDev = 64;
    static std::atomic<int> cuCount[kMaxDev];            // 0: this device's limit is not raised yet
    int dev = 0;
    MRIRT_HIP(hipGetDevice(&dev));
    const bool slot = dev >= 0 && dev < kMaxDev;
    cus = slot ? cuCount[dev].load(std::memory_order_acquire) : 0;
    if (cus != 0) return MRIRT_OK;
    MRIRT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(inj_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kFusedLdsBudget));
    MRIRT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) cus = 256;
    if (slot) cuCount[dev].store(cus, std::memory_order_release);
    return MRIRT_OK;
}

// Every argument was checked by the caller (inj_fused_check, pointers, 1 <= nMax < 2^31).
int inj_fused_dev_n(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords, const float* mods,
                    int64_t nMax, const uint32_t* nDev, int16_t* argmax, float* logits, hipStream_t s) {
    InjFusedArgs a = {};
    int rc = fused_net(desc, a.N, a.Y);
    if (rc != MRIRT_OK) return rc;
    if (nMax < 1 || nMax >= ((int64_t)1 << 31)) return MRIRT_ERR_ARG;
    a.B = B; a.w = w; a.b = b; a.coords = coords; a.mods = mods;
    a.countDev = nDev; a.nMax = (uint32_t)nMax; a.argmax = argmax; a.logits = logits;
    int cus = 0;
    if ((rc = fused_prepare(cus)) != MRIRT_OK) return rc;
    // as many workgroups as are resident at once: the LDS decides how many share a CU
    const int64_t perCu = (int64_t)(kFusedLdsBudget / a.Y.bytes) < 8 ? (int64_t)(kFusedLdsBudget / a.Y.bytes) : 8;
    const int64_t tiles = (nMax + kFusedTileRows - 1) / kFusedTileRows, resident = (int64_t)cus * perCu;
    hipLaunchKernelGGL(inj_fused_kernel, dim3((uint32_t)(tiles < resident ? tiles : resident)), dim3(kFusedThreads), (size_t)a.Y.bytes, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_inject_fused_lds_bytes(const MrirtInjectDesc* desc) {
    InjNet N;
    InjFusedLayout Y;
    return fused_net(desc, N, Y) == MRIRT_OK ? (int64_t)Y.bytes : 0;
}

extern "C" int mrirt_inject_classify(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                                     const float* mods, int64_t n_max, const uint32_t* count_dev, int16_t* argmax, float* logits,
                                     void* stream) {
    InjNet N;
    InjFusedLayout Y;
    int rc = inj_desc(desc, N);
    if (rc != MRIRT_OK) return rc;
    if (!B || !w || !b || !coords || (N.M != 0 && !mods) || (!argmax && !logits)) return MRIRT_ERR_NULL;
    if ((rc = fused_net(desc, N, Y)) != MRIRT_OK) return rc;
    if (n_max < 1 || n_max >= ((int64_t)1 << 31)) return MRIRT_ERR_ARG;
    return inj_fused_dev_n(desc, B, w, b, coords, mods, n_max, count_dev, argmax, logits, (hipStream_t)stream);
}

// mrirt_render_brats_inr's frame (csrc/brats_c5.hip: c5_frame) with this network: a pass's batch is classified by the fused
// forward, which reads the batch size from the same device word.  The refinement ticket counters stay unused.
struct C5InjectNet { const MrirtInjectDesc* desc; const float *B, *w, *b; };

static int c5_classify_inject(const C5Scratch& sc, uint32_t c, hipStream_t s, const void* ctx) {
    const C5InjectNet* n = static_cast<const C5InjectNet*>(ctx);
    return inj_fused_dev_n(n->desc, n->B, n->w, n->b, sc.coords, sc.feats, sc.cap, sc.counters + c, sc.classes, nullptr, s);
}

extern "C" int mrirt_render_brats_inject(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                         const void* labels, const MrirtInjectDesc* desc, const float* B, const float* w, const float* b,
                                         const float zmu[4], const float zsigma[4], uint32_t chunk_steps, void* scratch,
                                         int64_t scratch_bytes, void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream) {
    if (!desc || !B || !w || !b) return MRIRT_ERR_NULL;
    int rc = c5_check_common(ext, vol, zmu, zsigma, scratch, out_rgba);
    if (rc != MRIRT_OK) return rc;
    if ((rc = inj_fused_check(desc)) != MRIRT_OK) return rc;
    if (desc->numMods != 4) return MRIRT_ERR_ARG;                // sc.feats holds the four z-scored modalities as [n][4]
    const C5InjectNet net = { desc, B, w, b };
    return c5_frame(p, ext, vol, labels, zmu, zsigma, chunk_steps, scratch, scratch_bytes, out_rgba, pitch_px, stats_dev, stream,
                    ((int64_t)1 << 31) - 1, c5_classify_inject, &net);
}
