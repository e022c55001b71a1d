// The LDS-tiled fp32 GEMM of DESIGN.md section 14 (v_mfma_f32_16x16x4_f32), device side: staging of the two operand views and
// the k loop that accumulates one 64 x BN block tile.  gm_fetch / gm_stage serve csrc/inr_train.hip's tr_gemm_kernel and
// csrc/inr_muon.hip's muon_gemm_kernel alike; gm_accumulate serves Muon only, and tr_gemm_kernel keeps a copy of that loop.
// Calling gm_accumulate from tr_gemm_kernel was measured and dropped (profiles/r15_inr_shared): same
// bits, no spills, but the forward instantiations <64,1,0,*> went from 72 to 76 registers (7 -> 6 waves per SIMD) and the
// step at n = 65536 over 256-wide layers became 0.6 - 1.3 % slower, several times the parent's run-to-run spread.  The
// index arithmetic lives in inr_train.h.  Device code only.
#pragma once
#include "inr_train.h"

namespace mrirt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int R, bool KFAST>
__device__ __forceinline__ void gm_fetch(const TrView& v, uint32_t non0, int64_t k0, int64_t kEnd, float (&reg)[R / 16]) {
#pragma unroll
    for (int i = 0; i < R / 16; ++i) {
        uint32_t r, k;
        tr_stage_coord<R, KFAST>(threadIdx.x, i, r, k);
        const int64_t off = tr_view_offset(v, non0 + r, k0 + k, kEnd);
        reg[i] = off >= 0 ? v.p[off] : (off == -2 ? 1.0f : 0.0f);
    }
}

template <int R, bool KFAST>
__device__ __forceinline__ void gm_stage(float* lds, const float (&reg)[R / 16]) {
#pragma unroll
    for (int i = 0; i < R / 16; ++i) {
        uint32_t r, k;
        tr_stage_coord<R, KFAST>(threadIdx.x, i, r, k);
        lds[k * TrLds<R>::pitch + r] = reg[i];
    }
}

// acc[j] (j < BN / 16) = rows m0 + 16 wave .. + 15, columns n0 + 16 j .. + 15 of A . B over kBegin <= k < kEnd, summed in
// increasing k.  As / Bs: the block's LDS tiles (kTrBK x pitch floats each).  Every thread of the block calls it.
template <int BN, bool AKFAST, bool BKFAST>
__device__ __forceinline__ void gm_accumulate(const TrView& A, const TrView& B, uint32_t m0, uint32_t n0, int64_t kBegin,
                                                   int64_t kEnd, float* As, float* Bs, f32x4 (&acc)[BN / 16]) {
    constexpr int NT = BN / 16;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    float ra[kTrBM / 16], rb[BN / 16];
    gm_fetch<kTrBM, AKFAST>(A, m0, kBegin, kEnd, ra);
    gm_fetch<BN, BKFAST>(B, n0, kBegin, kEnd, rb);
    for (int64_t k0 = kBegin; k0 < kEnd; k0 += kTrBK) {
        __syncthreads();                                 // the previous tile's reads are done
        gm_stage<kTrBM, AKFAST>(As, ra);
        gm_stage<BN, BKFAST>(Bs, rb);
        __syncthreads();
        if (k0 + kTrBK < kEnd) {                         // the next tile's loads fly under this tile's MFMAs
            gm_fetch<kTrBM, AKFAST>(A, m0, k0 + kTrBK, kEnd, ra);
            gm_fetch<BN, BKFAST>(B, n0, k0 + kTrBK, kEnd, rb);
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
}

}  // namespace mrirt
