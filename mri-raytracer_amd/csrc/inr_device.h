// Device-only pieces the INR training kernels share (csrc/inr_train.hip, inr_optim.hip, inr_lossx.hip, inr_muon.hip): the
// fp64 wave sum, the per-point softmax of the two losses and the write-out of a sampled voxel.  Not for the host harnesses
// under tests/native/: what they walk is the index arithmetic of inr_train.h / inr_optim.h.
#pragma once
#include "inr_optim.h"

namespace mrirt {

// the 64 lanes fold by halves; lane 0 holds the wave's sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// softmax of one point: p[k] (fp32) and d[k] = z[k] - max (both 0 for k >= C); with PICK also dl = d[label] (0 for a label
// outside 0..C-1).  Returns s = sum_k exp d[k]: log p[k] = d[k] - logf(s).  What a caller does not read costs it nothing;
// PICK is a compile-time flag because an unread pick still changed the extended loss's registers (profiles/r15_inr_shared).
template <bool PICK>
__device__ __forceinline__ float point_softmax(const float* z, uint32_t C, int32_t label, float (&p)[kLossMaxClasses],
                                               float (&d)[kLossMaxClasses], float& dl) {
    float m = z[0];
    for (uint32_t k = 1; k < C; ++k) m = fmaxf(m, z[k]);
    float s = 0.0f;
    dl = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) {
        p[k] = 0.0f;
        d[k] = 0.0f;
        if (k < C) {
            d[k] = z[k] - m;
            p[k] = expf(d[k]);
            s += p[k];
            if (PICK && (int32_t)k == label) dl = d[k];
        }
    }
    const float inv = 1.0f / s;
#pragma unroll
    for (uint32_t k = 0; k < kLossMaxClasses; ++k) p[k] *= inv;
    return s;
}

// ... for a caller that needs no d[label]
__device__ __forceinline__ float point_softmax(const float* z, uint32_t C, float (&p)[kLossMaxClasses], float (&d)[kLossMaxClasses]) {
    float dl;
    return point_softmax<false>(z, C, 0, p, d, dl);
}

// row i of coords / labels / feats for the drawn voxel p: M + 1 dependent gathers.  The pointers come one by one, by value: a
// kernel that hands over its argument struct loses their address space (flat loads where these are global)
__device__ __forceinline__ void sample_write(int64_t i, const SamplePoint& p, const float* const* mods, const int16_t* const* seg,
                                             uint32_t M, uint32_t H, uint32_t W, uint32_t D, int64_t hwd, float* coords,
                                             float* feats, int32_t* labels) {
    const int64_t v = voxel_offset(p.x, p.y, p.z, W, D);
    coords[3 * i + 0] = sample_coord(p.x, H);
    coords[3 * i + 1] = sample_coord(p.y, W);
    coords[3 * i + 2] = sample_coord(p.z, D);
    labels[i] = (int32_t)seg[p.cs][v];
    if (M) {
        const float* m = mods[p.cs];
        for (uint32_t k = 0; k < M; ++k) feats[i * M + k] = m[mod_offset(k, v, hwd)];
    }
}

}  // namespace mrirt
