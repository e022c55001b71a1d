// The RGBA transfer-function table of the K1 march (brats_tf.hip, mrirt_render_brats_tf): the table's
// kernel argument, its copy into LDS and the per-sample event that replaces composite()'s grey ramp.
//
// Everything up to `val` is composite()'s code (brats_device.h): window, level and gamma stay as the table's domain mapping.
// Then, per sample (STRICT: unfused fp32 in this order; FAST contracts as elsewhere):
//     u = val * float(N - 1);  i = min(uint(floor(u)), N - 2);  f = u - float(i)          (exact)
//     e[k] = lerp(tf[i][k], tf[i + 1][k], f), k = 0..3;  sigma = e[3];  ++nLive
//     if sigma > 0:  alpha = 1 - exp(-(sigma * intensityAlpha) * stepSize)                 (always the full-range exp)
//                    C[k] += (alpha * T) * (e[k] * shade);  T *= 1 - alpha                 (shade = 1 when shading is off)
// With the two-entry ramp (0,0,0,0), (1,1,1,1): i = 0, f = val, e[k] = 0 + val * (1 - 0) = val — composite()'s frame exactly.
#pragma once
#include "brats_device.h"

namespace mrirt {

constexpr uint32_t kTfMinEntries = 2u, kTfMaxEntries = 1024u;

struct TfTable {
    const float4* rows;      // N x (r, g, b, sigma) in device memory, 16-byte aligned
    uint32_t n;              // 2 .. 1024
    uint32_t last;           // N - 2: the largest first row of a lookup
    float top;               // float(N - 1)
};

// The table into LDS, once per workgroup: coalesced 16-byte loads; the barrier is stage_lut's, which every table kernel calls
// next.  Why LDS: a per-lane table index read from global memory is a vector-memory load the compiler cannot count past (it
// would drain the gathers in flight, see stage_lut); two ds_read_b128 count on lgkmcnt.
__device__ __forceinline__ void stage_tf(const TfTable& tf, float4* tfS) {
    for (uint32_t i = threadIdx.x; i < tf.n; i += blockDim.x) tfS[i] = tf.rows[i];
}

// composite() line by line, except for the intensity event (see the head of this file).  GAMMA1: gamma == 1, where
// pow(val, 1) == val exactly (the pipelined kernels compile the fp64 pow out, as composite()'s GAMMA1 does)
template <bool STRICT, bool SHADE, bool GAMMA1 = false>
__device__ __forceinline__ void composite_tf(const K1Args& a, const TfTable& tf, const float4* tfS, const float rd[3], const Labels& lb,
                                             float v, const float g[3], RayState& r, const float4* lutS) {
    using Mm = M<STRICT>;
    if (a.wsum.d > 0.0f && a.wsum.d != 1.0f) v = Mm::divu_data(v, a.wsum);
    float val = satf(Mm::divu_data(v - a.tfLo, a.wwDiv));
    if constexpr (!GAMMA1) val = Mm::pow(val, a.gamma);
    ++r.nLive;
    const float u = val * tf.top;
    // val is in [0, 1], so u is in [0, N - 1] and the clamp changes nothing; it keeps the row index inside the table for a
    // gamma that makes pow() return inf or NaN (the clamp maps NaN to 0)
    const uint32_t i = min((uint32_t)floorf(clampf(u, 0.0f, tf.top)), tf.last);
    const float f = u - (float)i;
    const float4 lo = tfS[i], hi = tfS[i + 1u];                      // two adjacent rows: ds_read_b128 each
    const float e0 = Mm::lerp(lo.x, hi.x, f), e1 = Mm::lerp(lo.y, hi.y, f), e2 = Mm::lerp(lo.z, hi.z, f);
    const float sigma = Mm::lerp(lo.w, hi.w, f);
    if (sigma > 0.0f) {
        const float ex = -(sigma * a.intensityAlpha) * a.stepSize;
        const float alpha = 1.0f - Mm::exp_lit(ex);                   // sigma is not bounded by 1: never a.expSmall's short form
        const float at = alpha * r.T;
        if constexpr (SHADE) {
            const float gx = g[0] * a.halfInvVoxel[0], gy = g[1] * a.halfInvVoxel[1], gz = g[2] * a.halfInvVoxel[2];
            const float len2 = dot3(gx, gy, gz, gx, gy, gz);
            const float glen = STRICT ? sqrtf(len2) : __builtin_amdgcn_sqrtf(len2);
            float shade = a.ka + a.kd;
            if (glen > a.gradEps) {
                const float gd = fabsf(dot3(gx, gy, gz, rd[0], rd[1], rd[2]));
                const float ndl = fminf(STRICT ? gd / glen : gd * __builtin_amdgcn_rcpf(glen), 1.0f);
                float spec = ndl;
                for (uint32_t k = 0; k < a.specPow2; ++k) spec = spec * spec;
                shade = (a.ka + a.kd * ndl) + a.ks * spec;
            }
            r.C0 += at * (e0 * shade); r.C1 += at * (e1 * shade); r.C2 += at * (e2 * shade);
            ++r.nShaded;
        } else {
            r.C0 += at * e0; r.C1 += at * e1; r.C2 += at * e2;
        }
        r.T *= (1.0f - alpha);
    }
    if (a.showSeg != 0) {                                            // brats_rt.slang:143-151, as composite()
        const uint32_t l = lb.seg;
        if (l > 0 && l < 8) {
            const float4 c = lutS[l];
            const float alpha = c.w;
            const float at = alpha * r.T;
            r.C0 += at * c.x; r.C1 += at * c.y; r.C2 += at * c.z;
            r.T *= (1.0f - alpha);
        }
    }
    if (a.showPred != 0) {                                           // :154-162
        const uint32_t l = lb.pred;
        if (l > 0 && l < 8) {
            const float4 c = lutS[8u + l];
            const float alpha = c.w;
            const float at = alpha * r.T;
            r.C0 += at * c.x; r.C1 += at * c.y; r.C2 += at * c.z;
            r.T *= (1.0f - alpha);
        }
    }
}

}  // namespace mrirt
