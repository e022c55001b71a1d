// The RGBA transfer-function table of the K1 march (brats_tf.hip, mrirt_render_brats_tf): the table's
// kernel argument, its copy into LDS and TableEvent, the per-sample event composite() (brats_device.h) runs in place of its
// grey ramp.
//
// composite() is one function for both: window, level and gamma stay as the table's domain mapping, the shading factor and
// the overlays follow unchanged.  In between, per sample (STRICT: unfused fp32 in this order; FAST contracts as elsewhere):
//     u = val * float(N - 1);  i = min(uint(floor(u)), N - 2);  f = u - float(i)          (exact)
//     e[k] = lerp(tf[i][k], tf[i + 1][k], f), k = 0..3;  sigma = e[3];  ++nLive
//     if sigma > 0:  alpha = 1 - exp(-(sigma * intensityAlpha) * stepSize)                 (always the full-range exp)
//                    C[k] += (alpha * T) * (e[k] * shade);  T *= 1 - alpha                 (shade = 1 when shading is off)
// With the two-entry ramp (0,0,0,0), (1,1,1,1): i = 0, f = val, e[k] = 0 + val * (1 - 0) = val — GreyRamp's frame exactly.
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

// composite()'s EVENT of the table kernels (see the head of this file)
struct TableEvent {
    const TfTable& tf;
    const float4* tfS;               // stage_tf's copy of the rows
    // through the table the sign of a zero intensity can reach the frame (f, and a lerp from a row that holds -0): the
    // pipelined stages keep the generic kernel's 0 + s * w (Stage::consume)
    static constexpr bool kSeesZeroSign = true;
    template <bool STRICT>
    __device__ __forceinline__ EventSample sample(float val) const {
        using Mm = M<STRICT>;
        const float u = val * tf.top;
        // val is in [0, 1], so u is in [0, N - 1] and the clamp changes nothing; it keeps the row index inside the table for a
        // gamma that makes pow() return inf or NaN (the clamp maps NaN to 0)
        const uint32_t i = min((uint32_t)floorf(clampf(u, 0.0f, tf.top)), tf.last);
        const float f = u - (float)i;
        const float4 lo = tfS[i], hi = tfS[i + 1u];                      // two adjacent rows: ds_read_b128 each
        return { Mm::lerp(lo.x, hi.x, f), Mm::lerp(lo.y, hi.y, f), Mm::lerp(lo.z, hi.z, f), Mm::lerp(lo.w, hi.w, f) };
    }
    template <bool STRICT, bool LIT>
    __device__ __forceinline__ float exp(const K1Args&, float ex) const {
        return M<STRICT>::exp_lit(ex);                               // sigma is not bounded by 1: never a.expSmall's short form
    }
};

}  // namespace mrirt
