// What ONE sample of a K1 ray contributes to the soft prediction overlay (brats_soft.hip): the event the sample's class
// probabilities draw, and its derivative chain down to the sample's logits.  MRIRT_HD: the kernels run it per lane,
// tests/native/brats_soft_harness.hip walks the same functions on the CPU under AddressSanitizer + UBSan (as brats_grad.h).
//
// The event replaces the prediction overlay of brats_rt.slang:154-162 (composite() of brats_device.h, `lb.pred`), per step with
// z = the sample's C logits (fp32, 1 <= C <= 16), Kc = min(C, 8), D = stepSize * 1.5, w_k = lutColorAlpha[k].w,
// rgb_k = lutColorAlpha[k].rgb:
//     p = softmax(z)                          (all C classes)
//     sigma = sum_{k=1..Kc-1} p_k w_k         E = sum_{k=1..Kc-1} p_k w_k rgb_k
//     sigma > 0:   alpha = 1 - exp(-sigma D)  c = E / sigma            (fp64 from the fp32 logits; each rounded ONCE to fp32)
//     at = alpha T;  C += at c;  T *= 1 - alpha                        (fp32, exactly a label event of composite())
// and no event where sigma <= 0 (every LUT opacity zero, C == 1, the softmax underflowed onto class 0 or onto classes >= 8,
// a NaN row).  One-hot probabilities on class l give c == rgb_l exactly: w_l rgb_l is exact in fp64 and so is its quotient by w_l.
// With L = sum_p G[p] . C[p], T the transmittance in front of the event and R the colour every LATER event of the ray adds:
//     dL/dalpha = T (G . c) - (G . R) / (1 - alpha)
//     dL/dc     = T alpha G
//     dL/dp_k   = w_k [ dL/dalpha D (1 - alpha) + T alpha G . (rgb_k - c) / sigma ]     1 <= k < Kc;   0 for k = 0 and k >= 8
//     dlogits_j = p_j (dL/dp_j - sum_k p_k dL/dp_k)
// dL/dalpha only ever appears times (1 - alpha), so the chain carries dA = (1 - alpha) T (G . c) - G . R and never divides by
// 1 - alpha (which underflows to 0 for sigma D > 745).  All of it is fp64; dlogits is rounded once to fp32.
//
// The row is read from memory four logits at a time (one 16-byte load where VEC: C % 4 == 0 and the row is 16-byte aligned),
// once per pass — maximum, sums, and in the backward the probabilities again — so no per-class array lives in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mrirt_device.h"

namespace mrirt {

constexpr uint32_t kSoftMaxClasses = 16;     // logits per row
constexpr uint32_t kSoftDrawn = 8;           // LUT rows: classes >= 8 carry probability mass but draw nothing

// w_k and w_k rgb_k of LUT row k, exact in fp64 (24 x 24 bit products)
struct SoftRow { double w, wr, wg, wb; };

MRIRT_HD SoftRow soft_row(const float lut[4]) {
    const double w = (double)lut[3];
    return SoftRow{ w, w * (double)lut[0], w * (double)lut[1], w * (double)lut[2] };
}

// the launch refuses a LUT whose drawn opacities are negative or not finite (sigma would lose its sign or its meaning)
MRIRT_HD bool soft_lut_ok(const float lut[8][4]) {
    for (uint32_t k = 1; k < kSoftDrawn; ++k)
        if (!(lut[k][3] >= 0.0f) || !(lut[k][3] <= 3.402823466e38f)) return false;
    return true;
}

struct SoftQuad { float v[4]; };

// logits j0 .. j0 + 3 of the row at z (those >= C read as 0 and are never used)
template <bool VEC>
MRIRT_HD SoftQuad soft_load4(const float* __restrict__ z, uint32_t j0, uint32_t C) {
    SoftQuad q;
    if constexpr (VEC) {
        struct alignas(16) F4 { float x, y, z, w; };
        const F4 t = *reinterpret_cast<const F4*>(z + j0);
        q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) q.v[i] = j0 + i < C ? z[j0 + i] : 0.0f;
    }
    return q;
}

template <bool VEC>
MRIRT_HD void soft_store4(float* __restrict__ dl, uint32_t j0, uint32_t C, const SoftQuad& q) {
    if constexpr (VEC) {
        struct alignas(16) F4 { float x, y, z, w; };
        *reinterpret_cast<F4*>(dl + j0) = F4{ q.v[0], q.v[1], q.v[2], q.v[3] };
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (j0 + i < C) dl[j0 + i] = q.v[i];
    }
}

struct SoftEvent {
    float m;                     // max z
    double S, sigma, om;         // S = sum exp(z_j - m); om = 1 - alpha = exp(-sigma D)
    double c[3];
    float alphaF, cF[3];         // what the fp32 compositor applies
};

// z: the row's C logits; lut: the eight SoftRow.  Returns false where the sample draws no event.
template <bool VEC>
MRIRT_HD bool soft_event(const float* __restrict__ z, uint32_t C, const SoftRow* lut, double D, SoftEvent& ev) {
    float m = -INFINITY;
#pragma clang loop unroll(disable)
    for (uint32_t j0 = 0; j0 < C; j0 += 4) {
        const SoftQuad q = soft_load4<VEC>(z, j0, C);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (j0 + i < C) m = q.v[i] > m ? q.v[i] : m;
    }
    double S = 0.0, sg = 0.0, E0 = 0.0, E1 = 0.0, E2 = 0.0;
#pragma clang loop unroll(disable)
    for (uint32_t j0 = 0; j0 < C; j0 += 4) {
        const SoftQuad q = soft_load4<VEC>(z, j0, C);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t j = j0 + i;
            if (j < C) {
                const double e = exp((double)q.v[i] - (double)m);
                S += e;
                if (j >= 1 && j < kSoftDrawn) {
                    const SoftRow r = lut[j];
                    sg += e * r.w; E0 += e * r.wr; E1 += e * r.wg; E2 += e * r.wb;
                }
            }
        }
    }
    ev.m = m;
    ev.S = S;
    ev.sigma = sg / S;
    if (!(ev.sigma > 0.0)) return false;
    ev.om = exp(-ev.sigma * D);
    ev.c[0] = E0 / sg; ev.c[1] = E1 / sg; ev.c[2] = E2 / sg;      // E / sigma: the common 1 / S cancels
    ev.alphaF = (float)(1.0 - ev.om);
    ev.cF[0] = (float)ev.c[0]; ev.cF[1] = (float)ev.c[1]; ev.cF[2] = (float)ev.c[2];
    return true;
}

// the event on the ray's fp32 state, in composite()'s order of operations
MRIRT_HD void soft_apply(const SoftEvent& ev, float& C0, float& C1, float& C2, float& T) {
    const float at = ev.alphaF * T;
    C0 += at * ev.cF[0]; C1 += at * ev.cF[1]; C2 += at * ev.cF[2];
    T *= (1.0f - ev.alphaF);
}

// dlogits of the event's row -> dl[0 .. C): T in front of the event, G = dL/dC of the pixel, gR = G . R.
template <bool VEC>
MRIRT_HD void soft_grad(const SoftEvent& ev, const float* __restrict__ z, uint32_t C, const SoftRow* lut, double D, double T,
                        const double G[3], double gR, float* __restrict__ dl) {
    const double gc = (G[0] * ev.c[0] + G[1] * ev.c[1]) + G[2] * ev.c[2];
    const double dA = ev.om * T * gc - gR;                         // dL/dalpha (1 - alpha)
    const double Ta = T * (1.0 - ev.om);                           // dL/dc = Ta G
    // the drawn classes (two quads): p_k, dL/dp_k and their mean
    double pk[kSoftDrawn], dp[kSoftDrawn], mean = 0.0;
#pragma unroll
    for (uint32_t j0 = 0; j0 < kSoftDrawn; j0 += 4) {
        if (j0 < C) {
            const SoftQuad q = soft_load4<VEC>(z, j0, C);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t k = j0 + i;
                pk[k] = 0.0; dp[k] = 0.0;
                if (k < C) {
                    pk[k] = exp((double)q.v[i] - (double)ev.m) / ev.S;
                    if (k >= 1) {
                        const SoftRow r = lut[k];
                        const double gk = (G[0] * r.wr + G[1] * r.wg) + G[2] * r.wb;      // w_k (G . rgb_k)
                        dp[k] = r.w * D * dA + Ta * (gk - r.w * gc) / ev.sigma;
                        mean += pk[k] * dp[k];
                    }
                }
            }
        }
    }
#pragma unroll
    for (uint32_t j0 = 0; j0 < kSoftDrawn; j0 += 4) {
        if (j0 < C) {
            SoftQuad o;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) o.v[i] = (float)(pk[j0 + i] * (dp[j0 + i] - mean));
            soft_store4<VEC>(dl, j0, C, o);
        }
    }
    // classes >= 8: probability mass only
#pragma clang loop unroll(disable)
    for (uint32_t j0 = kSoftDrawn; j0 < C; j0 += 4) {
        const SoftQuad q = soft_load4<VEC>(z, j0, C);
        SoftQuad o;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            o.v[i] = j0 + i < C ? (float)((exp((double)q.v[i] - (double)ev.m) / ev.S) * (0.0 - mean)) : 0.0f;
        soft_store4<VEC>(dl, j0, C, o);
    }
}

// a row without an event
template <bool VEC>
MRIRT_HD void soft_zero_row(float* __restrict__ dl, uint32_t C) {
    const SoftQuad o = { { 0.0f, 0.0f, 0.0f, 0.0f } };
    for (uint32_t j0 = 0; j0 < C; j0 += 4) soft_store4<VEC>(dl, j0, C, o);
}

}  // namespace mrirt
