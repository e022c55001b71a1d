// What ONE sample of a K1 ray contributes to the backward pass (brats_backward.hip): the derivative chain of the transfer
// function + emission-absorption step, and the eight corners of the sample's trilinear cell with their weights and clamped
// LINEAR indices.  MRIRT_HD: the kernel runs it per lane, tests/native/brats_grad_harness.hip walks the same functions on the
// CPU under AddressSanitizer + UBSan against buffers of exactly the volume's size (as mesh_trace.h, edt_line.h, surface_cells.h).
//
// The function differentiated is the forward's (brats_rt.slang:117-165, composite() of brats_device.h), per step with
// D = stepSize, a = intensityAlpha, g = gamma:
//     v = sum_m w_m s_m / wSum      u = (v - (wl - ww/2)) / ww      val = pow(sat(u), g)
//     alpha = 1 - exp(-val a D)     C += alpha T val               T *= 1 - alpha          (only where val > 0)
// With L = sum_p G[p] . C[p], g1 = G_r + G_g + G_b and R = the colour every LATER event of the ray adds (label overlays of
// this step included; all of it is proportional to this event's 1 - alpha):
//     dL/dval = T g1 (alpha + val a D (1 - alpha)) - a D (G . R)
//     dL/da   = (T val g1 (1 - alpha) - G . R) val D
//     0 < u < 1:  dval/du = g val / u,  dval/dg = val ln u        (both 0 where u is saturated)
//     du/dv = 1 / ww,  du/dwl = -1 / ww,  du/dww = -(v - wl) / ww^2
//     dL/ds_m = dL/dv w_m / wSum, scattered to the cell's corners with the trilinear weights
// (docs/DifferentiableRendering.md:83-127 of the reference, specialised to K1).  The sample positions, cells, fractions and
// the march's t < t1 / T > ert decisions are the forward's own fp32 values and carry no gradient; this arithmetic is not
// under the STRICT contract and runs in fp64.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mrirt_device.h"

namespace mrirt {

// the launch constants of the chain, as MrirtBratsParams holds them
struct GradTf {
    float ww, wl, intensityAlpha, gamma, stepSize;
    float wsum;          // sum of the enabled volWeight in slot order (the forward normalises only when it is > 0)
};

struct GradSample {
    double dv;                      // dL/dv
    double dww, dwl, da, dgamma;    // this sample's terms of grad_tf
};

// v: the normalised weighted intensity (fp32, the forward's); T: the ray's transmittance in front of the event; g1 = G_r + G_g + G_b;
// gR = G . R.  Returns false where the forward composites nothing (val <= 0; a NaN sample saturates to 0 as in the shader).
MRIRT_HD bool grad_sample(const GradTf& k, float v, float T, double g1, double gR, GradSample& o) {
    o.dv = 0.0; o.dww = 0.0; o.dwl = 0.0; o.da = 0.0; o.dgamma = 0.0;
    const double ww = (double)k.ww, wl = (double)k.wl, dt = (double)k.stepSize, gam = (double)k.gamma;
    const double u = ((double)v - (wl - 0.5 * ww)) / ww;
    if (!(u > 0.0)) return false;
    const bool sat = u >= 1.0;
    const double lnu = sat ? 0.0 : log(u);
    const double val = sat ? 1.0 : (k.gamma == 1.0f ? u : exp(gam * lnu));
    const double ad = (double)k.intensityAlpha * dt;
    const double om = exp(-val * ad);                    // 1 - alpha
    const double alpha = 1.0 - om;
    const double Tg = (double)T * g1;
    const double dval = Tg * (alpha + val * ad * om) - ad * gR;
    o.da = (Tg * val * om - gR) * val * dt;
    if (!sat) {
        const double du = dval * gam * val / u;
        o.dgamma = dval * val * lnu;
        o.dv = du / ww;
        o.dwl = -o.dv;
        o.dww = -du * ((double)v - wl) / (ww * ww);
    }
    return true;
}

// dL/ds_m of one modality from dL/dv (the forward divides by wSum only when it is positive)
MRIRT_HD double grad_modality(const GradTf& k, double dv, float weight) {
    return k.wsum > 0.0f ? dv * (double)weight / (double)k.wsum : dv * (double)weight;
}

// The 2x2x2 cell of sampleLinear (brats_rt.slang:60-76) in trilerp()'s corner order c000, c100, c010, c110, c001, ...: LINEAR
// element indices (x fastest) and the weights of the nested lerp a + t (b - a).  The forward's clamp (dims - 1.001) keeps
// ix <= X - 2; the clamps here hold for ANY input, so an index is always inside the X Y Z elements of the grid.
struct GradCorners {
    uint32_t idx[8];
    float w[8];
};

MRIRT_HD uint32_t grad_clamp_index(uint32_t i, uint32_t n) { return i < n ? i : n - 1u; }

MRIRT_HD void grad_corners(uint32_t ix, uint32_t iy, uint32_t iz, float fx, float fy, float fz,
                           uint32_t X, uint32_t Y, uint32_t Z, GradCorners& c) {
    const uint32_t x0 = grad_clamp_index(ix, X), x1 = grad_clamp_index(x0 + 1u, X);
    const uint32_t y0 = grad_clamp_index(iy, Y), y1 = grad_clamp_index(y0 + 1u, Y);
    const uint32_t z0 = grad_clamp_index(iz, Z), z1 = grad_clamp_index(z0 + 1u, Z);
    const uint32_t r00 = (z0 * Y + y0) * X, r10 = (z0 * Y + y1) * X, r01 = (z1 * Y + y0) * X, r11 = (z1 * Y + y1) * X;
    c.idx[0] = r00 + x0; c.idx[1] = r00 + x1; c.idx[2] = r10 + x0; c.idx[3] = r10 + x1;
    c.idx[4] = r01 + x0; c.idx[5] = r01 + x1; c.idx[6] = r11 + x0; c.idx[7] = r11 + x1;
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    c.w[0] = gx * gy * gz; c.w[1] = fx * gy * gz; c.w[2] = gx * fy * gz; c.w[3] = fx * fy * gz;
    c.w[4] = gx * gy * fz; c.w[5] = fx * gy * fz; c.w[6] = gx * fy * fz; c.w[7] = fx * fy * fz;
}

}  // namespace mrirt
