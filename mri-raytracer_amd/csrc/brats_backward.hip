// K1 backward: dL/d(voxel) of every enabled modality and dL/d(ww, wl, intensityAlpha, gamma) of one frame of brats_main on
// LINEAR fp32 grids, unshaded (mrirt_render_brats_backward, include/mrirt.h; the per-sample chain: brats_grad.h).
//
// One lane = one ray, one wave = an 8 x 8 pixel packet, as the generic march (brats_march.hip).  Every ray marches twice inside
// the one launch, both times with the forward's own code (setup_ray, locate, Taps<0, false>, composite: STRICT), so the
// samples, the steps taken and T in front of every step are the forward's bits:
//   march 1  the forward loop; leaves C_final and nothing else;
//   march 2  the same loop again; in front of every step it composites the intensity event alone on a copy of the ray's state,
//            which gives the colour behind that event, hence R = C_final - C_behind: all the chain needs.  Nothing per sample is stored.
// Voxel gradients go out as float atomicAdd (one global_atomic_add_f32 each: the hardware add, no compare-and-swap loop); a lane
// whose dL/dv is exactly 0 issues none.  The four transfer-function sums stay in registers (fp64), are reduced across the wave and
// cost one fp64 atomicAdd per wave and scalar.  A ray that misses the box, has t1 <= t0 or G == 0 in all three channels leaves at once.
#include "brats_grad.h"
#include "brats_host.h"

namespace mrirt {

struct BackwardArgs {
    const float4* grad;            // dL/dC per pixel (RGBA; alpha ignored), pitch = K1Args::map.pitch
    float* gradVol[4];             // += ; nullptr: not wanted (or disabled)
    double* gradTf;                // += (ww, wl, intensityAlpha, gamma); nullptr: not wanted
    GradTf tf;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void brats_backward_kernel(const K1Args a, const BackwardArgs b) {
    __shared__ float4 lutShared[16];
    const float4* lutS = stage_lut(a, lutShared);
    uint32_t px, py;
    int64_t gidx;
    const int kind = map_pixel(a.map, px, py, gidx);
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    bool marches = kind == 1 && setup_ray(a, px, py, ro, rd, t0, t1);
    float4 G = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (marches) G = b.grad[gidx];
    marches = marches && (G.x != 0.0f || G.y != 0.0f || G.z != 0.0f);
    double sWw = 0.0, sWl = 0.0, sA = 0.0, sGam = 0.0;
    if (marches) {
        const float g[3] = { 0.0f, 0.0f, 0.0f };
        const Labels none = { 0u, 0u };
        // march 1: the forward
        RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
        float t = t0;
        while (t < t1 && r.T > a.ert) {
            Cell s;
            locate<true>(a, ro, rd, t, s);
            const float v = blend_modalities(a, s);
            Labels lb;
            fetch_labels(a, s, lb);
            composite<true, false>(a, rd, lb, v, g, r, lutS);
            t += a.stepSize;
        }
        const float cf0 = r.C0, cf1 = r.C1, cf2 = r.C2;
        // march 2: the same steps, each with its derivatives
        const double g1 = ((double)G.x + (double)G.y) + (double)G.z;
        r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
        t = t0;
        while (t < t1 && r.T > a.ert) {
            Cell s;
            locate<true>(a, ro, rd, t, s);
            const float v = blend_modalities(a, s);
            Labels lb;
            fetch_labels(a, s, lb);
            RayState ri = r;                                             // the intensity event alone: the colour behind it
            composite<true, false>(a, rd, none, v, g, ri, lutS);
            const double gR = ((double)G.x * ((double)cf0 - (double)ri.C0) + (double)G.y * ((double)cf1 - (double)ri.C1)) +
                              (double)G.z * ((double)cf2 - (double)ri.C2);
            const float vn = b.tf.wsum > 0.0f ? (float)((double)v / (double)b.tf.wsum) : v;
            GradSample gs;
            if (grad_sample(b.tf, vn, r.T, g1, gR, gs)) {
                sWw += gs.dww; sWl += gs.dwl; sA += gs.da; sGam += gs.dgamma;
                if (gs.dv != 0.0) {
                    GradCorners c;
                    grad_corners(s.ix, s.iy, s.iz, s.fx, s.fy, s.fz, a.grid.X, a.grid.Y, a.grid.Z, c);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        if (a.enabled[m] != 0 && b.gradVol[m] != nullptr) {          // uniform
                            const double ds = grad_modality(b.tf, gs.dv, a.weight[m]);
#pragma unroll
                            for (int k = 0; k < 8; ++k) atomicAdd(b.gradVol[m] + c.idx[k], (float)(ds * (double)c.w[k]));
                        }
                    }
                }
            }
            composite<true, false>(a, rd, lb, v, g, r, lutS);
            t += a.stepSize;
        }
    }
    if (b.gradTf != nullptr && __ballot(marches) != 0) {                         // every lane of the wave takes part
        sWw = wave_sum(sWw); sWl = wave_sum(sWl); sA = wave_sum(sA); sGam = wave_sum(sGam);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(b.gradTf + 0, sWw);
            atomicAdd(b.gradTf + 1, sWl);
            atomicAdd(b.gradTf + 2, sA);
            atomicAdd(b.gradTf + 3, sGam);
        }
    }
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_render_brats_backward(const MrirtBratsParams* p, const MrirtRenderExt* ext,
                                           const float* const vol[4], const uint32_t* labels, const uint32_t* preds,
                                           const float* grad_rgba, int64_t grad_pitch_px,
                                           float* const grad_vol[4], double* grad_tf, void* stream) {
    if (!p || !vol || !grad_rgba) return MRIRT_ERR_NULL;
    if (ext) {
        // one layout, no shading, whole frames, the STRICT march (the function differentiated is the one the forward executed)
        if (ext->layout != MRIRT_LAYOUT_LINEAR || ext->labelLayout != MRIRT_LAYOUT_LINEAR) return MRIRT_ERR_LAYOUT;
        if (ext->shadeMode != 0 || ext->tileSize != 0 || ext->outFormat != MRIRT_OUT_RGBA32F || ext->math != MRIRT_MATH_STRICT)
            return MRIRT_ERR_ARG;
    }
    const void* v[4] = { vol[0], vol[1], vol[2], vol[3] };
    K1Args a;
    Prepared cfg;
    const int rc = prepare(p, ext, v, labels, preds, true, grad_pitch_px, a, cfg);
    if (rc != MRIRT_OK) return rc;
    if (p->showPred != 0 && !preds) return MRIRT_ERR_NULL;
    BackwardArgs b;
    bool any = grad_tf != nullptr;
    for (int m = 0; m < 4; ++m) {
        b.gradVol[m] = (grad_vol && p->volEnabled[m] != 0) ? grad_vol[m] : nullptr;
        any = any || b.gradVol[m] != nullptr;
    }
    if (!any) return MRIRT_OK;                                         // nothing asked for
    b.grad = reinterpret_cast<const float4*>(grad_rgba);
    b.gradTf = grad_tf;
    b.tf.ww = p->ww; b.tf.wl = p->wl; b.tf.intensityAlpha = p->intensityAlpha; b.tf.gamma = p->gamma;
    b.tf.stepSize = p->stepSize; b.tf.wsum = a.wsum.d;
    const dim3 grid(a.map.chunk * kXcds), block(a.map.blockPx == 8 ? 64 : 256);
    void* args[] = { &a, &b };
    MRIRT_HIP(hipLaunchKernel(reinterpret_cast<const void*>(&brats_backward_kernel), grid, block, args, 0,
                              static_cast<hipStream_t>(stream)));
    return MRIRT_OK;
}
