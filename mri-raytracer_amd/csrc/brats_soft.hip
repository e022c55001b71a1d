// The soft prediction overlay of K1 and its backward pass: one frame of brats_main on LINEAR fp32 grids, unshaded, whose
// prediction-overlay event is driven by per-sample class probabilities (mrirt_render_brats_soft), and dL/dlogits of that frame
// (mrirt_render_brats_soft_backward).  include/mrirt.h states the contract, brats_soft.h holds the per-sample chain.
//
// One lane = one ray, one wave = an 8 x 8 pixel packet, the generic march's pixel map (as brats_backward.hip).  The rays, the
// cells, the intensity event and the ground-truth overlay are the forward's own STRICT code (setup_ray, locate, Taps<0, false>,
// composite with Labels{seg, 0}); the logits of sample k of ray p are row offsets[p] + k, the whole-ray C5 numbering of
// mrirt_brats_sample_counts / mrirt_brats_emit_samples.  The backward marches every ray twice inside the one launch:
//   march 1  the forward loop; leaves C_final and nothing else;
//   march 2  the same loop again; behind every soft event the ray's colour is C_after, hence R = C_final - C_after.  Nothing per
//            sample is stored.  It then keeps stepping t to t1 and writes the zero rows of the steps not taken.
// Every row of a ray that hits the box has exactly one writer (its lane) and is written with `=`: no atomics, the same bits
// from run to run.  A ray's rows are contiguous; a row goes as dwordx4 where C % 4 == 0 (and the buffers are 16-byte aligned).
#include "brats_host.h"
#include "brats_soft.h"

namespace mrirt {

struct SoftArgs {
    const float* logits;           // [rows][C]
    const int64_t* offsets;        // first row of pixel y * width + x
    const float4* grad;            // backward: dL/dC per pixel (alpha ignored), pitch = K1Args::map.pitch
    float* dlogits;                // backward: [rows][C], =
    float stepSize;                // D = stepSize * 1.5 is formed in the kernel (exact in fp64)
    uint32_t C;
};

// w_k and w_k rgb_k next to stage_lut's rows: a per-lane class index into the kernel arguments would be a vector-memory load
// the compiler cannot count past (brats_device.h, stage_lut)
__device__ __forceinline__ const float4* stage_soft(const K1Args& a, float4* lutS, SoftRow* softS) {
    // (row k by lane k with k a constant: scalar loads of the kernel arguments)
#pragma unroll
    for (uint32_t k = 0; k < kSoftDrawn; ++k)
        if (threadIdx.x == k) softS[k] = soft_row(a.lut[k]);
    return stage_lut(a, lutS);                                                 // (its barrier covers both tables)
}

// one step of the frame: the intensity event and the ground-truth overlay (composite), then the soft event of `row`
template <bool VEC>
__device__ __forceinline__ bool soft_step(const K1Args& a, const SoftArgs& b, const float ro[3], const float rd[3], float t, int64_t row,
                                          const float4* lutS, const SoftRow* softS, RayState& r, SoftEvent& ev) {
    const float g[3] = { 0.0f, 0.0f, 0.0f };
    Cell s;
    locate<true>(a, ro, rd, t, s);
    const float v = blend_modalities(a, s);
    Labels lb;
    fetch_labels(a, s, lb);                                                      // (a.showPred == 0: lb.pred = 0)
    composite<true, false>(a, rd, lb, v, g, r, lutS);
    return soft_event<VEC>(b.logits + row * (int64_t)b.C, b.C, softS, (double)b.stepSize * 1.5, ev);
}

template <bool VEC>
__global__ __launch_bounds__(256) void brats_soft_kernel(const K1Args a, const SoftArgs b) {
    __shared__ float4 lutShared[16];
    __shared__ SoftRow softShared[kSoftDrawn];
    const float4* lutS = stage_soft(a, lutShared, softShared);
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    if (kind == 1 && setup_ray(a, px, py, ro, rd, t0, t1)) {
        int64_t row = b.offsets[(int64_t)py * a.map.width + px];
        for (float t = t0; t < t1 && r.T > a.ert; t += a.stepSize, ++row) {
            SoftEvent ev;
            if (soft_step<VEC>(a, b, ro, rd, t, row, lutS, softShared, r, ev)) soft_apply(ev, r.C0, r.C1, r.C2, r.T);
        }
    }
    if (kind != 0) store_rgba<false>(a.out, oidx, r.C0, r.C1, r.C2, 1.0f);
    if (a.stats != nullptr) wave_count_add(a.stats, r.nLive);
}

template <bool VEC>
__global__ __launch_bounds__(256) void brats_soft_backward_kernel(const K1Args a, const SoftArgs b) {
    __shared__ float4 lutShared[16];
    __shared__ SoftRow softShared[kSoftDrawn];
    const float4* lutS = stage_soft(a, lutShared, softShared);
    uint32_t px, py;
    int64_t gidx;
    const int kind = map_pixel(a.map, px, py, gidx);
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    if (kind != 1 || !setup_ray(a, px, py, ro, rd, t0, t1)) return;              // a ray that misses owns no rows
    const int64_t row0 = b.offsets[(int64_t)py * a.map.width + px];
    const float4 Gf = b.grad[gidx];
    bool alive = Gf.x != 0.0f || Gf.y != 0.0f || Gf.z != 0.0f;                    // G == 0: the ray's rows are zeros
    float cf0 = 0.0f, cf1 = 0.0f, cf2 = 0.0f;
    if (alive) {
        // march 1: the forward
        RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
        int64_t row = row0;
        for (float t = t0; t < t1 && r.T > a.ert; t += a.stepSize, ++row) {
            SoftEvent ev;
            if (soft_step<VEC>(a, b, ro, rd, t, row, lutS, softShared, r, ev)) soft_apply(ev, r.C0, r.C1, r.C2, r.T);
        }
        cf0 = r.C0; cf1 = r.C1; cf2 = r.C2;
    }
    // march 2: the same steps, each event with its derivatives; then on to t1 with zero rows
    const double G[3] = { (double)Gf.x, (double)Gf.y, (double)Gf.z };
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    int64_t row = row0;
    for (float t = t0; t < t1; t += a.stepSize, ++row) {
        float* dl = b.dlogits + row * (int64_t)b.C;
        alive = alive && r.T > a.ert;
        bool event = false;
        if (alive) {
            SoftEvent ev;
            event = soft_step<VEC>(a, b, ro, rd, t, row, lutS, softShared, r, ev);
            if (event) {
                const double T = (double)r.T;                                    // in front of the soft event
                soft_apply(ev, r.C0, r.C1, r.C2, r.T);
                const double gR = (G[0] * ((double)cf0 - (double)r.C0) + G[1] * ((double)cf1 - (double)r.C1)) +
                                  G[2] * ((double)cf2 - (double)r.C2);
                soft_grad<VEC>(ev, b.logits + row * (int64_t)b.C, b.C, softShared, (double)b.stepSize * 1.5, T, G, gR, dl);
            }
        }
        if (!event) soft_zero_row<VEC>(dl, b.C);
    }
}

// the checks both entry points share; fills the kernel arguments
static int soft_prepare(const MrirtBratsParams* p, const MrirtRenderExt* ext, const float* const vol[4], const uint32_t* labels,
                        const float* logits, uint32_t num_classes, const int64_t* offsets, const void* frame, int64_t pitch_px,
                        K1Args& a, SoftArgs& b) {
    if (!p || !vol || !logits || !offsets || !frame) return MRIRT_ERR_NULL;
    if (ext) {
        // one layout, no shading, whole frames, the STRICT march (as mrirt_render_brats_backward)
        if (ext->layout != MRIRT_LAYOUT_LINEAR || ext->labelLayout != MRIRT_LAYOUT_LINEAR) return MRIRT_ERR_LAYOUT;
        if (ext->shadeMode != 0 || ext->tileSize != 0 || ext->outFormat != MRIRT_OUT_RGBA32F || ext->math != MRIRT_MATH_STRICT)
            return MRIRT_ERR_ARG;
    }
    if (num_classes < 1 || num_classes > kSoftMaxClasses) return MRIRT_ERR_ARG;
    if (!soft_lut_ok(p->lutColorAlpha)) return MRIRT_ERR_ARG;
    const void* v[4] = { vol[0], vol[1], vol[2], vol[3] };
    Prepared cfg;
    const int rc = prepare(p, ext, v, labels, nullptr, true, pitch_px, a, cfg);
    if (rc != MRIRT_OK) return rc;
    a.showPred = 0;                                                   // the soft event takes the prediction overlay's place
    b.logits = logits; b.offsets = offsets; b.grad = nullptr; b.dlogits = nullptr;
    b.stepSize = p->stepSize;
    b.C = num_classes;
    return MRIRT_OK;
}

static bool soft_vec(uint32_t C, const void* x, const void* y) {
    return C % 4 == 0 && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_render_brats_soft(const MrirtBratsParams* p, const MrirtRenderExt* ext, const float* const vol[4],
                                       const uint32_t* labels, const float* logits, uint32_t num_classes, const int64_t* offsets,
                                       float* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream) {
    K1Args a;
    SoftArgs b;
    const int rc = soft_prepare(p, ext, vol, labels, logits, num_classes, offsets, out_rgba, pitch_px, a, b);
    if (rc != MRIRT_OK) return rc;
    a.out = out_rgba; a.stats = stats_dev;
    const dim3 grid(a.map.chunk * kXcds), block(a.map.blockPx == 8 ? 64 : 256);
    void* args[] = { &a, &b };
    const void* fn = soft_vec(num_classes, logits, logits) ? reinterpret_cast<const void*>(&brats_soft_kernel<true>)
                                                           : reinterpret_cast<const void*>(&brats_soft_kernel<false>);
    MRIRT_HIP(hipLaunchKernel(fn, grid, block, args, 0, static_cast<hipStream_t>(stream)));
    return MRIRT_OK;
}

extern "C" int mrirt_render_brats_soft_backward(const MrirtBratsParams* p, const MrirtRenderExt* ext, const float* const vol[4],
                                                const uint32_t* labels, const float* logits, uint32_t num_classes,
                                                const int64_t* offsets, const float* grad_rgba, int64_t grad_pitch_px,
                                                float* dlogits, void* stream) {
    if (!dlogits) return MRIRT_ERR_NULL;
    K1Args a;
    SoftArgs b;
    const int rc = soft_prepare(p, ext, vol, labels, logits, num_classes, offsets, grad_rgba, grad_pitch_px, a, b);
    if (rc != MRIRT_OK) return rc;
    b.grad = reinterpret_cast<const float4*>(grad_rgba);
    b.dlogits = dlogits;
    const dim3 grid(a.map.chunk * kXcds), block(a.map.blockPx == 8 ? 64 : 256);
    void* args[] = { &a, &b };
    const void* fn = soft_vec(num_classes, logits, dlogits) ? reinterpret_cast<const void*>(&brats_soft_backward_kernel<true>)
                                                            : reinterpret_cast<const void*>(&brats_soft_backward_kernel<false>);
    MRIRT_HIP(hipLaunchKernel(fn, grid, block, args, 0, static_cast<hipStream_t>(stream)));
    return MRIRT_OK;
}
