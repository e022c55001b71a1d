// K1 with an RGBA transfer-function table: mrirt_render_brats_tf (include/mrirt.h).
//
// The march of brats_march.hip — ray set-up, sampleLinear's cell, the layouts' gathers (Taps), the label fetches, compositing
// (composite(): window, level, gamma, shading, overlays), the frame store and the counters are its code, shared through
// brats_device.h, and the pipeline's Stage is its Stage, shared through brats_stage.h — with composite()'s grey ramp replaced
// by a lookup in an N x (r, g, b, sigma) table: TableEvent (brats_tf.h), the EVENT of composite() and of Stage.  The table sits
// in LDS: dynamic shared memory of 16 N bytes per workgroup (N <= 1024: 16 KiB), filled once with coalesced 16-byte loads next
// to the overlay rows of stage_lut, one barrier for both.
//
// What is this unit's own: stage_tf, the two kernels' loops, the choice of pipelined against generic, and the entry point's
// checks.  Two kernel families: brats_tf_kernel<STRICT, LAYOUT, SHADE> — gathers issued and consumed per step, any subset of the
// four modalities, 64-bit offsets: every layout — and brats_tf_pipe_kernel<STRICT, LAYOUT, CELLS>, the two-stage software pipeline
// for the two viewer configurations (below; kernelVariant bit 2 keeps a launch on the generic kernel).  No skipping, no dispatch
// order, no class stream.  (The loops are brats_march_kernel's and brats_march_pipe_kernel's, restated: as device functions
// shared with those kernels they moved the code of most of them — DESIGN.md section 22.)
#include "brats_host.h"
#include "brats_stage.h"
#include "brats_tf.h"

namespace mrirt {

template <bool STRICT, int LAYOUT, bool SHADE>
__global__ __launch_bounds__(256) void brats_tf_kernel(const K1Args a, const TfTable tf) {
    using Mm = M<STRICT>;
    constexpr bool kMod4 = LAYOUT == MRIRT_LAYOUT_MOD4;
    static_assert(!((kMod4 || LAYOUT == MRIRT_LAYOUT_QUAD) && SHADE), "QUAD and MOD4 grids carry no gradients");
    extern __shared__ float4 tfShared[];
    __shared__ float4 lutShared[16];
    stage_tf(tf, tfShared);
    const float4* lutS = stage_lut(a, lutShared);                     // (its barrier covers the table too)
    const TableEvent ev = { tf, tfShared };
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    const bool marches = kind == 1 && setup_ray(a, px, py, ro, rd, t0, t1);
    WaveGrid<LAYOUT> wg;
    if constexpr (LAYOUT == 4) wg.f = a.vga.ax[vga_pick_axis(a, ro, rd, marches)];      // every lane votes: outside the branch
    else wg.g = &a.grid;
    if (marches) {
        float t = t0;
        while (t < t1 && r.T > a.ert) {
            Cell s;
            locate<STRICT>(a, ro, rd, t, s);
            float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
            if constexpr (kMod4) {
                // one tap set carries the four modalities (Stage, brats_stage.h): blended in ascending order, enabled ones only
                Taps<2, true> taps;
                float sv[4], rest[3];
                taps.template issue<true>(a.vol[0], a.grid, s);
                taps.template eval<STRICT>(s, sv[0], rest);
                sv[1] = rest[0]; sv[2] = rest[1]; sv[3] = rest[2];
#pragma unroll
                for (int m = 0; m < 4; ++m) if (a.enabled[m] != 0) v = Mm::mad(sv[m], a.weight[m], v);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (a.enabled[m] != 0) {
                        Taps<LAYOUT, SHADE> taps;
                        float sv, gm[3];
                        taps.template issue<true>(wg.base(a.vol[m]), wg.dims(), s);
                        taps.template eval<STRICT>(s, sv, gm);
                        v = Mm::mad(sv, a.weight[m], v);
                        if constexpr (SHADE) {
#pragma unroll
                            for (int k = 0; k < 3; ++k) g[k] = Mm::mad(gm[k], a.weight[m], g[k]);
                        }
                    }
                }
            }
            Labels lb;
            fetch_labels(a, s, lb);
            composite<STRICT, SHADE>(a, rd, lb, v, g, r, lutS, ev);
            t += a.stepSize;
        }
    }
    finish(a, kind, oidx, r);
}

// ---------------------------------------------------------------------------------------
// Pipelined table kernels: the two-stage march of brats_march_pipe_kernel (same order, one static issue site and one counted
// wait per stage, the pipeline filling inside the loop, the drain behind it: explained there) for exactly two configurations,
// each an instance of the plain Stage:
//   MOD4, unshaded, overlays off (CELLS false: 8 gathers) or through label cells (CELLS true: 9): the viewer's frame, config C2;
//   VGA, shaded, one modality, no overlays (8 gathers): config C3.
// TableEvent's lookup sits between a stage's gathers and the other stage's wait and reads LDS only, so it touches lgkmcnt and
// never vmcnt.  STRICT instances are compiled for gamma == 1 (no fp64 pow: registers); any other STRICT gamma takes the generic
// kernel.  tests/test_tf_host.py runs tools/check_async_loads.py's in-flight scan on these kernels (the build gate's own scan
// goes by the plain kernels' name).
// ---------------------------------------------------------------------------------------
template <bool STRICT, int LAYOUT, bool CELLS>
__global__ __launch_bounds__(256, 3) void brats_tf_pipe_kernel(const K1Args a, const TfTable tf) {
    constexpr bool kMod4 = LAYOUT == MRIRT_LAYOUT_MOD4;
    static_assert(kMod4 || (LAYOUT == MRIRT_LAYOUT_VGA && !CELLS), "MOD4 (with or without label cells) or VGA without overlays");
    using PipeStage = Stage<LAYOUT, !kMod4, kMod4 ? 4 : 1, CELLS, false, CELLS, TableEvent>;
    extern __shared__ float4 tfShared[];
    __shared__ float4 lutShared[16];
    stage_tf(tf, tfShared);
    const float4* lutS = stage_lut(a, lutShared);
    const TableEvent ev = { tf, tfShared };
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    const bool marches = kind == 1 && setup_ray(a, px, py, ro, rd, t0, t1) && t0 < t1 && 1.0f > a.ert;   // the while-condition at entry
    WaveGrid<LAYOUT> wg;
    if constexpr (LAYOUT == 4) wg.f = a.vga.ax[vga_pick_axis(a, ro, rd, marches)];      // every lane votes: outside the branch
    else wg.g = &a.grid;
    if (marches) {
        PipeStage A, B;
        constexpr int kN = PipeStage::kLoads;
        float tI = t0;                                           // time of the next sample to ISSUE (the running sum)
        float tA = t0, tB = t0;                                  // time of the sample each stage holds
        uint32_t n = 0;
        while (true) {
            if (n != 0u) {
                A.template arrive<kN>(a);                        // B's kN loads may still be in flight
                A.template consume<STRICT, STRICT>(a, rd, r, lutS, ev);
                if (!(tB < t1 && r.T > a.ert)) break;            // the loop test for the next sample (held by B)
            }
            tA = tI;
            locate<STRICT>(a, ro, rd, tA, A.s);                  // beyond the ray's end the sample is speculative: clamped addresses
            A.issue_async(a, wg);
            tI += a.stepSize;
            if (n != 0u) {
                B.template arrive<kN>(a);
                B.template consume<STRICT, STRICT>(a, rd, r, lutS, ev);
                if (!(tA < t1 && r.T > a.ert)) break;
            }
            tB = tI;
            locate<STRICT>(a, ro, rd, tB, B.s);
            B.issue_async(a, wg);
            tI += a.stepSize;
            n = 1u;
        }
        // the speculative gathers of the stage that was not consumed are still in flight: their destinations must stay
        // untouched until they land
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    finish(a, kind, oidx, r);
}

using TfKernel = void (*)(K1Args, TfTable);

// the pipelined kernel of a launch, or nullptr: the launch takes the generic kernel
template <bool STRICT>
static TfKernel tf_pipe_kernel(const K1Args& a, const Prepared& cfg, uint32_t variant) {
    if ((variant & 4u) != 0u || a.grid.wide != 0 || (STRICT && a.gamma != 1.0f)) return nullptr;
    const bool overlays = a.showSeg != 0 || a.showPred != 0;
    if (cfg.layout == MRIRT_LAYOUT_MOD4 && !cfg.shade) {
        if (!overlays) return brats_tf_pipe_kernel<STRICT, MRIRT_LAYOUT_MOD4, false>;
        if (a.labCell != nullptr) return brats_tf_pipe_kernel<STRICT, MRIRT_LAYOUT_MOD4, true>;
    }
    if (cfg.layout == MRIRT_LAYOUT_VGA && cfg.shade && a.nch == 1 && !overlays) return brats_tf_pipe_kernel<STRICT, MRIRT_LAYOUT_VGA, false>;
    return nullptr;
}

template <bool STRICT>
static TfKernel tf_kernel(uint32_t layout, bool shade) {
    switch (layout) {                                               // (QUAD and MOD4 launches are unshaded: checked by the caller)
        case MRIRT_LAYOUT_LINEAR: return shade ? brats_tf_kernel<STRICT, 0, true> : brats_tf_kernel<STRICT, 0, false>;
        case MRIRT_LAYOUT_BRICK:  return shade ? brats_tf_kernel<STRICT, 1, true> : brats_tf_kernel<STRICT, 1, false>;
        case MRIRT_LAYOUT_VG:     return shade ? brats_tf_kernel<STRICT, 2, true> : brats_tf_kernel<STRICT, 2, false>;
        case MRIRT_LAYOUT_QUAD:   return brats_tf_kernel<STRICT, 3, false>;
        case MRIRT_LAYOUT_VGA:    return shade ? brats_tf_kernel<STRICT, 4, true> : brats_tf_kernel<STRICT, 4, false>;
        case MRIRT_LAYOUT_MOD4:   return brats_tf_kernel<STRICT, MRIRT_LAYOUT_MOD4, false>;
        default: return nullptr;
    }
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_render_brats_tf(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                     const void* labels, const void* preds, const float* tf_rgba, uint32_t tf_entries,
                                     void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream) {
    if (!tf_rgba) return MRIRT_ERR_NULL;
    if (tf_entries < kTfMinEntries || tf_entries > kTfMaxEntries) return MRIRT_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(tf_rgba) & 15u) != 0) return MRIRT_ERR_ARG;       // rows are read as 16-byte loads
    if (ext && (ext->kernelVariant & ~6u) != 0) return MRIRT_ERR_ARG;                  // bit 1: workgroup flip; bit 2: the generic table kernel
    K1Args a;
    Prepared cfg;
    const int rc = prepare(p, ext, vol, labels, preds, true, pitch_px, a, cfg);
    if (rc != MRIRT_OK) return rc;
    if (p->showPred != 0 && !preds && a.labCell == nullptr) return MRIRT_ERR_NULL;
    if (a.map.numBlocks == 0) return MRIRT_OK;                      // a rank that owns no tile launches nothing
    if ((cfg.layout == MRIRT_LAYOUT_QUAD || cfg.layout == MRIRT_LAYOUT_MOD4) && cfg.shade) return MRIRT_ERR_LAYOUT;
    if (!out_rgba) return MRIRT_ERR_NULL;
    const bool strict = cfg.math == MRIRT_MATH_STRICT;
    const uint32_t variant = ext ? ext->kernelVariant : 0u;
    TfKernel k = strict ? tf_pipe_kernel<true>(a, cfg, variant) : tf_pipe_kernel<false>(a, cfg, variant);
    if (k == nullptr) k = strict ? tf_kernel<true>(cfg.layout, cfg.shade) : tf_kernel<false>(cfg.layout, cfg.shade);
    if (k == nullptr) return MRIRT_ERR_LAYOUT;
    a.out = out_rgba;
    a.stats = stats_dev;
    TfTable tf;
    tf.rows = reinterpret_cast<const float4*>(tf_rgba);
    tf.n = tf_entries;
    tf.last = tf_entries - 2u;
    tf.top = (float)(tf_entries - 1u);
    void* args[] = { &a, &tf };
    return launch_k1(reinterpret_cast<const void*>(k), a, args, (size_t)tf_entries * sizeof(float4), static_cast<hipStream_t>(stream));
}
