// The host-side seam between the K1 units: what brats_march.hip (the march, its plan and prepare()), brats_skip.hip (the
// skipping pre-pass), brats_c5.hip (the per-sample INR render), brats_slab.hip / brats_ring.hip (the LDS marches) and
// inr_mlp.hip (the INR forward's host side; its kernels: inr_fwd.h) call across translation units.  tests/native/index_harness.hip reaches prepare() through this header.
#pragma once
#include "brats_device.h"

namespace mrirt {

// what prepare() decodes of MrirtRenderExt besides the kernel arguments (kernelVariant: see prepare(), brats_march.hip)
struct Prepared { uint32_t layout, math; bool shade, pipe, slab, ring, leap, tag; };

// brats_march.hip: validate + fill the kernel arguments shared by every K1 and C5 entry point
int prepare(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
            const void* labels, const void* preds, bool needVolumes, int64_t pitch_px,
            K1Args& a, Prepared& cfg);

// One launch of a register-gather march kernel (brats_march.hip, brats_tf.hip): the grid and the workgroup size of prepare()'s
// pixel map, `lds` bytes of dynamic shared memory.  args: the kernel's parameters, K1Args first.
inline int launch_k1(const void* kernel, const K1Args& a, void** args, size_t lds, hipStream_t s) {
    const dim3 grid(a.map.chunk * kXcds), block(a.map.blockPx == 8 ? 64 : 256);
    MRIRT_HIP(hipLaunchKernel(kernel, grid, block, args, lds, s));
    return MRIRT_OK;
}

// brats_skip.hip: the pre-pass of a skipping launch.  Builds the empty-radius map of `a`'s configuration in skip->mask
// on `s` (unless skip->mapReady: the caller vouches that the scratch already holds it) and points a.skipDist / a.mX,
// mXY, mY, mZ at it.
int launch_skip_prepass(const MrirtBratsParams* p, const MrirtSkip* skip, bool strict, hipStream_t s, K1Args& a);

// brats_order.hip: the builder of the dispatch order (k1_order.h), launched ahead of a march whose a.map.order / a.map.steps
// are bound: the table from the record of the last frame, and the record zeroed for this one.  A weak reference: host-only
// programs that link brats_march.hip without this unit (tests/native/index_harness.hip) still link, and an ordered launch
// there is refused (MRIRT_ERR_ARG) rather than run without its builder.
__attribute__((weak)) int launch_order_build(const K1Args& a, uint32_t classes, hipStream_t s);

// brats_slab.hip: the LDS-staged march (VGA layout, one modality, no overlays), selected by brats_march.hip
int launch_slab_march(const K1Args& a, bool strict, bool shade, hipStream_t s);
// brats_ring.hip: the plane-synchronous LDS ring march (same launches)
int launch_ring_march(const K1Args& a, bool strict, bool shade, hipStream_t s);

// inr_mlp.hip: the MLP forward with the point count in device memory (argmax only); segTicket: nullptr, or a zeroed device
// word the near-tie refinement deals its segments with
int inr_forward_dev_n(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t nMax,
                      const uint32_t* nDev, int16_t* argmax, uint32_t* segTicket, hipStream_t s);

// brats_c5.hip: the chunked C5 frame.  Its scratch as c5_carve lays it out, and its frame loop, shared by
// mrirt_render_brats_inr and mrirt_render_brats_inject (csrc/inr_inject_fused.hip): the two differ only in the classifier a
// pass enqueues -- classify(sc, pass, stream, ctx) -> status, over sc.coords / sc.feats with the batch size at
// sc.counters + pass, writing sc.classes.
struct C5Ray;
struct C5Scratch { uint32_t* counters; C5Ray* rays; float4* geom; uint2* rowOwner; float* coords; float* feats; float* mix; uint32_t* seg; int16_t* classes; int64_t cap, bytes; };
constexpr uint32_t kC5MaxPasses = 1024;
typedef int (*C5Classify)(const C5Scratch& sc, uint32_t pass, hipStream_t s, const void* ctx);
// what both entry points refuse of their common arguments before they look at their network
int c5_check_common(const MrirtRenderExt* ext, const void* const vol[4], const float* zmu, const float* zsigma, const void* scratch,
                    const void* out_rgba);
// The network was checked by the caller; everything else is refused here, before anything touches the scratch.  maxCap: the
// largest batch capacity (image x chunk_steps) the classifier takes.
int c5_frame(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4], const void* labels, const float zmu[4],
             const float zsigma[4], uint32_t chunk_steps, void* scratch, int64_t scratch_bytes, void* out_rgba, int64_t pitch_px,
             uint64_t* stats_dev, void* stream, int64_t maxCap, C5Classify classify, const void* ctx);

}  // namespace mrirt
