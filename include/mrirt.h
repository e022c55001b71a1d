/* mrirt.h — C ABI of the MI355X-native MRI volume ray-marcher (libmrirt.so).
 *
 * This is the drop-in boundary for the reference's render call.  The reference
 * (klukaszek/MRI-RayTracer) has no FFI of its own: its render call is the third-party slangpy
 *     kernel.dispatch(thread_count=[W,H,1], vars={...}, command_encoder=ce)
 * at inr/viewer/brats_viewer.py:431-442, scripts/volumeRendering/app.py:350-358 and
 * scripts/raymarch/app.py:212-223, binding buffers BY NAME to the Slang globals.  Each entry
 * point below replaces one of those dispatches: same inputs (the Slang cbuffer as a POD, the
 * StructuredBuffers as plain device pointers), same output (one RGBA pixel per thread).
 *
 * Rules of the boundary:
 *   - extern "C", plain pointers and sizes, no torch / C++ types;
 *   - every data pointer is a DEVICE pointer owned by the caller; nothing is retained;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) and NOT synchronised;
 *   - returns MRIRT_OK (0) or a negative MrirtStatus; never throws across the boundary;
 *   - parameter structs are read on the host during the call (they may live on the stack).
 */
#ifndef MRIRT_H
#define MRIRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: MRIRT_LAYOUT_LABCELL + mrirt_build_label_cells, MrirtInrDesc.flags / tieSigmas (they replace the process-environment
 *    switches of version 2), mrirt_brats_skip_applicable, mrirt_install_abort_trace. */
/* 4: MRIRT_LAYOUT_MOD4 + mrirt_build_mod4_grid (the four modalities of a BraTS case as ONE float4 grid: unshaded K1 and
 *    mrirt_render_brats_inr); the packed INR image ends in 32 KiB of slack more (mrirt_inr_pack_bytes says how much to allocate). */
/*    Backward-compatible additions under the same version: MrirtMeshParams + mrirt_render_mesh (K4, the triangle-mesh BVH
 *    ray tracer), mrirt_sizeof(6); mrirt_edt_scratch_bytes, mrirt_edt_squared, mrirt_hausdorff (no new struct);
 *    mrirt_surface_scratch_bytes, mrirt_surface_count, mrirt_surface_extract (no new struct);
 *    mrirt_render_brats_backward (the K1 backward pass on LINEAR grids; no new struct);
 *    mrirt_render_brats_soft, mrirt_render_brats_soft_backward (the soft prediction overlay and its gradient to the
 *    per-sample logits; no new struct);
 *    the INR training loop: MrirtInrCache, MrirtAdamW, MrirtInrTrainCfg, MrirtInrTrainState (mrirt_sizeof(7..10)),
 *    mrirt_inr_sample_batch, mrirt_inr_adamw_scratch_bytes, mrirt_inr_adamw_step, mrirt_inr_lr_schedule,
 *    mrirt_inr_train_run_scratch_bytes, mrirt_inr_train_run;
 *    SIREN training (no new struct): mrirt_siren_train_scratch_bytes, mrirt_siren_forward_f32, mrirt_siren_backward,
 *    mrirt_siren_train_run_scratch_bytes, mrirt_siren_train_run;
 *    Muon: MrirtMuon (mrirt_sizeof(11)), mrirt_muon_scratch_bytes, mrirt_muon_orthogonalize, mrirt_muon_step,
 *    mrirt_inr_train_run_muon_scratch_bytes, mrirt_inr_train_run_muon;
 *    the extended loss and the tumour-ratio sampler: MrirtInrLossExt, MrirtInrTumourIndex, MrirtInrTrainExt
 *    (mrirt_sizeof(13..15)), mrirt_inr_loss_ext_scratch_bytes, mrirt_inr_loss_ext, mrirt_inr_tumour_count,
 *    mrirt_inr_tumour_index_scratch_bytes, mrirt_inr_tumour_index, mrirt_inr_sample_batch_mix,
 *    mrirt_inr_train_run_ext_scratch_bytes, mrirt_inr_train_run_ext;
 *    case preparation (no new struct): mrirt_prep_scratch_bytes, mrirt_prep_window, mrirt_prep_normalize,
 *    mrirt_prep_zscore_scratch_bytes, mrirt_prep_zscore_stats, mrirt_prep_zscore_apply, mrirt_prep_gaussian3d;
 *    connected components (no new struct): mrirt_cc_scratch_bytes, mrirt_cc_label, mrirt_cc_sizes, mrirt_cc_filter,
 *    mrirt_slice_counts;
 *    the coordinate-injection INR: MrirtInjectDesc, MrirtInjectDropout (mrirt_sizeof(17), (18)), mrirt_inject_scratch_bytes,
 *    mrirt_inject_forward, mrirt_inject_uncertainty, mrirt_inject_predict_volume, mrirt_boundary_weights_scratch_bytes,
 *    mrirt_boundary_weights;
 *    its training step (no new struct): mrirt_inject_train_scratch_bytes, mrirt_inject_forward_train, mrirt_inject_backward;
 *    the notebook's unified loss and the samplers' field gather: MrirtUnifiedLoss (mrirt_sizeof(20)),
 *    mrirt_unified_loss_scratch_bytes, mrirt_unified_loss, mrirt_inr_sample_field;
 *    the notebook's hybrid sampler and coordinate noise: MrirtInrClassIndex, MrirtInrHybrid (mrirt_sizeof(22), (23)),
 *    mrirt_inr_class_count, mrirt_inr_class_index_scratch_bytes, mrirt_inr_class_index, mrirt_select_largest,
 *    mrirt_inr_normal3, mrirt_inr_sample_candidates, mrirt_inr_sample_batch_hybrid;
 *    the fused forward of the coordinate-injection INR and the C5 frame driven by it (no new struct):
 *    mrirt_inject_fused_lds_bytes, mrirt_inject_classify, mrirt_render_brats_inject. */
#define MRIRT_ABI_VERSION 4

typedef enum MrirtStatus {
    MRIRT_OK = 0,
    MRIRT_ERR_NULL = -1,       /* a required pointer is NULL                         */
    MRIRT_ERR_DIMS = -2,       /* volume dims < 2 on an axis, or image size 0        */
    MRIRT_ERR_LAYOUT = -3,     /* unknown layout / dtype / mode                      */
    MRIRT_ERR_LAUNCH = -4,     /* hipLaunch / HIP runtime error (see mrirt_last_hip_error) */
    MRIRT_ERR_ARG = -5,        /* inconsistent argument (pitch < width, bad tile spec, ...) */
    MRIRT_ERR_NO_DEVICE = -6   /* no gfx950 device visible                           */
} MrirtStatus;

/* ------------------------------------------------------------------------------------ */
/* K1  brats_main                                                                        */
/* ------------------------------------------------------------------------------------ */

/* Field-for-field mirror of `struct Params`, inr/viewer/brats_rt.slang:12-31, including
 * its hand padding (so the 16-byte cbuffer layout is preserved).                        */
typedef struct MrirtBratsParams {
    uint32_t imageSize[2]; float fovY; float pad0;
    float eye[3]; float pad1;
    float U[3]; float pad2; float V[3]; float pad3; float W[3]; float pad4;
    float volMin[3]; float pad5; float voxelSize[3]; float pad6; uint32_t dims[3]; uint32_t pad7;
    float stepSize; float nearT; float farT; float pad8;
    float bgColor[3]; float pad9;
    uint32_t volEnabled[4];
    float volWeight[4];
    float ww; float wl; float intensityAlpha; float padInt;
    float gamma; float gradBoost; float gradScale; float padTone;   /* gradBoost/gradScale: unread, as in the shader */
    uint32_t showSeg;
    uint32_t showPred;
    uint32_t padFlags[2];
    float lutColorAlpha[8][4];
} MrirtBratsParams;

/* Grid storage layouts.  LINEAR is the reference's (x fastest: x + y*X + z*X*Y,
 * inr/viewer/brats_viewer.py:64).  BRICK is this library's HBM layout (DESIGN.md "Data
 * layout"): 4x4x2-voxel bricks, one 128-byte line per fp32 brick, produced by mrirt_brick_*. */
typedef enum MrirtLayout {
    MRIRT_LAYOUT_LINEAR = 0,
    MRIRT_LAYOUT_BRICK = 1,
    /* fp32 intensity grids only: one float4 per voxel, 2x2x2-voxel bricks (8 x 16 B = one 128-B
     * line).  VG   = (v, dv/dx, dv/dy, dv/dz) with the lattice central differences
     *                v[clamp(c+e)] - v[clamp(c-e)] precomputed at load time (mrirt_build_vec4_grid):
     *                a gradient-shaded sample is 8 dwordx4 gathers instead of 32 dword gathers,
     *                bit-identical arithmetic.
     *        QUAD = (v[x,y], v[x,y+1], v[x+1,y], v[x+1,y+1]) (indices clamped): an unshaded
     *                trilinear sample is 2 dwordx4 gathers instead of 8 dword gathers.          */
    MRIRT_LAYOUT_VG = 2,
    MRIRT_LAYOUT_QUAD = 3,
    /* VGA = the VG voxels stored three times, in 128-B bricks one voxel thick along x, y or z (1x4x2 / 4x1x2 /
     *       4x2x1 voxels).  A ray packet's samples of one march step lie on a sheet parallel to the face the rays
     *       entered through; the kernel reads the copy whose bricks are flat in that direction (chosen per packet),
     *       so a gather touches about half the cache lines of the 2x2x2 bricks.  Same bits as VG; 3x the memory
     *       (6 GiB for a 512^3 channel: sized for 288 GB of HBM).  mrirt_vga_elems / mrirt_build_vec4_grid.        */
    MRIRT_LAYOUT_VGA = 4,
    /* Label grids only (labelLayout), with QUAD intensity grids: BOTH overlays' nearest labels per CELL.  sampleLabel's
     * rounded voxel (brats_rt.slang:78-83) is always one of the eight corners of the cell sampleLinear blends
     * (round(clamp(q, 0, d-1)) - floor(clamp(q, 0, d-1.001)) is 0 or 1 per axis), and the shader draws labels 1..7 only
     * (:145,156), so one 8-byte element per voxel holds what a sample needs of both grids: .x = the ground-truth labels of
     * the cell's corners as eight nibbles (corner (dx,dy,dz) in bits 4 (dx + 2 dy + 4 dz) .., neighbours clamped to the grid,
     * labels >= 8 stored as 8), .y = the prediction's likewise; elements in the QUAD grid's order (mrirt_vec4_elems).  A
     * sample then takes ONE 8-byte gather at the offset its intensity taps already have instead of two nearest-voxel
     * gathers.  mrirt_build_label_cells makes it; `labels` points at it, `preds` is ignored.                              */
    MRIRT_LAYOUT_LABCELL = 5,
    /* MOD4 = the FOUR modalities of one case interleaved: float4 (gIntensity0..3)[voxel] in the VG grid's element order
     *        (2x2x2-voxel bricks of 8 x 16 B, mrirt_vec4_elems).  An unshaded sample of a multi-modality frame — the reference
     *        viewer's own frame, and the per-sample network of mrirt_render_brats_inr — takes eight 16-byte gathers for the eight
     *        corners of ALL four modalities (the same 128 B per sample as four QUAD grids) from a grid a quarter of the size:
     *        268 MB instead of 1.07 GB for 256^3 x 4, one set of cache lines per sample instead of four.  Trilinear arithmetic
     *        unchanged (sampleLinear's order): same bits.  mrirt_build_mod4_grid makes it; vol[0] points at it (vol[1..3] are
     *        ignored); which modalities are drawn stays volEnabled; label grids as before or as MRIRT_LAYOUT_LABCELL.
     *        mrirt_render_brats_ex / _skip (the pipelined march) and mrirt_render_brats_inr.  MRIRT_ERR_LAYOUT with gradient
     *        shading (no gradients in it), with a class stream (mrirt_render_brats_stream), and for grids of 4 GiB or label
     *        grids of 2^30 elements upwards.                                                                                 */
    MRIRT_LAYOUT_MOD4 = 6
} MrirtLayout;

typedef enum MrirtMath {
    MRIRT_MATH_STRICT = 0,  /* unfused fp32 in the oracle's order, fp64-backed exp/pow: bit-faithful */
    MRIRT_MATH_FAST = 1     /* FMA contraction, hardware exp2/rcp; within the 1e-4 image tolerance   */
} MrirtMath;

typedef enum MrirtOutFormat { MRIRT_OUT_RGBA32F = 0, MRIRT_OUT_RGBA16F = 1 /* reference's rgba16_float */ } MrirtOutFormat;

/* Build-defined extensions (no reference counterpart).  A NULL pointer
 * or an all-zero struct selects exactly the reference's behaviour.                         */
typedef struct MrirtRenderExt {
    uint32_t cameraMode;        /* 0 perspective (brats_rt.slang:36-46), 1 orthographic        */
    float    orthoHalfHeight;
    uint32_t shadeMode;         /* 0 off, 1 lattice central-difference gradient + Blinn-Phong  */
    float    ka, kd, ks;
    uint32_t specPow2;          /* specular exponent 2^specPow2 by repeated squaring           */
    float    gradEps;
    uint32_t ertOverride;       /* 0: the reference's T > 0.01; 1: use ertThreshold            */
    float    ertThreshold;
    uint32_t math;              /* MrirtMath                                                   */
    uint32_t outFormat;         /* MrirtOutFormat                                              */
    uint32_t layout;            /* MrirtLayout of ALL bound fp32 intensity grids               */
    uint32_t labelLayout;       /* MrirtLayout (LINEAR, BRICK or LABCELL) of the labels / preds grids */
    /* Image-tile sharding (one process per GPU).  tileSize == 0: whole image into
     * out[y*pitch + x].  Otherwise this call renders the tiles t with t % tileWorld ==
     * tileRank (t = ty*tilesX + tx, tiles of tileSize^2 pixels) into a COMPACT buffer
     * out[local_tile][tileSize][tileSize][4]; pitch is ignored.  Slots of an edge tile that
     * lie outside the image hold the background (K1: bgColor, K2: 0; alpha 1).  A rank that
     * owns no tile (mrirt_tiles_for_rank == 0: tileWorld larger than the number of tiles)
     * launches nothing, counts nothing and returns MRIRT_OK, and since its compact buffer
     * is empty, out_rgba may be NULL for it in the K1 entry points and mrirt_render_volume:
     * a NULL out_rgba is MRIRT_ERR_NULL only where the call has at least one block to write. */
    uint32_t tileSize, tileRank, tileWorld;
    uint32_t kernelVariant;     /* 0 = library default; others select experimental kernels (bench/tests) */
    /* Tile sharding, load balance: the dealt tile t sits at row ty = t / tilesX, column tx = (t % tilesX + tileSkew * ty) % tilesX
     * (0: tx = t % tilesX, the plain row-major deal).  When tilesX is a multiple of tileWorld the plain deal hands every rank
     * whole tile COLUMNS (rank = tx % world); a skew of (tilesX - 1) % tileWorld turns that into diagonals, rank = (tx + ty) % world,
     * so every rank draws from every column and row of the image.  mrirt_detile takes the same value.                         */
    uint32_t tileSkew;
    uint32_t reserved;
} MrirtRenderExt;

/* Argument checks shared by every K1 entry point (MRIRT_ERR_ARG, nothing is launched): stepSize must be a
 * finite positive number that still advances t in fp32 at the far end of the box (t + stepSize > t) and may
 * not cut the box diagonal into more than 2^20 steps; voxelSize finite and > 0; volMin / eye / U / V / W finite, fovY
 * finite in perspective mode (a camera that is not finite makes NaN rays); intensityAlpha not a NaN (the strict exp
 * would turn it into an opacity of 1 where the shader's is NaN).  The
 * reference's UI clamps its slider to >= 0.001 (inr/viewer/brats_viewer.py:168); the shader itself would
 * spin.  K2: stepCount finite and <= 2^20, near / far finite.  K3: maxSteps <= 2^20.                      */

/* Drop-in for kernel.dispatch(...) of brats_main, inr/viewer/brats_viewer.py:431-442.
 *   vol[m]  = gIntensity<m>  (fp32, X*Y*Z, LINEAR; may be NULL when volEnabled[m] == 0)
 *   labels  = gLabels, preds = gPreds (uint32 per voxel; may be NULL when showSeg/showPred == 0)
 *   out_rgba= gOutput as fp32 RGBA, pitch_px pixels per row (>= imageSize[0])             */
int mrirt_render_brats(const MrirtBratsParams* params, const float* const vol[4],
                       const uint32_t* labels, const uint32_t* preds,
                       float* out_rgba, int64_t pitch_px, void* stream);

/* As above with extensions; grids are in ext->layout, out in ext->outFormat.
 * stats_dev (optional): 2 device uint64 counters, atomically incremented by
 * {live samples, gradient-shaded samples} — used for sample accounting, not timed.       */
int mrirt_render_brats_ex(const MrirtBratsParams* params, const MrirtRenderExt* ext,
                          const void* const vol[4], const void* labels, const void* preds,
                          void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);

/* K1 with an RGBA transfer-function table (build-defined extension).  Same arguments and checks as
 * mrirt_render_brats_ex, plus the table: tf_rgba = tf_entries rows of (r, g, b, sigma) fp32 in DEVICE memory, 16-byte
 * aligned, 2 <= tf_entries <= 1024.  Window, level and gamma stay as the table's domain mapping: everything up to
 *   val = pow(saturate((v - (wl - ww/2)) / ww), gamma)                   (brats_rt.slang:132-133)
 * is the plain march; then per sample, with N = tf_entries (STRICT: unfused fp32 in this order; FAST may contract):
 *   u = val * float(N-1);  i = min(uint(floor(u)), N-2);  f = u - float(i)
 *   e[k] = tf[i][k] + f * (tf[i+1][k] - tf[i][k]), k = 0..3;  sigma = e[3];  the sample counts as live
 *   if sigma > 0:  alpha = 1 - exp(-(sigma * intensityAlpha) * stepSize)      (the full-range exp: sigma may exceed 1)
 *                  C[k] += (alpha * T) * (e[k] * shade);  T *= 1 - alpha       (shade = 1 unless shadeMode = 1)
 * Label overlays, t += stepSize and the loop test are unchanged.  The two-entry ramp (0,0,0,0), (1,1,1,1) gives e[k] = val:
 * the frame and the counters of mrirt_render_brats_ex, bit for bit (STRICT).
 *   Intensity layouts: LINEAR, BRICK, VG, VGA shaded or not, 1-4 modalities; QUAD and MOD4 unshaded only (MRIRT_ERR_LAYOUT
 *   with shading, as mrirt_render_brats_ex).  Label layouts: LINEAR, BRICK, LABCELL.  Both cameras, ertOverride, rgba16f
 *   output, tile sharding with tileSkew, STRICT and FAST.
 *   stats_dev (optional) = {live samples, gradient-shaded samples with sigma > 0}.
 *   Refused with nothing launched: tf_rgba NULL -> MRIRT_ERR_NULL; tf_entries < 2 or > 1024, a table that is not 16-byte
 *   aligned, kernelVariant bits other than bit 1 (workgroup flip) and bit 2 -> MRIRT_ERR_ARG.
 *   kernelVariant bit 2 means "the generic table kernel" here: without it MOD4 unshaded launches (overlays off or through
 *   label cells) and VGA shaded one-modality launches without overlays take a software-pipelined table kernel (STRICT: for
 *   gamma == 1; grids below 4 GiB) — the same frame and counters, bit for bit.
 * There is no empty-space skipping (it would need the largest sigma over a cell's val range), no dispatch order and no
 * class stream with a table.                                                                                            */
int mrirt_render_brats_tf(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                          const void* labels, const void* preds,
                          const float* tf_rgba, uint32_t tf_entries,
                          void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);

/* Host CPU twin? No: the product has no CPU fallback.  The CPU restatement lives in oracle/. */

/* Per-sample INR query along the rays (build-defined, BASELINE config 5): the label
 * of the prediction overlay (brats_rt.slang:154-162) comes from an MLP evaluated AT each sample
 * instead of sampleLabel(gPreds).  Three device passes around mrirt_inr_forward:
 *   1. mrirt_brats_sample_counts: counts[y*W + x] = steps ray (x,y) takes in [t0,t1) (no ERT: the
 *      classes are needed to know T).  Caller: exclusive prefix sum -> offsets (int64), total.
 *   2. mrirt_brats_emit_samples: MLP inputs of sample k of ray p at row offsets[p] + k:
 *      coords[row][3] = 2*clamp(pIdx,0,dim-1)/(dim-1) - 1 (== predict_volume's coordinate at lattice
 *      points, inr/inr/model.py:124-128), feats[row][4] = the four trilinear samples z-scored as
 *      (v - zmu[m]) / zsigma[m] (inr/viewer/brats_viewer.py:281-287).  All four grids must be bound.
 *      Caller: mrirt_inr_forward(desc, coords, feats, total, NULL, classes).
 *   3. mrirt_render_brats_stream: K1 as mrirt_render_brats_ex, the prediction label of sample k of
 *      ray p read from classes[offsets[p] + k] (requires params->showPred != 0; whole-frame only). */
int mrirt_brats_sample_counts(const MrirtBratsParams* params, const MrirtRenderExt* ext, uint32_t* counts, void* stream);
int mrirt_brats_emit_samples(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                             const float zmu[4], const float zsigma[4], const int64_t* offsets,
                             float* coords, float* feats, void* stream);
int mrirt_render_brats_stream(const MrirtBratsParams* params, const MrirtRenderExt* ext,
                              const void* const vol[4], const void* labels,
                              const int16_t* classes, const int64_t* offsets,
                              void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);

/* The one-call, chunked and ERT-aware form of this render is mrirt_render_brats_inr (declared after the INR section). */

/* ------------------------------------------------------------------------------------ */
/* Brick layout conversion (load-time; replaces create_buffer + copy_from_numpy,         */
/* inr/viewer/brats_viewer.py:219-230)                                                   */
/* ------------------------------------------------------------------------------------ */

/* Number of ELEMENTS (not bytes) a bricked grid of `dims` occupies. */
int64_t mrirt_brick_elems(const uint32_t dims[3]);
/* linear (x fastest) -> bricked; elem_bytes in {1,4}; dst holds mrirt_brick_elems(dims) elements. */
int mrirt_brick_grid(const void* linear, void* bricked, const uint32_t dims[3], uint32_t elem_bytes, void* stream);
/* inverse, for round-trip tests */
int mrirt_unbrick_grid(const void* bricked, void* linear, const uint32_t dims[3], uint32_t elem_bytes, void* stream);
/* Number of float4 ELEMENTS a VG / QUAD grid of `dims` occupies. */
int64_t mrirt_vec4_elems(const uint32_t dims[3]);
/* Number of float4 ELEMENTS the three copies of a VGA grid of `dims` occupy together. */
int64_t mrirt_vga_elems(const uint32_t dims[3]);
/* linear fp32 (x fastest) -> VG, QUAD or VGA float4 grid (layout = MRIRT_LAYOUT_VG / _QUAD / _VGA). */
int mrirt_build_vec4_grid(const float* linear, void* vec4_grid, const uint32_t dims[3], uint32_t layout, void* stream);
/* four linear fp32 grids (gIntensity0..3, brats_viewer.py:64-69; all required) -> the MRIRT_LAYOUT_MOD4 grid:
 * mrirt_vec4_elems(dims) float4 elements, device. */
int mrirt_build_mod4_grid(const float* const linear[4], void* mod4_grid, const uint32_t dims[3], void* stream);
/* linear uint32 label grids (the reference's gLabels / gPreds uploads, brats_viewer.py:71-73; either may be NULL = no labels)
 * -> the MRIRT_LAYOUT_LABCELL grid: mrirt_vec4_elems(dims) elements of 8 bytes, device. */
int mrirt_build_label_cells(const uint32_t* seg_linear, const uint32_t* pred_linear, const uint32_t dims[3], void* cells, void* stream);
/* BC4 / RGTC1-unorm slices (8-byte blocks, [depth][ceil(h/4)][ceil(w/4)], device, 8-byte aligned) -> u8 voxels
 * [depth][height][width]: the decode scripts/volumeRendering/app.py:200-250 does on the host. */
int mrirt_bc4_decode(const void* blocks, uint32_t width, uint32_t height, uint32_t depth, uint8_t* out_u8, void* stream);

/* ------------------------------------------------------------------------------------ */
/* K2  volume_cs                                                                         */
/* ------------------------------------------------------------------------------------ */

/* Mirror of `struct Params`, scripts/volumeRendering/volume_render.slang:9-21. */
typedef struct MrirtVolumeParams {
    uint32_t imageSize[2]; float fovY; float stepCount;
    float nearPlane; float farPlane;
    float eye[3]; float padEye; float U[3]; float padU; float V[3]; float padV; float W[3]; float padW;
    uint32_t volDim[3]; uint32_t padDim;
} MrirtVolumeParams;

typedef enum MrirtVoxelMode {
    MRIRT_VOX_U32X4 = 0,   /* reference: StructuredBuffer<uint4>, one u32 per u8 voxel (app.py:150-153) */
    MRIRT_VOX_U8 = 1,      /* real bytes (1 B/voxel)                                                     */
    MRIRT_VOX_F32 = 2,     /* fp32 grid (build-defined generalisation)                    */
    MRIRT_VOX_CELL8 = 3    /* 8 B/voxel: the eight bytes of the trilinear cell based at the voxel, built */
                           /* once by mrirt_build_cell8 — one gather per sample, same bytes, same frame  */
} MrirtVoxelMode;

/* Drop-in for kernel.dispatch(...) of volume_cs, scripts/volumeRendering/app.py:350-358.
 * volume = gVolumeU8 in `mode`; ext may be NULL (uses cameraMode/orthoHalfHeight/math/outFormat/tiles). */
int mrirt_render_volume(const MrirtVolumeParams* params, const MrirtRenderExt* ext, const void* volume,
                        uint32_t mode, void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);
/* load time: u8 voxels (src_mode MRIRT_VOX_U8, or the reference's one-u32-per-voxel MRIRT_VOX_U32X4) ->
 * MRIRT_VOX_CELL8 grid of dims[0]*dims[1]*dims[2] 8-byte elements */
int mrirt_build_cell8(const void* voxels, uint32_t src_mode, const uint32_t dims[3], void* cell8, void* stream);

/* ------------------------------------------------------------------------------------ */
/* K3  raymarch_cs                                                                       */
/* ------------------------------------------------------------------------------------ */

/* Mirror of `struct Params` + the four float3 globals, scripts/raymarch/raymarch.slang:7-21. */
typedef struct MrirtSdfParams {
    uint32_t imageSize[2]; float fovY; uint32_t maxSteps;
    float maxDistance; float hitThreshold; float normalEps; float pad0;
    float gEye[3]; float pad1; float gU[3]; float pad2; float gV[3]; float pad3; float gW[3]; float pad4;
} MrirtSdfParams;

/* Drop-in for kernel.dispatch(...) of raymarch_cs, scripts/raymarch/app.py:212-223.
 * width/height are the render_texture dimensions (the shader queries the texture, :64). */
int mrirt_render_sdf(const MrirtSdfParams* params, uint32_t width, uint32_t height,
                     float* out_rgba, int64_t pitch_px, void* stream);

/* ------------------------------------------------------------------------------------ */
/* K4  compute_main (triangle-mesh BVH ray tracer)                                       */
/* ------------------------------------------------------------------------------------ */

/* Mirror of `struct Params`, scripts/mesh_rt/mesh_rt.slang:12-21, in cbuffer packing: 80 bytes, eye at 16, U at 32, V at 48,
 * W at 64 (padEye is the 4-byte hole the packing leaves after eye).  maxBounces is read by nothing, as in the shader. */
typedef struct MrirtMeshParams {
    uint32_t imageSize[2]; float fovY; uint32_t maxBounces;
    float eye[3]; float padEye;
    float U[3]; float padU; float V[3]; float padV; float W[3]; float padW;
} MrirtMeshParams;

/* Drop-in for kernel.dispatch(...) of compute_main, scripts/mesh_rt/app.py:233-243: one ray per pixel, the frame in STRICT
 * math only (bit-identical to the shader's arithmetic, unfused fp32 in its order).
 *   nodes = gBVHNodes (float4 x 2 per node, bvh.py's packing), tris = gTris (uint4, xyz used), verts = gVerts (float4, xyz)
 *   maxDepth: nodes on the longest root-to-leaf path (the traversal stack holds at most that many entries), 1..64
 *   ext (may be NULL): cameraMode, orthoHalfHeight, outFormat; math FAST, tiles or a kernelVariant -> MRIRT_ERR_ARG
 *   stats_dev (optional): 2 device uint64 counters, atomically incremented by {nodes popped, triangles tested}
 *   status_dev (optional): device word; bit 0 is set (atomic or) by a ray that met an index out of range, a stack deeper
 *              than maxDepth or more pops than nodeCount (a cycle).  Such a ray stops and its pixel is (1, 0, 1, 1).
 * nodeCount / triCount must be in [1, 2^23) (the shader decodes indices stored as floats with int(x + 0.5)), vertCount >= 1. */
int mrirt_render_mesh(const MrirtMeshParams* params, const MrirtRenderExt* ext,
                      const float* nodes, uint32_t nodeCount,
                      const uint32_t* tris, uint32_t triCount,
                      const float* verts, uint32_t vertCount,
                      uint32_t maxDepth, void* out_rgba, int64_t pitch_px,
                      uint64_t* stats_dev, uint32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Tile sharding helpers (multi-GPU)                               */
/* ------------------------------------------------------------------------------------ */
/* Exact empty-space skipping (build-defined acceleration).  The frame and the
 * sample counters are bit-identical to mrirt_render_brats_ex: a sample in a skipped macro cell still
 * counts as a march step, it just fetches and composites nothing, and a macro cell (8^3 voxels) is skipped
 * only when an upper bound of every enabled modality there cannot lift the transfer function above 0 for
 * THIS launch's window / weights and no shown label grid has a label there.  Applies to the VG / QUAD
 * pipelined kernels; any other configuration renders without skipping.                                   */
typedef struct MrirtSkip {
    const float* macroUb[4];      /* per modality: mrirt_build_macro_max output, or NULL (modality unused)   */
    const uint32_t* macroSeg;     /* mrirt_build_macro_labels of gLabels (needed when showSeg)               */
    const uint32_t* macroPred;    /* ... of gPreds (needed when showPred)                                    */
    uint32_t* mask;               /* scratch of maskWords uint32 (8^3 macro-cell bits, then the byte maps of the
                                     empty-radius transform); written by a launch unless mapReady             */
    uint32_t maskWords;           /* size of `mask` in words: must be >= mrirt_skip_mask_words(dims) (checked: a caller
                                     built against an older formula gets MRIRT_ERR_ARG, not device writes past its buffer) */
    uint32_t mapReady;            /* != 0: `mask` still holds the map a previous launch built from the SAME dims, window
                                     (ww, wl), gamma, volEnabled, volWeight, showSeg / showPred, math mode and summaries —
                                     the four pre-pass launches are skipped (a viewer frame changes the camera, not these).
                                     The caller orders that launch before this one (same stream, or an event).            */
} MrirtSkip;
int64_t mrirt_macro_cells(const uint32_t dims[3]);
int64_t mrirt_skip_mask_words(const uint32_t dims[3]);
/* from the LINEAR (x fastest) fp32 / uint32 grids, before any layout conversion */
int mrirt_build_macro_max(const float* linear, const uint32_t dims[3], float* macro_ub, void* stream);
int mrirt_build_macro_labels(const uint32_t* labels_linear, const uint32_t dims[3], uint32_t* macro_any, void* stream);
int mrirt_render_brats_skip(const MrirtBratsParams* params, const MrirtRenderExt* ext,
                            const void* const vol[4], const void* labels, const void* preds,
                            const MrirtSkip* skip, void* out_rgba, int64_t pitch_px,
                            uint64_t* stats_dev, void* stream);
/* Host-only query, nothing is launched: 1 = mrirt_render_brats_skip with these arguments marches with an empty-radius map
 * (it builds one into skip->mask, or trusts skip->mapReady); 0 = it is the plain launch and never reads or writes
 * skip->mask (window width or gamma <= 0, a negative weight, more than 256 macro cells on an axis, a missing summary, or a
 * launch whose kernel reads no map — e.g. the generic kernel of a VG / QUAD launch with an overlay shown over label grids
 * of 2^30 elements or more): a caller that caches maps must not mark such a scratch as holding one.  The answer comes
 * from the same plan as the launch.  < 0: the MrirtStatus the render call would return for these arguments.            */
int mrirt_brats_skip_applicable(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                                const void* labels, const void* preds, const MrirtSkip* skip);
/* Host-only query, nothing is launched: which march kernel family mrirt_render_brats_skip (skip != NULL) / mrirt_render_brats_ex
 * (skip == NULL) takes for these arguments — the generic kernel (any layout, 64-bit offsets: grids >= 4 GiB, label grids
 * >= 2^30 elements, BRICK), the software-pipelined one, the rolling one (2-4 shaded modalities), or the opt-in LDS kernels —
 * with MRIRT_KERNEL_SKIPPING / MRIRT_KERNEL_LABEL_CELLS or'ed in.  MRIRT_KERNEL_NONE: a rank that owns no tile.
 * < 0: the MrirtStatus the render call would return.  (Tests and the bench line name the kernel they measured with it.)  */
typedef enum MrirtKernelFamily {
    MRIRT_KERNEL_NONE = 0, MRIRT_KERNEL_GENERIC = 1, MRIRT_KERNEL_PIPELINED = 2, MRIRT_KERNEL_ROLLING = 3,
    MRIRT_KERNEL_SLAB = 4, MRIRT_KERNEL_RING = 5,
    MRIRT_KERNEL_SKIPPING = 16, MRIRT_KERNEL_LABEL_CELLS = 32
} MrirtKernelFamily;
int mrirt_brats_kernel_family(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                              const void* labels, const void* preds, const MrirtSkip* skip);

/* Dispatch order (build-defined scheduling; the frame and the counters are the same bits under any order: every ray is
 * independent).  The march records per workgroup how many steps its longest ray took (`steps`), and before the next frame
 * a small kernel on the same stream bins each XCD's workgroups into `classes` classes by those steps — thresholds at the
 * XCD's own quantiles — and writes `order`: the classes longest first, the launch's own order inside a class, every
 * workgroup on the XCD it had; then it zeroes `steps`.  The long ray packets so start in the first rounds of a launch
 * and its tail is made of short ones.  A zeroed record gives the identity, so a scratch starts as zeros in `steps`
 * (`order` needs no initial value); a record from another camera or scene can only cost time.
 * classes: 1 .. 16, 0 = the caller's own table: no builder runs, `order` is read as it stands (entries that are no
 * permutation leave pixels unwritten or written twice, never memory outside the frame and the record) and `steps`
 * accumulates maxima until the caller zeroes it.
 * One scratch per stream: frames in flight on different streams must not share a record.                              */
typedef struct MrirtOrder {
    uint32_t* order;              /* `words` uint32: order[b] = the pixel-map position workgroup b marches           */
    uint32_t* steps;              /* `words` uint32: the record, by pixel-map position (the index space of `order`'s values) */
    uint32_t words;               /* >= mrirt_order_words(imageSize, ext) (checked)                                   */
    uint32_t classes;
} MrirtOrder;
/* words of both tables for an untiled launch of this image size (ext: layout and kernelVariant decide the workgroup size);
 * 0: a tiled launch or an empty image — no ordering */
int64_t mrirt_order_words(const uint32_t imageSize[2], const MrirtRenderExt* ext);
/* mrirt_render_brats_skip with a dispatch order.  Ordered launches are the pipelined and rolling kernel families, whole
 * frame (tileSize == 0), marching without an empty-radius map; any other launch, or order == NULL, ignores the scratch
 * and is mrirt_render_brats_skip. */
int mrirt_render_brats_ordered(const MrirtBratsParams* params, const MrirtRenderExt* ext,
                               const void* const vol[4], const void* labels, const void* preds,
                               const MrirtSkip* skip, const MrirtOrder* order, void* out_rgba, int64_t pitch_px,
                               uint64_t* stats_dev, void* stream);
/* Host-only query, nothing is launched: 1 = mrirt_render_brats_ordered with these arguments and a scratch orders its
 * launch, 0 = it ignores the scratch; < 0: the MrirtStatus the render call would return. */
int mrirt_brats_order_applicable(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                                 const void* labels, const void* preds, const MrirtSkip* skip);
/* Host-only: the table the builder kernel writes for this record, for `words` workgroups (any count) and `classes` as above
 * (0 = 4); `steps` is left as it is. */
int mrirt_order_build_host(const uint32_t* steps, uint32_t words, uint32_t classes, uint32_t* order);

/* ------------------------------------------------------------------------------------ */
/* number of tiles rank `rank` of `world` renders for a W x H image */
int64_t mrirt_tiles_for_rank(uint32_t width, uint32_t height, uint32_t tileSize, uint32_t rank, uint32_t world);
/* scatter gathered compact tile buffers [world][max_local][ts][ts][4] back into a pitch-linear frame */
int mrirt_detile(const void* gathered, void* frame, uint32_t width, uint32_t height, int64_t pitch_px,
                 uint32_t tileSize, uint32_t world, uint32_t tileSkew, uint32_t outFormat, void* stream);

/* ------------------------------------------------------------------------------------ */
/* INR forward (inr/inr/model.py:11-50,119-141; notebooks/neumors_inr.ipynb:1165-1178)   */
/* ------------------------------------------------------------------------------------ */
typedef enum MrirtInrKind {
    MRIRT_INR_FOURIER_RELU = 0,   /* inputs built on the device: coords, Fourier features, modalities; ReLU */
    MRIRT_INR_SIREN = 1,          /* inputs (coords, modalities); sin activations, first layer scaled by w0 */
    MRIRT_INR_RAW_RELU = 2,       /* feats IS the [n][inDim] input matrix (apply_mlp); ReLU                 */
    MRIRT_INR_RAW_SIREN = 3       /* the same with the SIREN activations                                    */
} MrirtInrKind;

typedef struct MrirtInrDesc {
    uint32_t kind;           /* MrirtInrKind                                                    */
    uint32_t numLayers;      /* linear layers incl. head (<= 8)                                 */
    uint32_t inDim;          /* raw input width (3 + 6K + M for Fourier; 7 for the SIREN)       */
    uint32_t outDim;         /* classes (<= 16)                                                 */
    uint32_t hidden;         /* hidden width (multiple of 32, <= 256)                           */
    uint32_t fourierFreqs;   /* K (Fourier kind)                                                */
    uint32_t numMods;        /* M (<= 8 for kinds 0 and 1: the kernel stages 3 + 8 raw inputs per point) */
    float    w0;             /* SIREN first-layer frequency (30)                                */
    const void* weights;     /* device: packed bf16 weights, see mrirt_inr_pack_bytes           */
    const float* biases;     /* device: fp32 biases, layers concatenated, each padded to its padded out width */
    uint32_t flags;          /* MrirtInrFlags; 0 = the library's defaults                       */
    float    tieSigmas;      /* near-tie mark: top-2 gap < tieSigmas * sqrt(2) * calibrated rms error; 0 = default (3) */
} MrirtInrDesc;

/* A/B switches of the INR forward (measurement and tests; every combination computes the same classes up to the near-tie
 * refinement they switch off).  Version 2 read these from the process environment at every launch.                      */
typedef enum MrirtInrFlags {
    MRIRT_INR_NO_WEIGHT_STATIONARY = 1,  /* 4 x 256 SIRENs take the streaming kernel instead of the weight-stationary one */
    MRIRT_INR_NO_REFINE = 2,             /* no near-tie marking and no second pass: classes are the bf16 pass's           */
    MRIRT_INR_MARK_ONLY = 4              /* mark near-ties (bit 14 of the stored class) but run no second pass            */
} MrirtInrFlags;

/* bytes to allocate for the packed weight buffer of a network shape (0: unsupported shape): the bf16 MFMA image,
 * 64 KiB of slack (the kernel's last weight-chunk prefetch reads and ignores it), the split-bf16 (hi + lo) image the
 * near-tie refinement reads, 32 KiB of slack after it (the refinement's tile DMA always moves a full ring slot), and a
 * 1 KiB calibration record.  Size the buffer from this function, never from this list. */
int64_t mrirt_inr_pack_bytes(const MrirtInrDesc* desc);
/* pack fp32 row-major [in,out] weights (device, layers concatenated unpadded) into `packed`.  The images depend on
 * desc->kind and desc->w0 (the SIREN's w0 / 2 pi and 1 / 2 pi are folded in): pack and forward with the same
 * descriptor.  When desc->weights == packed and desc->biases is set (the usual call), the network is also
 * CALIBRATED here (mrirt_inr_calibrate); this synchronises `stream` once (load time). */
int mrirt_inr_pack_weights(const MrirtInrDesc* desc, const float* w_f32, void* packed, void* stream);
/* Near-tie calibration of a packed network: 8192 pseudo-random inputs through the bf16 pass and through the
 * split-bf16 pass; the rms difference of the logits is stored in the calibration record.  The class outputs
 * (argmax / predict_volume / mrirt_render_brats_inr) then re-evaluate every point whose two largest bf16 logits are
 * closer than 3 sqrt(2) times that error with split-bf16 operands in every layer, so the stored class agrees with an
 * fp32 evaluation except on ties ~1e-5 of the logit range apart.  Without a calibration nothing is re-evaluated. */
int mrirt_inr_calibrate(const MrirtInrDesc* desc, void* stream);
/* logits[n][outDim] (fp32) and/or argmax[n] (int16) for n points.
 * coords[n][3] in [-1,1]; feats[n][numMods].  Either output may be NULL.  logits are the bf16 pass's (those of
 * re-evaluated points, when argmax is requested too, the split-bf16 pass's). */
int mrirt_inr_forward(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t n,
                      float* logits, int16_t* argmax, void* stream);
/* the same with EVERY point evaluated by the split-bf16 pass (~16-bit operands in every layer, three MFMAs per
 * product): the accuracy reference of the bf16 path, three times its matrix work */
int mrirt_inr_forward_refined(const MrirtInrDesc* desc, const float* coords, const float* feats, int64_t n,
                              float* logits, int16_t* argmax, void* stream);
/* predict_volume (inr/inr/model.py:119-141): mods[M][H][W][D] fp32 -> pred[H][W][D] int16 */
int mrirt_inr_predict_volume(const MrirtInrDesc* desc, const float* mods, const uint32_t hwd[3],
                             int16_t* pred, void* stream);

/* ------------------------------------------------------------------------------------ */
/* INR training step (inr/inr/model.py:57-90 make_loss_and_grad): fp32, ReLU kinds only  */
/* ------------------------------------------------------------------------------------ */
/* One step is forward_f32 -> loss -> backward on one stream with one scratch buffer.  The network is its fp32 master copy:
 * w_f32 row-major [in][out] per layer, layers concatenated unpadded (what mrirt_inr_pack_weights takes), b_f32 the biases
 * concatenated UNPADDED; grad_w / grad_b have the same two layouts.  desc->weights / desc->biases are not read.  Kinds
 * MRIRT_INR_FOURIER_RELU and MRIRT_INR_RAW_RELU over every shape mrirt_inr_pack_bytes accepts; the SIREN kinds are refused
 * (MRIRT_ERR_ARG).  1 <= n < 2^31.  Products and sums are fp32 (v_mfma_f32_16x16x4_f32, a k-ordered fma chain); every sum over
 * the batch runs in a fixed order (no float atomics): the same inputs give the same bits.  No host synchronisation.
 * scratch: device memory, 16-byte aligned, owned by the caller; 0 bytes = unsupported kind / shape / n. */
int64_t mrirt_inr_train_scratch_bytes(const MrirtInrDesc* desc, int64_t n);
/* what the loss alone needs (the first bytes of the step's scratch: the three calls may share one buffer) */
int64_t mrirt_inr_loss_scratch_bytes(int64_t n);
/* logits[n][outDim] = the network on coords[n][3] / feats[n][numMods] (RAW kind: feats[n][inDim], coords unused); leaves
 * the input matrix and every hidden activation in scratch for the backward pass */
int mrirt_inr_forward_f32(const MrirtInrDesc* desc, const float* w_f32, const float* b_f32, const float* coords,
                          const float* feats, int64_t n, float* logits, void* scratch, int64_t scratch_bytes, void* stream);
/* loss[1] = (1 - dw) ce + dw (1 - mean_k dice_k) for dw > 0, else ce, with ce = mean_p(ce_p cw[label_p]) and
 * dice_k = (2 sum_p p_pk y_pk + 1e-6) / (sum_p p_pk + sum_p y_pk + 1e-6); aux[2 C] = ce per class (sum_p ce_p y_pk /
 * max(count_k, 1)), then dice per class; dlogits[n][C] = dloss/dlogits (NULL: not computed).  labels int32 in 0..C-1 (a
 * label outside it reads no memory; it counts for no class and weighs 0).  class_weights: C floats on the HOST.
 * 1 <= num_classes <= 16, dice_weight finite.  The class sums are fp64.  loss and aux stay on the device. */
int mrirt_inr_loss(const float* logits, const int32_t* labels, int64_t n, uint32_t num_classes, const float* class_weights,
                   float dice_weight, float* loss, float* aux, float* dlogits, void* scratch, int64_t scratch_bytes, void* stream);
/* grad_w / grad_b (+= with flags bit 0, else =) from dlogits[n][outDim] and what forward_f32 left in the same scratch for
 * the same desc and n: dW_l = h_{l-1}^T dz_l, db_l = sum_p dz_l, dz_{l-1} = (dz_l W_l^T) where z_{l-1} > 0, else 0. */
int mrirt_inr_backward(const MrirtInrDesc* desc, const float* w_f32, int64_t n, const float* dlogits, float* grad_w,
                       float* grad_b, uint32_t flags, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* INR training loop (inr/inr/train.py:18-259, inr/inr/dataloader.py:86-96,133-155)      */
/* ------------------------------------------------------------------------------------ */
/* A device-resident set of cases of one shape: case k is mods[k] = float [numMods][H][W][D] and seg[k] = int16 [H][W][D],
 * C order (what mrirt_inr_predict_volume reads).  `mods` and `seg` are DEVICE arrays of ncases device pointers (mods may be
 * NULL when numMods == 0).  Every axis >= 2, H W D < 2^31, numMods <= 8, 1 <= ncases <= 65535. */
typedef struct MrirtInrCache {
    const float* const* mods;
    const int16_t* const* seg;
    uint32_t ncases, numMods;
    uint32_t hwd[3];
    uint32_t reserved;
} MrirtInrCache;

/* Micro-batch `batch_index` of the stream `seed`: n voxels drawn with Philox4x32-10, point i from key (seed lo, seed hi) and
 * counter (i, batch_index lo, batch_index hi, 0); its output words r0..r3 give case = mulhi32(r0, ncases), x = mulhi32(r1, H),
 * y = mulhi32(r2, W), z = mulhi32(r3, D) with mulhi32(r, m) = (r m) >> 32 (no rejection step: a value's probability is off
 * by at most m / 2^32).  coords[n][3] = (float(x) / float(H - 1)) * 2 - 1 ..., feats[n][numMods] = mods[case][m][x][y][z],
 * labels[n] = seg[case][x][y][z] widened to int32 — the three arrays mrirt_inr_forward_f32 / mrirt_inr_loss take.  The same
 * arguments give the same bits.  1 <= n < 2^31; feats may be NULL when numMods == 0.  No host synchronisation. */
int mrirt_inr_sample_batch(const MrirtInrCache* cache, uint64_t seed, uint64_t batch_index, int64_t n, float* coords,
                           float* feats, int32_t* labels, void* stream);

/* optax.chain(clip_by_global_norm(clipNorm), adamw(lr)) for one update.  lr is the step's (already scheduled) rate. */
typedef struct MrirtAdamW {
    float lr, b1, b2, eps, weightDecay;
    float clipNorm;          /* <= 0 or +inf: no clipping */
} MrirtAdamW;

/* Update number t + 1 (t = updates already applied) of the nw weights and nb biases in place, with their first and second
 * moments, from the gradients gw / gb scaled by gscale:
 *   g = grad gscale;  norm = sqrt(sum g^2) over gw then gb, in fp64 (fixed order, no atomics);
 *   s = float(norm < clipNorm ? 1 : clipNorm / norm), NaN for a non-finite norm; 1 without clipping;
 *   gc = g s;  mu = b1 mu + (1 - b1) gc;  nu = b2 nu + ((1 - b2) gc) gc;  mh = mu / (1 - b1^(t+1));  nh = nu / (1 - b2^(t+1));
 *   p = p - lr (mh / (sqrtf(nh) + eps) + weightDecay p)
 * in fp32 without contraction; 1 - b1, 1 - b2, 1 - b1^(t+1), 1 - b2^(t+1) are evaluated in fp64 and rounded to fp32.
 * gnorm: two doubles on the device, [0] = norm, [1] = s (widened).  nw >= 1, nb >= 0, nw + nb < 2^31; hyper-parameters
 * finite (clipNorm may be +inf), 0 <= b1, b2 < 1, eps > 0, gscale finite.  scratch: device, 16-byte aligned,
 * mrirt_inr_adamw_scratch_bytes(nw + nb) bytes.  No host synchronisation: s is read on the device. */
int64_t mrirt_inr_adamw_scratch_bytes(int64_t n);
int mrirt_inr_adamw_step(float* w, float* b, const float* gw, const float* gb, float* mu_w, float* mu_b, float* nu_w,
                         float* nu_b, int64_t nw, int64_t nb, const MrirtAdamW* hp, uint64_t t, float gscale, double* gnorm,
                         void* scratch, int64_t scratch_bytes, void* stream);

/* optax.warmup_cosine_decay_schedule(0, peak, warmup, decay_steps, end) at t updates already applied, in fp64:
 * t < warmup: peak t / warmup; else T = decay_steps - warmup (T <= 0: MRIRT_ERR_ARG, as optax asserts), u = min(t - warmup, T) / T,
 * lr = peak ((1 - a) 0.5 (1 + cos(pi u)) + a), a = end / peak.  peak > 0, end >= 0, both finite.  Host only. */
int mrirt_inr_lr_schedule(double peak, double end, uint32_t warmup, uint32_t decay_steps, uint64_t t, double* lr);

typedef struct MrirtInrTrainCfg {
    int64_t microBatch;          /* points per micro-batch, 1 .. 2^31 - 1                            */
    uint32_t accum;              /* micro-batches per update, >= 1; gradients are scaled by 1 / accum */
    uint32_t warmupSteps, decaySteps, reserved;      /* the schedule's warmup and decay_steps         */
    uint64_t seed;
    double peakLr, minLr;
    float classWeights[16];      /* the first desc->outDim are read                                   */
    float diceWeight;
    MrirtAdamW adamw;            /* lr is not read: the schedule sets it                              */
} MrirtInrTrainCfg;

typedef struct MrirtInrTrainState {      /* device pointers, the flat layouts of mrirt_inr_forward_f32 */
    float *w, *b, *mu_w, *mu_b, *nu_w, *nu_b;
} MrirtInrTrainState;

/* Enqueues `steps` optimiser steps: step k runs accum x (mrirt_inr_sample_batch with batch_index (first_step + k) accum + a
 * -> mrirt_inr_forward_f32 -> mrirt_inr_loss -> mrirt_inr_backward, flags 0 for a = 0 and bit 0 after) and one
 * mrirt_inr_adamw_step with gscale = 1 / accum, t = first_step + k and lr = the schedule at t: the bits of the separate calls.
 * desc: MRIRT_INR_FOURIER_RELU with numMods == cache->numMods; outDim is the number of classes.  history (device):
 * [steps][accum][1 + 2 outDim] floats, per micro-batch the loss, then CE per class, then Dice per class.  Every argument is
 * checked before anything is launched; no host synchronisation, no allocation.  scratch: device, 16-byte aligned. */
int64_t mrirt_inr_train_run_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg);
int mrirt_inr_train_run(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                        const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history, void* scratch,
                        int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* SIREN training (notebooks/neumors_inr.ipynb:1150-1200): the fp32 step and loop for     */
/* the sine kinds.  Added within ABI 4: new symbols only                                  */
/* ------------------------------------------------------------------------------------ */
/* The twins of mrirt_inr_train_scratch_bytes / _forward_f32 / _backward / _train_run_scratch_bytes / _train_run for
 * MRIRT_INR_SIREN (x = (coords, modalities), inDim = 3 + numMods) and MRIRT_INR_RAW_SIREN (x = feats[n][inDim]) with
 * fourierFreqs == 0 and a finite w0 != 0; every other kind is MRIRT_ERR_ARG (the ReLU kinds train through mrirt_inr_*, which
 * go on refusing the SIREN kinds: one way to train each kind).  Same layouts of w_f32 / b_f32 / gradients, same argument
 * meaning, same checks before any launch, no host synchronisation, no allocation, flags bit 0 = accumulate.
 *   forward   x' = w0 x (one fp32 multiply);  a_l = (in_l . W_l) + b_l with in_0 = x', in_l = h_{l-1};  h_l = sin32(a_l);
 *             the head is linear.  c_l = cos32(a_l) is stored in scratch beside h_l.
 *   backward  da_l = dh_l c_l (one fp32 multiply);  dh_{l-1} = da_l W_l^T;  dW_l = in_l^T da_l;  db_l = sum_p da_l
 * sin32 / cos32: the fp32 argument widened to fp64, reduced by multiples of pi/2, evaluated by polynomials in fp64 and
 * rounded once to fp32 — correctly rounded on every argument tested for |a| <= 2^20 (the stated domain); a finite argument
 * beyond it gives sin = +-0, cos = 1; NaN and +-inf give NaN.  mrirt_inr_loss, mrirt_inr_sample_batch, mrirt_inr_adamw_step
 * and mrirt_inr_lr_schedule serve both families.  mrirt_siren_train_run: desc is MRIRT_INR_SIREN with
 * numMods == cache->numMods; it enqueues the same sequence as mrirt_inr_train_run with the mrirt_siren_* step. */
int64_t mrirt_siren_train_scratch_bytes(const MrirtInrDesc* desc, int64_t n);
int mrirt_siren_forward_f32(const MrirtInrDesc* desc, const float* w_f32, const float* b_f32, const float* coords,
                            const float* feats, int64_t n, float* logits, void* scratch, int64_t scratch_bytes, void* stream);
int mrirt_siren_backward(const MrirtInrDesc* desc, const float* w_f32, int64_t n, const float* dlogits, float* grad_w,
                         float* grad_b, uint32_t flags, void* scratch, int64_t scratch_bytes, void* stream);
int64_t mrirt_siren_train_run_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg);
int mrirt_siren_train_run(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                          const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history, void* scratch,
                          int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Muon for INR training (notebooks/neumors_inr.ipynb:1191-1192: optax.contrib.muon).    */
/* Added within ABI 4: new symbols and one new struct only, mrirt_sizeof(11)             */
/* ------------------------------------------------------------------------------------ */
/* Muon (Jordan et al. 2024) as optax's scale_by_muon states it, for the weight matrices of a network of shape `desc` (any
 * kind the training entry points take; only numLayers, inDim, hidden, outDim matter); the biases take AdamW.  optax's
 * defaults: beta 0.95, nesterov 1, nsSteps 5, nsCoeffs (3.4445, -4.7750, 2.0315), eps 1e-8, weightDecay 0. */
typedef struct MrirtMuon {
    float beta, eps, weightDecay;
    float nsCoeffs[3];           /* c0, c1, c2 of X <- c0 X + (c1 A + c2 A A) X, A = X X^T */
    uint32_t nsSteps, nesterov;
} MrirtMuon;
/* Update number t (0-based) of W[in][out] (flat row-major layout of mrirt_inr_forward_f32), with g' = (g gscale) s and s the
 * clip factor of mrirt_inr_adamw_step over ALL gradients (same kernels, same gnorm[2]); every operation below is one fp32
 * rounding unless said otherwise, in the order written:
 *   mu  <- beta mu + omb g'                        omb = float(1 - beta), c1 = float(1 - beta^(t+1)), c2 = float(1 - beta^(t+2)),
 *   m^   = beta (mu / c2) + omb (g' / c1)          evaluated in fp64 on the host;  without nesterov m^ = mu / c1
 *   X    = float(double(m^) / (sqrt(sum m^^2) + double(eps)))      the sum in fp64 in a fixed order; X^T when in > out
 *   nsSteps times: A = X X^T;  B = c1 A + c2 (A A);  X <- c0 X + (B X)      the sums on the fp32 MFMA, increasing k
 *   W   <- W - lr (float(sqrt(max(1, out / in))) O + weightDecay W)          O = X, transposed back
 * Biases: adamw_one of mrirt_inr_adamw_step with adamw's b1, b2, eps, weightDecay and the same s, lr, t.  adamw also supplies
 * lr and clipNorm.  There is no second moment of the weights.
 * mrirt_muon_orthogonalize: out_flat = NS(m_flat) for every layer's matrix in one call (out_flat may be m_flat; neither may
 * overlap scratch).  An all-zero matrix gives zeros; a NaN anywhere in a matrix makes that layer's output NaN, not the others'.
 * mrirt_muon_scratch_bytes: device bytes either call needs (0 for a shape the training entry points refuse).
 * Checks before any launch: MRIRT_ERR_NULL; MRIRT_ERR_ARG for beta outside [0, 1), eps not finite or <= 0, non-finite
 * nsCoeffs / weightDecay / gscale, nsSteps outside 1..16, nesterov > 1, what mrirt_inr_adamw_step refuses of `adamw`, a
 * scratch that is not 16-byte aligned or too small, a refused shape.  No allocation, no host synchronisation, no float
 * atomics: the same inputs give the same bits. */
int64_t mrirt_muon_scratch_bytes(const MrirtInrDesc* desc);
int mrirt_muon_orthogonalize(const MrirtInrDesc* desc, const float* m_flat, float* out_flat, const MrirtMuon* hp, void* scratch,
                             int64_t scratch_bytes, void* stream);
int mrirt_muon_step(const MrirtInrDesc* desc, float* w, float* b, const float* gw, const float* gb, float* mu_w, float* mu_b,
                    float* nu_b, const MrirtMuon* hp, const MrirtAdamW* adamw, uint64_t t, float gscale, double* gnorm,
                    void* scratch, int64_t scratch_bytes, void* stream);
/* mrirt_inr_train_run / mrirt_siren_train_run (by desc->kind: MRIRT_INR_FOURIER_RELU or MRIRT_INR_SIREN) with
 * mrirt_muon_step in place of mrirt_inr_adamw_step; cfg->adamw is the bias / clip half; state->nu_w is not touched. */
int64_t mrirt_inr_train_run_muon_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg);
int mrirt_inr_train_run_muon(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg, const MrirtMuon* hp,
                             const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps, float* history, void* scratch,
                             int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* The loss and the sampling mix of scripts/jax_inr_brats.py (lines 179-257, 466-528).    */
/* Added within ABI 4: new symbols and three new structs only, mrirt_sizeof(13..15)      */
/* ------------------------------------------------------------------------------------ */
/* loss_fn of jax_inr_brats.py:205-257 on given logits.  C classes, n points, e = edemaClass, eps = labelSmoothing; per point
 * yh_k = [label == k] (all 0 for a label outside 0..C-1), y_k = yh_k (1 - eps) + eps / C, p = softmax(z),
 * ce_p = -sum_k y_k log p_k, w_p = classWeights[label] (0 for a label outside the range).
 *   CE    focalGamma == 0: (1/n) sum_p ce_p w_p.  Otherwise pt = sum_k y_k p_k, m_p = max(1 - pt, 0)^gamma (times
 *         sum_k y_k focalAlpha_k with flags bit 1) and CE = [(1/n) sum_p m_p ce_p] [(1/n) sum_p w_p].  The product of two means
 *         is the reference's: focal_ce_loss returns a scalar, which lines 230-233 multiply by the weight vector and average.
 *         (The clamp at 0 only acts where rounding puts pt above 1, where the reference's power is NaN.)
 *   DL    I_k = sum_p p_k y_k, S_k = sum_p p_k + sum_p y_k, dice_k = (2 I_k + 1e-6) / (S_k + 1e-6); flags bit 0: 1 - mean_k dice_k
 *         (model.py); clear: 1 - sum_k dice_k v_k, v_k = Y_k / (sum_j Y_j + 1e-6), Y_k = sum_p y_k (the script's default).
 *   loss  = diceWeight > 0 ? (1 - dw) CE + dw DL : CE, then with g = [label == e], q = p_e, TP = sum q g, FP = sum q (1 - g),
 *         FN = sum (1 - q) g, each only when its weight is > 0:
 *           + edemaFpWeight FP / n  + tverskyWeight (1 - TP / (TP + tverskyAlpha FP + tverskyBeta FN + 1e-6))
 *           + edemaLogitReg (1/n) sum_p softplus(z_e) (1 - g),  softplus(z) = max(z, 0) + log1p(exp(-|z|)).
 * aux[2 C]: sum_p ce_p yh_k / max(count_k, 1), then dice_k.  terms[5] (may be NULL): CE, DL (0 when dw <= 0), FP / n, the
 * Tversky index, the logit-regulariser mean (the last three 0 when e >= C).  dlogits[n][C] (may be NULL): the exact derivative
 * of loss through the softmax Jacobian, the softplus' direct term added at j = e; y, v_k and the class-weight mean are
 * constants.  Per-point values are fp32, every sum over the batch is fp64 in a fixed order (per-block partial sums, at most
 * 256 blocks, added in block order): no float atomics, the same inputs give the same bits; no label indexes memory; three
 * launches; no host synchronisation; loss, aux and terms stay on the device.  Finite logits give finite outputs.
 * With focalGamma 0, labelSmoothing 0, flags bit 0 set and the three edema weights 0 it runs mrirt_inr_loss's operations in
 * mrirt_inr_loss's order: the same bits in loss, aux and dlogits.
 * Checks before any launch: MRIRT_ERR_NULL (logits, labels, ext, loss, aux, scratch); MRIRT_ERR_ARG for n outside 1..2^31-1,
 * num_classes outside 1..16, focalGamma other than 0 or a value in [1, 8], labelSmoothing outside [0, 1), a non-finite
 * diceWeight / class weight / focalAlpha (when used), a negative or non-finite edemaFpWeight, tverskyAlpha, tverskyBeta,
 * tverskyWeight or edemaLogitReg, edemaClass >= num_classes while any of edemaFpWeight, tverskyWeight, edemaLogitReg is > 0,
 * flags above 3, a scratch that is not 16-byte aligned or smaller than mrirt_inr_loss_ext_scratch_bytes(n). */
typedef struct MrirtInrLossExt {
    float classWeights[16];      /* first C read */
    float focalAlpha[16];        /* read only with flags bit 1 */
    float diceWeight;
    float focalGamma;            /* 0: plain CE; otherwise 1 <= gamma <= 8 */
    float labelSmoothing;        /* 0 <= eps < 1 */
    float edemaFpWeight, tverskyAlpha, tverskyBeta, tverskyWeight, edemaLogitReg;   /* weights >= 0, finite */
    uint32_t edemaClass;         /* the reference's 2; must be < C when any of the three edema weights is > 0 */
    uint32_t flags;              /* bit 0: Dice = mean over classes (model.py); clear: prevalence-weighted (the script's default)
                                    bit 1: focalAlpha is used */
} MrirtInrLossExt;
int64_t mrirt_inr_loss_ext_scratch_bytes(int64_t n);
int mrirt_inr_loss_ext(const float* logits, const int32_t* labels, int64_t n, uint32_t num_classes, const MrirtInrLossExt* ext,
                       float* loss, float* aux, float* terms, float* dlogits, void* scratch, int64_t scratch_bytes, void* stream);

/* The tumour voxels of a cache: for every case the flat offsets (x W D + y D + z) of the voxels with seg > 0, ascending, the
 * cases concatenated; offsets[c] .. offsets[c + 1] is case c's range.  Both arrays live on the device. */
typedef struct MrirtInrTumourIndex {
    const uint32_t* index;
    const int64_t* offsets;      /* [ncases + 1] */
} MrirtInrTumourIndex;
/* counts[c] (device, [ncases]) = voxels of case c with seg > 0.  The caller reads them once (load time), forms the exclusive
 * prefix sum offsets[ncases + 1] and sizes index by offsets[ncases].  mrirt_inr_tumour_index then fills index in ascending
 * order: tumour voxels per chunk of 4096 voxels, a scan per case in a launch of its own, then the emit (three launches, no
 * workgroup waits for another, no atomic append); a slot outside offsets[c] .. offsets[c + 1] is never written.  H W D >= 2^32
 * is MRIRT_ERR_ARG; otherwise the cache's own limits hold.  scratch: device, 16-byte aligned,
 * mrirt_inr_tumour_index_scratch_bytes(cache) bytes (0 for a refused cache). */
int mrirt_inr_tumour_count(const MrirtInrCache* cache, int64_t* counts, void* stream);
int64_t mrirt_inr_tumour_index_scratch_bytes(const MrirtInrCache* cache);
int mrirt_inr_tumour_index(const MrirtInrCache* cache, const int64_t* offsets, uint32_t* index, void* scratch, int64_t scratch_bytes,
                           void* stream);
/* mrirt_inr_sample_batch with the first n_tumour points drawn from the tumour voxels (the reference puts its tumour draws
 * first too, jax_inr_brats.py:466-528; its rejection loop and its one case per micro-batch are replaced by this rule, which
 * is this library's: counter-based, one launch).  Point i >= n_tumour is mrirt_inr_sample_batch's point i, same bits.  Point
 * i < n_tumour takes the same Philox words r0..r3: case = mulhi32(r0, ncases), cnt = offsets[case + 1] - offsets[case]; with
 * cnt > 0 the voxel is index[offsets[case] + ((uint64) r1 cnt >> 32)], decoded to (x, y, z); with cnt == 0 the uniform draw
 * from r1..r3 (the reference's "fallback fill").  0 <= n_tumour <= n, else MRIRT_ERR_ARG; n_tumour == 0 accepts a NULL
 * index.  The host forms n_tumour = int(n clip(ratio, 0, 1)) in double, as line 468 does. */
int mrirt_inr_sample_batch_mix(const MrirtInrCache* cache, const MrirtInrTumourIndex* tumour, uint64_t seed, uint64_t batch_index,
                               int64_t n, int64_t n_tumour, float* coords, float* feats, int32_t* labels, void* stream);

/* One run for every combination: the step by desc->kind (MRIRT_INR_FOURIER_RELU or MRIRT_INR_SIREN), the update Muon when
 * muon is given (else AdamW), the loss mrirt_inr_loss_ext when loss is given (cfg->classWeights / diceWeight are then not
 * read by the loss, though still checked), the sampler mrirt_inr_sample_batch_mix when nTumour > 0 (0 <= nTumour <=
 * cfg->microBatch; tumour.index / .offsets then required).  With every member NULL / 0 it enqueues the launches of
 * mrirt_inr_train_run / mrirt_siren_train_run and returns their bits.  The history layout is mrirt_inr_train_run's.
 * scratch: the plain run's, then mrirt_muon_step's (with muon), then mrirt_inr_loss_ext's (with loss).  Every member is
 * checked before anything is launched. */
typedef struct MrirtInrTrainExt {
    const MrirtInrLossExt* loss;
    const MrirtMuon* muon;
    MrirtInrTumourIndex tumour;
    int64_t nTumour;
} MrirtInrTrainExt;
int64_t mrirt_inr_train_run_ext_scratch_bytes(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                                              const MrirtInrTrainExt* ext);
int mrirt_inr_train_run_ext(const MrirtInrDesc* desc, const MrirtInrCache* cache, const MrirtInrTrainCfg* cfg,
                            const MrirtInrTrainExt* ext, const MrirtInrTrainState* state, uint64_t first_step, uint32_t steps,
                            float* history, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Exact distance transform and Hausdorff distance (inr/inr/model.py:164-195)            */
/* ------------------------------------------------------------------------------------ */
/* labels / pred / truth: the int16 [H][W][D] C-order volume mrirt_inr_predict_volume writes (device).  The coordinate of
 * index i on axis k is c_k(i) = double(float(i) * spacing[k]); the squared distance field of a mask M is
 *   F_M(x) = min over y in M of ((d0^2 + d1^2) + d2^2),  d_k = c_k(x_k) - c_k(y_k),
 * every operation in unfused fp64 in that order, +inf everywhere when M is empty — bit for bit what a nearest-neighbour
 * query over the reference's float32 coordinate grid returns, squared.
 * Limits (checked before any HIP call): every axis in 1..4096 and H*W*D < 2^31 (MRIRT_ERR_DIMS); finite spacing whose
 * product with the last index is finite too, num_classes in 1..32, scratch_bytes large enough (MRIRT_ERR_ARG).
 * mrirt_edt_scratch_bytes: device bytes mrirt_hausdorff needs for num_classes in 1..32 (two fp64 fields + 32 B per class),
 * what mrirt_edt_squared needs for num_classes == 0 (64: it runs in place in field_sq); 0 for a volume outside the limits. */
int64_t mrirt_edt_scratch_bytes(const uint32_t hwd[3], uint32_t num_classes);
/* field_sq[H][W][D] (device, fp64) = F_M for M = (labels == cls); any cls is valid (a class that does not occur: +inf) */
int mrirt_edt_squared(const int16_t* labels, const uint32_t hwd[3], int32_t cls, const float spacing[3],
                      double* field_sq, void* scratch, int64_t scratch_bytes, void* stream);
/* For every class c < num_classes, P = (pred == c), T = (truth == c):
 *   directed_sq[2c] = max over P of F_T, directed_sq[2c + 1] = max over T of F_P (device, fp64; both NaN when the class is
 * absent from either volume); the reference's hausdorff[c] is sqrt(max of the two).  A label outside [0, num_classes)
 * belongs to no class.  The result stays in device memory: nothing synchronises with the host. */
int mrirt_hausdorff(const int16_t* pred, const int16_t* truth, const uint32_t hwd[3], const float spacing[3],
                    uint32_t num_classes, double* directed_sq, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Class surfaces from label volumes (naive surface nets), the input of K4                */
/* ------------------------------------------------------------------------------------ */
/* labels: the int16 [n0][n1][n2] C-order volume of mrirt_inr_predict_volume / mrirt_hausdorff (device); axis k is world axis
 * k.  Voxel v is inside iff 0 <= labels[v] < 32 and bit labels[v] of class_mask is set; every voxel outside the volume is
 * outside, so surfaces close at the volume's faces.  Cell c (0 <= c_k <= n_k, linear index (c0 (n1+1) + c1)(n2+1) + c2) has
 * the voxels c - 1 + b, b in {0,1}^3, as corners and is active when they are neither all inside nor all outside.
 *   vertex of an active cell: over its edges whose two corners differ (from corner b along axis a, b_a = 0) S_k = sum of
 *     2 b_k + (k == a) and m their number; q_k = float(S_k) / float(2 m), x_k = (float(c_k - 1) + q_k) * spacing[k] + origin[k],
 *     every operation a separate float32 one.  Vertices are numbered in increasing linear cell index.
 *   quads: cell c owns the lattice edge from voxel c - 1 to c - 1 + e_a when c_b >= 1 and c_c >= 1, (a, b, c) one of (0,1,2),
 *     (1,2,0), (2,0,1).  An owned edge whose voxels differ emits the quad Q(ib, ic) = vertex of cell c - (1-ib) e_b - (1-ic) e_c
 *     as the triangles (Q00, Q10, Q11), (Q00, Q11, Q01) when voxel c - 1 is inside (normal along +a), else (Q00, Q11, Q10),
 *     (Q00, Q01, Q11); quads are ordered by owning cell, then by a.
 * The mesh is closed and oriented outwards.  With origin = volMin and spacing = voxelSize of MrirtBratsParams it lies on
 * the K1 volume (K1 samples lattice points, no half-voxel offset).
 * Limits (checked before any HIP call): every extent >= 1 (MRIRT_ERR_DIMS); (n0+1)(n1+1)(n2+1) <= 2^31 - 1, finite
 * spacing > 0, finite origin, vert_cap / tri_cap >= 0, scratch 16-byte aligned and scratch_bytes large enough (MRIRT_ERR_ARG).
 * mrirt_surface_scratch_bytes: device bytes both calls need (5 B per cell + 16 B per 1024 cells, rounded up); 0 for a
 * volume outside the limits. */
int64_t mrirt_surface_scratch_bytes(const uint32_t hwd[3]);
/* counts_dev (device, int64[2]) = { vertices V, triangles T } of the class set's surface; an empty set gives { 0, 0 }.
 * Nothing synchronises with the host. */
int mrirt_surface_count(const int16_t* labels, const uint32_t hwd[3], uint32_t class_mask, void* scratch, int64_t scratch_bytes,
                        int64_t* counts_dev, void* stream);
/* verts (device, float32 [vert_cap][3]) and tris (device, int32 [tri_cap][3]) receive the mesh.  Complete on its own (no
 * earlier mrirt_surface_count needed): counts_dev is always written; geometry is written only when V <= vert_cap AND
 * T <= tri_cap, and then exactly V vertices and T triangles — nothing past them.  verts / tris may be NULL when their
 * capacity is 0. */
int mrirt_surface_extract(const int16_t* labels, const uint32_t hwd[3], uint32_t class_mask, const float spacing[3],
                          const float origin[3], float* verts, int64_t vert_cap, int32_t* tris, int64_t tri_cap,
                          void* scratch, int64_t scratch_bytes, int64_t* counts_dev, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Connected components of label volumes; the counts of the slice-consistency score     */
/* ------------------------------------------------------------------------------------ */
/* labels: the int16 [n0][n1][n2] C-order volume of mrirt_surface_* (device), with the same inside rule: voxel v is inside iff
 * 0 <= labels[v] < 32 and bit labels[v] of class_mask is set; a voxel outside the volume is outside.  Two inside voxels are
 * adjacent iff they differ by at most 1 on every axis and on at most `connectivity` (1, 2 or 3) axes: the 6, 18 or 26
 * neighbours, scipy.ndimage.generate_binary_structure(3, connectivity).  A component is a class of the transitive closure;
 * its root is its smallest linear index (i0 n1 + i1) n2 + i2, and components are numbered 1 .. N by increasing root — the
 * numbering of scipy.ndimage.label.
 * Limits (checked before any HIP call): every extent >= 1 (MRIRT_ERR_DIMS); n0 n1 n2 <= 2^31 - 1, connectivity in 1..3,
 * 0 <= n_components <= n0 n1 n2, min_voxels >= 0, keep_largest 0 or 1, scratch 16-byte aligned and scratch_bytes large
 * enough (MRIRT_ERR_ARG).  Nothing synchronises with the host; every result is the same from run to run.
 * mrirt_cc_scratch_bytes: device bytes mrirt_cc_label needs (4 B per 1024 voxels, and per 1024 of those until one such
 * chunk is left, each part rounded up to 256 B); 0 for a volume outside the limits. */
int64_t mrirt_cc_scratch_bytes(const uint32_t hwd[3]);
/* components (device, int32 [n0][n1][n2]) = the component number of every inside voxel, 0 outside; it is the call's working
 * array and every element is written.  count_dev (device, int64[1]) = N. */
int mrirt_cc_label(const int16_t* labels, const uint32_t hwd[3], uint32_t class_mask, uint32_t connectivity,
                   int32_t* components, int64_t* count_dev /* [1] = N */, void* scratch, int64_t scratch_bytes, void* stream);
/* sizes (device, int32 [n_components]): sizes[k - 1] = voxels of component k.  Numbers outside 1 .. n_components are not
 * counted; n_components == 0 accepts a NULL sizes and does nothing. */
int mrirt_cc_sizes(const int32_t* components, const uint32_t hwd[3], int64_t n_components, int32_t* sizes, void* stream);
/* out[v] = labels[v] where components[v] is 0 (or outside 1 .. n_components) or v's component is kept, else fill.  A
 * component is kept iff its size >= min_voxels and, with keep_largest, it is the largest one (ties: the lowest number).
 * out may be labels. */
int mrirt_cc_filter(const int16_t* labels, const int32_t* components, const int32_t* sizes, int64_t n_components,
                    const uint32_t hwd[3], int64_t min_voxels, int32_t keep_largest, int16_t fill, int16_t* out, void* stream);
/* counts (device, int64 [n2][3]) = { A, I, U } per index z of the LAST axis, on the raw int16 values p: A = #(p_z > 0);
 * for z >= 1, I = #((p_z == p_{z-1}) & (p_z > 0)) and U = #((p_z > 0) | (p_{z-1} > 0)); I = U = 0 at z = 0. */
int mrirt_slice_counts(const int16_t* labels, const uint32_t hwd[3], int64_t* counts /* [n2][3] = A, I, U */, void* stream);

/* ------------------------------------------------------------------------------------ */
/* K1 backward: frame gradients to voxel grids and transfer-function parameters         */
/* ------------------------------------------------------------------------------------ */
/* For one K1 frame on LINEAR fp32 grids (whole image, shadeMode 0, either camera mode) with C[p] the RGB brats_main writes
 * for pixel p, and an upstream G[p] = dL/dC[p] (grad_rgba: device fp32 RGBA, 16-byte aligned, grad_pitch_px pixels per row;
 * the alpha channel is ignored: the shader writes the constant 1):
 *   grad_vol[m][voxel] += dL/d vol[m][voxel]                   (LINEAR order, every enabled modality)
 *   grad_tf[0..3]      += dL/d(ww, wl, intensityAlpha, gamma)  (device doubles)
 * The function differentiated is the one the forward executed: ray set-up, t0 / t1, the sample positions, their cells and
 * trilinear weights are constants (the forward's own fp32 values), and so are the steps taken: the `t < t1 && T > ert`
 * decisions come from re-marching in the forward's STRICT arithmetic (early ray termination is a discrete decision and
 * carries no gradient).  Label overlays (showSeg, showPred) are fixed occluders: they enter T and the colour behind a
 * sample but receive no gradient.  Not differentiated: camera, stepSize, volWeight, the LUT.  The per-sample chain is
 * written out in csrc/brats_grad.h; its arithmetic is fp64, the voxel sums are float atomic adds (their order, hence
 * the last bits, varies from run to run).  ww must not be 0.
 * Accumulates (+=): the caller zeroes, or keeps summing over views.  grad_vol (or grad_vol[m]) may be NULL for a modality that
 * is disabled or whose gradient is not wanted (a disabled modality's buffer is never touched); grad_tf may be NULL.
 * Checks (before any HIP call): those of every K1 entry point, and
 *   MRIRT_ERR_LAYOUT  ext->layout or ext->labelLayout other than MRIRT_LAYOUT_LINEAR
 *   MRIRT_ERR_ARG     shadeMode != 0, tile sharding, outFormat != MRIRT_OUT_RGBA32F, math != MRIRT_MATH_STRICT */
int mrirt_render_brats_backward(const MrirtBratsParams* params, const MrirtRenderExt* ext,
                                const float* const vol[4], const uint32_t* labels, const uint32_t* preds,
                                const float* grad_rgba, int64_t grad_pitch_px,
                                float* const grad_vol[4], double* grad_tf, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Soft prediction overlay: a differentiable INR render (frame gradients to the logits)  */
/* ------------------------------------------------------------------------------------ */
/* The frame is K1's (brats_rt.slang:85-168) on LINEAR fp32 grids (whole image, shadeMode 0, either camera mode) with the
 * third event of each step, the prediction overlay of :154-162, replaced by a SOFT event that the sample's class
 * probabilities drive.  The forward's own STRICT fp32 values are constants of the frame: ray set-up, t0 / t1, the sample
 * positions, cells and trilinear weights, the intensity event and the ground-truth overlay event (setup_ray, locate,
 * Taps<0, false>, composite with Labels{seg, 0}).  params->showPred is ignored: the soft event takes that overlay's place.
 * The soft event of sample k of ray p (p = y * width + x):
 *   z = logits[offsets[p] + k][0 .. C)    its logits row (fp32, 1 <= C = num_classes <= 16; rows are C floats apart); the
 *                                         numbering is that of mrirt_brats_sample_counts / mrirt_brats_emit_samples, and the
 *                                         caller vouches that every row offsets[p] .. offsets[p] + counts[p] - 1 exists
 *   Kc = min(C, 8),  D = stepSize * 1.5,  w_k = lutColorAlpha[k].w,  rgb_k = lutColorAlpha[k].rgb
 *   p = softmax(z) over all C classes
 *   sigma = sum_{k=1..Kc-1} p_k w_k        E = sum_{k=1..Kc-1} p_k w_k rgb_k
 *   sigma > 0:  alpha = 1 - exp(-sigma D),  c = E / sigma    evaluated in fp64 from the fp32 logits, each rounded ONCE to fp32,
 *               then applied exactly like a label event:  at = alpha T;  C += at c;  T *= (1 - alpha)   (fp32)
 *   sigma <= 0: no event (every LUT opacity zero, C == 1, the softmax underflowed onto class 0).  Classes >= 8 carry
 *               probability mass but draw nothing, as labels >= 8 do in the shader.
 * One-hot probabilities on class l reproduce the hard event of the shader: c == rgb_l exactly, alpha up to the rounding of
 * the fp32 against the fp64 argument of exp.  The loop condition `t < t1 && T > ert` is tested before every step on the fp32
 * state, as in the forward; early termination is a discrete decision and carries no gradient.
 *   stats_dev: optional, ONE device uint64 counter, atomically incremented by the composited samples (steps taken).
 * Backward, with G = dL/dC per pixel (grad_rgba: device fp32 RGBA, 16-byte aligned, grad_pitch_px pixels per row, alpha
 * ignored), T the transmittance in front of a soft event and R = C_final - C_after that event (what all later events add):
 *   dL/dalpha = T (G . c) - (G . R) / (1 - alpha)
 *   dL/dc     = T alpha G
 *   dL/dp_k   = w_k [ dL/dalpha D (1 - alpha) + T alpha G . (rgb_k - c) / sigma ]   for 1 <= k < Kc; 0 for k = 0 and k >= 8
 *   dlogits_j = p_j (dL/dp_j - sum_k p_k dL/dp_k)
 * in fp64 (csrc/brats_soft.h), stored as fp32.  Every row offsets[p] .. offsets[p] + counts[p] - 1 is written with `=`, not
 * `+=`; exact zeros: rows of steps not taken after termination, rows with sigma <= 0, rows of rays whose G is zero in all
 * three channels.  Rays that miss the box own no rows; rows no ray owns are not touched.  Each row has one writer and there
 * are no atomics: the same inputs give the same bits.  Not differentiated: camera, stepSize, the LUT, voxels and transfer
 * function (mrirt_render_brats_backward is for the last two); intensity and ground-truth events are fixed occluders.
 * Checks (before any HIP call): those of every K1 entry point, and
 *   MRIRT_ERR_NULL    logits, offsets, out_rgba / grad_rgba or dlogits is NULL
 *   MRIRT_ERR_LAYOUT  ext->layout or ext->labelLayout other than MRIRT_LAYOUT_LINEAR
 *   MRIRT_ERR_ARG     shadeMode != 0, tile sharding, outFormat != MRIRT_OUT_RGBA32F, math != MRIRT_MATH_STRICT, num_classes
 *                     outside 1..16, lutColorAlpha[k].w negative or not finite for a k in 1..7 */
int mrirt_render_brats_soft(const MrirtBratsParams* params, const MrirtRenderExt* ext, const float* const vol[4],
                            const uint32_t* labels, const float* logits, uint32_t num_classes, const int64_t* offsets,
                            float* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);
int mrirt_render_brats_soft_backward(const MrirtBratsParams* params, const MrirtRenderExt* ext, const float* const vol[4],
                                     const uint32_t* labels, const float* logits, uint32_t num_classes, const int64_t* offsets,
                                     const float* grad_rgba, int64_t grad_pitch_px, float* dlogits, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Per-sample INR render, one call (BASELINE config 5)                                   */
/* ------------------------------------------------------------------------------------ */
/* The same render as ONE call, chunked and ERT-aware (north star: "all LIVE sample points"): the march advances
 * chunk_steps per pass; each pass emits the MLP inputs of the next <= chunk_steps samples of every ray that is
 * still alive (t < t1 and T > 0.01 after the previous pass), classifies that batch with the MFMA forward and
 * composites it, so a ray that has terminated is not classified any further (a ray that terminates inside a pass
 * wastes at most chunk_steps - 1 queries).  Batch sizes stay in device memory: nothing synchronises with the host.
 *   net      : Fourier/ReLU (MRIRT_INR_FOURIER_RELU) or SIREN (MRIRT_INR_SIREN, the 7-input network of
 *              notebooks/neumors_inr.ipynb:853-899,1165-1178: x = (coords, 4 z-scored modalities)), numMods == 4
 *   scratch  : device memory of mrirt_brats_inr_scratch_bytes(params, chunk_steps) bytes, owned by the caller
 *              (58 B per pixel per step of a pass + 64 B per pixel + 12 KiB: 1.5 GB for 512 x 512 x 96)
 *   stats_dev: optional, THREE device uint64 counters, atomically incremented by
 *              {composited (live) samples, gradient-shaded samples, MLP queries}
 * The frame is bit-identical to mrirt_brats_sample_counts / _emit_samples / mrirt_render_brats_stream run over whole rays (the MLP is batch-position invariant).
 * Refused before anything is enqueued or written (besides the checks every K1 entry point shares):
 *   MRIRT_ERR_NULL    params, vol (or a vol[m]; MOD4: vol[0]), net, its weights or biases, zmu, zsigma, scratch or out_rgba is
 *                     NULL; showSeg without labels
 *   MRIRT_ERR_LAYOUT  a label-cell binding, VGA voxels, gradient shading with QUAD or MOD4 voxels
 *   MRIRT_ERR_ARG     tiles; a net that is not Fourier/ReLU or SIREN over four modalities or that mrirt_inr_pack_bytes refuses;
 *                     showPred == 0; chunk_steps outside 1..4096; width x height x chunk_steps >= 2^32 - 2^21;
 *                     scratch_bytes too small; more than 1024 passes (box diagonal / stepSize, stretched by the fp32 drift of
 *                     t += stepSize, over chunk_steps)
 * mrirt_brats_inr_scratch_bytes returns 0 for a chunk_steps or an image it refuses. */
int64_t mrirt_brats_inr_scratch_bytes(const MrirtBratsParams* params, uint32_t chunk_steps);
int mrirt_render_brats_inr(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                           const void* labels, const MrirtInrDesc* net, const float zmu[4], const float zsigma[4],
                           uint32_t chunk_steps, void* scratch, int64_t scratch_bytes,
                           void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Case preparation: percentile window, normalisation, z-score, Gaussian pre-filter      */
/* ------------------------------------------------------------------------------------ */
/* What the reference does to a case on the host before any kernel sees it (inr/viewer/brats_viewer.py:46-65,281-287,
 * scripts/jax_inr_brats.py:266-270), with the same results bit for bit.  Every pointer but `weights` is a device pointer;
 * each call is a chain of launches on `stream`, nothing synchronises with the host, and two calls on the same data give the
 * same bits (integer atomics only; every fp64 sum is taken in an order fixed by n).
 *
 * Window: np.percentile(vol, q) of n fp32 values, default method `linear`, as NumPy evaluates it for fp32 data — with
 * s = sort(vol) (NaN last, -0.0 == +0.0) and every operation a separate fp32 one:
 *   v = f32(n - 1) * (f32(q) / f32(100));  k = floor(v) (at most n - 1);  g = v - f32(k)
 *   a = s[k];  b = s[min(k + 1, n - 1)];  d = b - a;   p = g < 0.5 ? a + d * g : b - d * (1 - g);   NaN if vol holds a NaN
 * record (8 floats) = { lo, hi, span, min, max, p_lo, p_hi, 0 }: (lo, hi) = (p_lo, p_hi), or (min, max) when p_hi <= p_lo;
 * span = f32(max(1e-6, double(hi) - double(lo))) (1e-6 when the difference is NaN).
 * Limits (checked before any HIP call): 1 <= n <= 2^31 - 1, 0 <= q_lo, q_hi <= 100, scratch 16-byte aligned and at least
 * mrirt_prep_scratch_bytes(n) bytes (MRIRT_ERR_ARG).  mrirt_prep_scratch_bytes: with B = min(ceil(n / 4096), 512) histogram blocks,
 * 256 B of state + 8 B per block (rounded up to 256 B) + 4096 B of totals + 4096 B per block; 0 for n outside the limits. */
int64_t mrirt_prep_scratch_bytes(int64_t n);
int mrirt_prep_window(const float* vol, int64_t n, float q_lo, float q_hi, float* record, void* scratch, int64_t scratch_bytes,
                      void* stream);
/* clip((v - lo) / span, 0, 1) in fp32 (correctly rounded division; NaN stays NaN) with lo = record[0], span = record[2] read on
 * the device.  vol: [X][Y][Z] C order, dims = { X, Y, Z }.  norm (may be NULL; may be vol): the same order.  linear (may be
 * NULL; not vol): the x-fastest buffer of the K1 grids, index x + y X + z X Y.  At least one output; X Y Z <= 2^31 - 1. */
int mrirt_prep_normalize(const float* vol, const uint32_t dims[3], const float* record, float* norm, float* linear, void* stream);
/* Z-score over the non-zero voxels of num_mods (1..64) volumes of n values each, mods = [num_mods][n]:
 *   count = #(v != 0);  mu = sum(v) / count;  sigma = sqrt(sum((v - mu)^2) / count)   over v != 0, in fp64
 *   stats (4 num_mods 32-bit words) = { f32 mu[num_mods], f32 sigma[num_mods], f32 divisor[num_mods], u32 count[num_mods] }
 *   with divisor = f32(sigma) + f32(1e-6): mu and divisor are the zmu / zsigma of mrirt_render_brats_inr, which divides by
 *   zsigma as given.
 *   apply: out = (v - mu) / divisor in fp32 for every voxel, zeros included; a volume with count == 0 is copied unchanged.
 *   out may be mods.
 * scratch: 16-byte aligned, mrirt_prep_zscore_scratch_bytes(n, num_mods) bytes; 0 for arguments outside the limits. */
int64_t mrirt_prep_zscore_scratch_bytes(int64_t n, uint32_t num_mods);
int mrirt_prep_zscore_stats(const float* mods, int64_t n, uint32_t num_mods, void* stats, void* scratch, int64_t scratch_bytes,
                            void* stream);
int mrirt_prep_zscore_apply(const float* mods, int64_t n, uint32_t num_mods, const void* stats, float* out, void* stream);
/* scipy.ndimage.gaussian_filter on an fp32 C-order volume, mode `reflect`: axes 0, 1, 2 in that order, each pass in unfused
 * fp64 stored as fp32:  t = x[i] w[r];  for j = -r .. -1:  t += (x[i + j] + x[i - j]) w[j + r];  an index outside the axis
 * reflects as m = i mod 2n, m < n ? m : 2n - 1 - m.  weights: HOST array of 2 radius + 1 doubles (SciPy's: exp(-0.5 x^2 /
 * sigma^2) over its sum, radius = int(4 sigma + 0.5)), read during the call; 0 <= radius <= 16 (MRIRT_ERR_ARG).  out may be
 * vol; scratch is one more volume of the same size; any other overlap is MRIRT_ERR_ARG. */
int mrirt_prep_gaussian3d(const float* vol, const uint32_t dims[3], const double* weights, int32_t radius, float* out,
                          float* scratch, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Coordinate-injection INR: forward, volume prediction, MC-dropout entropy, boundary map */
/* ------------------------------------------------------------------------------------ */
/* Added within ABI 4: new symbols and two new structs only, mrirt_sizeof(17) and (18)   */
/* The third network of the reference (notebooks/improved.ipynb, cells 6 - 10): a learnable Gaussian Fourier projection B, an
 * MLP that takes the coordinates and the modalities again in its hidden layers, dropout after every hidden ReLU.  fp32, every
 * operation separate (the library is built with -ffp-contract=off).  DESIGN.md section 23.
 *
 * Network: L = numLayers linear layers, the head included, 2 <= L <= 8.  Fourier width F = fourierDim, even, 2 <= F <= 256; B is
 * [F / 2][3] fp32, row-major.  M = numMods <= 8.  width[l] (1 <= width[l] <= 256) is layer l's output width; C = width[L - 1]
 * <= 16 classes.  Bit l of coordLayers / modLayers may be set only for 1 <= l <= L - 2 (the head takes h alone).  Input widths:
 *   in_0 = F + M;   in_l = width[l - 1] + 3 [l in coordLayers] + M [l in modLayers]  (1 <= l <= L - 2);   in_{L-1} = width[L - 2]
 * with the concatenation order [h, coords, mods].  w: fp32 [in][out] per layer, the layers one after the other, unpadded; b
 * likewise (the layout of the other fp32 entry points).
 * Features of a point with coordinates c (fp32, unfused, in this order):
 *   c01_a = (c_a + 1.0f) * 0.5f;   p_j = ((c01_x B[j][0]) + (c01_y B[j][1])) + (c01_z B[j][2]);   a_j = 6.2831855f * p_j
 *   (s_j, k_j) = the STRICT sine and cosine of a_j (csrc/siren_sincos.h: float32(sin(double(a))); |a| > 2^20 gives +0 and 1, NaN
 *   and +-inf give NaN);   x0 = [s_0 .. s_{F/2-1}, k_0 .. k_{F/2-1}, mods]
 * Layers: z = x W + b on v_mfma_f32_16x16x4_f32 (products summed in increasing k, the bias added once after the sum), below the
 * head h = max(z, 0) as jnp.maximum has it (-0 gives +0, a NaN stays).  argmax: the first index of the maximum, a NaN counting as
 * the maximum (np.argmax).
 * Dropout (the library's own rule, not JAX's key stream): keep in (0, 1]; keep == 1 masks nothing.  Element (point i, layer
 * l <= L - 2, unit j) of sample s draws Philox4x32-10 under key (seed lo, seed hi) at counter (i lo, i hi, 256 s + l, j >> 2) and
 * takes word j & 3: kept iff word < floor((double)keep 2^32).  A kept value is multiplied by scale = 1.0f / keep (computed once on
 * the host), a dropped one is +0.  i is the GLOBAL point index: index0 + the row for the point entry points, the C-order voxel
 * index (x W + y) D + z for a volume, so neither chunking nor splitting a call changes a mask.
 * Uncertainty: p_s = softmax(logits_s) (subtract the maximum, expf, one division by the sum as a reciprocal multiply);
 *   mean_k = (sum_s p_s[k], s ascending, fp32) / (float)S;   entropy = -(sum_k mean_k * logf(mean_k + 1e-10f)), k ascending. */
typedef struct MrirtInjectDesc {
    uint32_t numLayers, fourierDim, numMods;
    uint32_t width[8];
    uint32_t coordLayers, modLayers;
} MrirtInjectDesc;
typedef struct MrirtInjectDropout {
    uint64_t seed;
    float keep;
    uint32_t samples;          /* S, 1..64; mrirt_inject_forward takes 1 only                                               */
    uint32_t sample0;          /* the first sample's index s (the others follow); sample0 + samples <= 2^24                  */
    uint32_t reserved;         /* 0                                                                                          */
    uint64_t index0;           /* global index of row 0 of a point entry point; 0 for a volume                               */
} MrirtInjectDropout;
/* Every pointer but desc / dropout / hwd is a device pointer; the work is a chain of launches on `stream`, nothing
 * synchronises with the host, nothing is allocated, there are no float atomics and every element has one writer: the same
 * inputs give the same bits.  scratch: 16-byte aligned, at least mrirt_inject_scratch_bytes(desc, n) bytes (n = chunk for a
 * volume); that size is monotone in n and 0 for a refused desc or n outside 1 .. 2^31 - 1.
 * Checked before anything is launched: MRIRT_ERR_NULL for a NULL desc, B, w, b, coords, mods (unless numMods == 0), hwd,
 * scratch or required output; MRIRT_ERR_ARG for a bad shape or injection bit, n / chunk outside 1 .. 2^31 - 1, keep outside
 * (0, 1], samples outside 1..64 (forward: other than 1), sample0 + samples > 2^24, reserved != 0, an axis < 2 or H W D >= 2^31,
 * a misaligned or too-small scratch.
 * forward: coords [n][3], mods [n][M]; logits [n][C] and / or argmax [n] (int16), either may be NULL but not both; dropout NULL
 *   is the evaluation forward.
 * uncertainty: S = dropout->samples passes s = sample0 .. sample0 + S - 1 -> entropy [n]; mean_probs [n][C] may be NULL.
 * predict_volume: mods [M][H][W][D] fp32 C order, the coordinate of index i on an axis of extent E is
 *   ((float)i / (float)(E - 1)) * 2.0f - 1.0f; pred [H][W][D] int16 from the evaluation forward; entropy [H][W][D] fp32 (may be
 *   NULL; then dropout must be NULL too, and with entropy dropout is required); `chunk` points per pass.  The result does not
 *   depend on chunk. */
int64_t mrirt_inject_scratch_bytes(const MrirtInjectDesc* desc, int64_t n);
int mrirt_inject_forward(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                         const float* mods, int64_t n, const MrirtInjectDropout* dropout, float* logits, int16_t* argmax,
                         void* scratch, int64_t scratch_bytes, void* stream);
int mrirt_inject_uncertainty(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                             const float* mods, int64_t n, const MrirtInjectDropout* dropout, float* entropy, float* mean_probs,
                             void* scratch, int64_t scratch_bytes, void* stream);
int mrirt_inject_predict_volume(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* mods,
                                const uint32_t hwd[3], int64_t chunk, const MrirtInjectDropout* dropout, int16_t* pred,
                                float* entropy, void* scratch, int64_t scratch_bytes, void* stream);
/* The boundary weight map of the notebook's cache (cell 5): out[v] = float32(max over c = 1 .. num_classes - 1 of
 * 1.0 / (1.0 + sqrt(d2_c[v]))) in fp64, d2_c the exact squared distance (unit spacing) to the nearest voxel of class c
 * (mrirt_edt_squared); a class that does not occur contributes 0, so the map is 0 where no tumour class is present.
 * labels: int16 [H][W][D]; every axis 1..4096, H W D < 2^31, num_classes 1..32 (else MRIRT_ERR_ARG).  scratch: 16-byte aligned,
 * mrirt_boundary_weights_scratch_bytes(hwd) bytes (one fp64 field; 0 for a refused volume). */
int64_t mrirt_boundary_weights_scratch_bytes(const uint32_t hwd[3]);
int mrirt_boundary_weights(const int16_t* labels, const uint32_t hwd[3], uint32_t num_classes, float* out, void* scratch,
                           int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Coordinate-injection INR: training step (gradients to every W_l, b_l and to B)        */
/* ------------------------------------------------------------------------------------ */
/* Added within ABI 4: three symbols, no new struct.  csrc/inr_inject_train.hip; DESIGN.md section 24.
 * The conventions are those of the section above and of mrirt_inr_forward_f32 / mrirt_inr_loss / mrirt_inr_backward: device
 * pointers (desc and dropout excepted), a chain of launches on `stream`, no host synchronisation, no allocation, no float
 * atomics, one writer per element: the same inputs give the same bits.  One scratch of mrirt_inject_train_scratch_bytes(desc,
 * n) bytes (16-byte aligned; monotone in n; 0 for a refused desc or n) serves forward, loss and backward: its first
 * mrirt_inr_loss_scratch_bytes(n) bytes are the scratch of mrirt_inr_loss, which may be called between the two on the same
 * buffer; behind them lie the features [n][F], every hidden activation after dropout ([n][width[l]] each), dz ping and pong
 * ([n][max hidden width] each), the feature gradient [n][F], c01 [n][3] and min(ceil(n / 256), 64) slabs of
 * max(max_l (in_l + 1) out_l, 3 F / 2) floats, every region aligned to 256 bytes.
 * Refused before anything is launched: MRIRT_ERR_NULL for a NULL desc, B, w, b, coords, mods (unless numMods == 0), logits /
 * dlogits, grad_B, grad_w, grad_b or scratch; MRIRT_ERR_ARG for what mrirt_inject_forward refuses of desc, n and dropout
 * (samples must be 1), a flags bit other than bit 0, a misaligned or too-small scratch.
 *
 * forward_train: exactly mrirt_inject_forward with the same arguments -- logits [n][C] are the same bits -- and the features
 *   and each layer's post-dropout activation h_l stay in the scratch.  dropout NULL or keep == 1: no mask.
 * backward: must follow forward_train on the same scratch and be given the same B, w, coords, mods and dropout (it reads
 *   only keep: scale = 1.0f / keep as in the forward; no Philox word is drawn).  With x_l = [h_{l-1} | coords | mods] as the
 *   forward formed it (x_0 = [s, k, mods]), dz_{L-1} = dlogits, and for l = L - 1 .. 0:
 *     dW_l[i][j] = sum_p x_l[p][i] dz_l[p][j],  db_l[j] = sum_p dz_l[p][j]: slab z covers the points [z len, (z + 1) len), len =
 *       256 doubled until at most 64 slabs cover n; inside a slab the products are summed in increasing p from +0 on
 *       v_mfma_f32_16x16x4_f32; the slabs are added 0, 1, 2, .. (from +0, or from the old value with flags bit 0)
 *     l >= 1:  dh[p][i] = sum_j dz_l[p][j] W_l[i][j], j ascending, for i < width[l - 1] only (the injected rows get no
 *       gradient);  dz_{l-1}[p][i] = dh[p][i] * scale where the saved h_{l-1}[p][i] > 0, else +0 (no multiplication without
 *       dropout; as scale >= 1, "kept and z > 0" is "saved value > 0"; a NaN activation passes no gradient)
 *     l == 0:  dF[p][i] = sum_j dz_0[p][j] W_0[i][j], i < F;   g[p][j] = (dF[p][j] * k_pj) - (dF[p][F / 2 + j] * s_pj), and g = +0
 *       where !(|a_j| <= 2^20), a_j recomputed from B and coords as the features compute it (there the feature is a constant);
 *       dB[j][a] = 6.2831855f * (sum_p g[p][j] c01[p][a]), the sum in slab order, the constant applied once to the finished
 *       sum before it is added to an old value (flags bit 0)
 *   grad_B [F / 2][3]; grad_w, grad_b in the flat unpadded layouts of w and b.  flags bit 0: accumulate into the three.
 *   No gradient reaches coords or mods. */
int64_t mrirt_inject_train_scratch_bytes(const MrirtInjectDesc* desc, int64_t n);
int mrirt_inject_forward_train(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b,
                               const float* coords, const float* mods, int64_t n, const MrirtInjectDropout* dropout,
                               float* logits, void* scratch, int64_t scratch_bytes, void* stream);
int mrirt_inject_backward(const MrirtInjectDesc* desc, const float* B, const float* w, const float* coords,
                          const float* mods, int64_t n, const MrirtInjectDropout* dropout, const float* dlogits,
                          float* grad_B, float* grad_w, float* grad_b, uint32_t flags,
                          void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Unified focal + Dice + TV + boundary loss; the samplers' field gather                 */
/* ------------------------------------------------------------------------------------ */
/* Added within ABI 4: three symbols and one new struct, mrirt_sizeof(20) (19 stays 0).  csrc/inr_unified.hip; DESIGN.md
 * section 25.  The loss of the reference's notebooks/improved.ipynb, cell 8, after the forward: logits [n][C], labels [n],
 * boundary weights [n] (or NULL) -> loss [1], aux [8 + C], dlogits [n][C] (or NULL).  It stands where mrirt_inr_loss stands
 * between mrirt_inject_forward_train and mrirt_inject_backward, with a scratch of its own.  Device pointers (cfg excepted),
 * three launches on `stream` (two without dlogits), no host synchronisation, no allocation, no float atomics, one writer per
 * element: the same inputs give the same bits.
 *
 * Per point, in fp32, with t_k = [label == k] (all 0 for a label outside 0..C-1; no label indexes memory):
 *   zc = clip(z, -10, 10);  ps = softmax(zc);  pc = clip(ps, 1e-7f, 1 - 1e-7f);  pu = softmax(z);  am = first index of max z
 * Sums over the batch, fp64, per-block then in block order:
 *   P_k = sum pc_k   A_k = sum pc_k t_k   T_k = sum t_k   S_k = sum pu_k   Q_k = sum pu_k^2
 *   FL = sum (1 - pc_y + 1e-7)^gamma (-log(pc_y + 1e-10))     (y the label; 0 for a label outside the range)
 *   Bd = sum boundary_w |am - label|  (0 with a NULL boundary_w)     Acc = sum [am == label]
 * Then, in fp64:
 *   TI_k = clip(A_k / (A_k + alpha (P_k - A_k) + beta (T_k - A_k) + 1e-7), 0, 1);  mFTL = mean_k (1 - TI_k + 1e-7)^(1 / gamma)
 *   mFL = FL / n;  ufl = clip(lambda mFTL + (1 - lambda) mFL, 0, 1e6)
 *   dice_k = (2 A_k + 1) / (P_k + T_k + 1);  dl = clip(1 - sum_k dice_k cw_k / (sum_k cw_k + 1e-10), 0, 10)
 *   tv = sum_k (Q_k / n - (S_k / n)^2);  bl = Bd / n
 *   loss = uflWeight ufl + diceWeight dl + tvWeight tv + boundaryWeight bl
 *   aux = [ufl, mFTL, mFL, dl, tv, bl, mean_{k >= 1} dice_k (0 for C == 1), Acc / n, dice_0 .. dice_{C-1}]
 * The notebook's UNIFIED_FOCAL_DELTA is passed to its loss and never read; it has no member here.
 * dlogits is the exact derivative of `loss`: the pc paths through the softmax Jacobian over zc, tv through the one over z.  A clip
 * passes the gradient where lo <= x <= hi and none outside (at an exact tie JAX halves it); the two scalar clips pass none when
 * active; the boundary term and Acc have none (argmax has none).
 * A row holding a logit that is not finite (NaN, +-inf) takes no part: it adds nothing to any sum -- Acc and Bd included, n stays
 * the divisor -- and its dlogits row is +0, so loss, aux and every other row are those of the batch with that row's terms
 * removed.  Finite logits give finite outputs.
 * Refused before anything is launched, in this order: MRIRT_ERR_NULL for a NULL logits, labels, cfg, loss, aux or scratch;
 * MRIRT_ERR_ARG for n outside 1..2^31-1, num_classes outside 1..16, gamma outside [0.25, 1] (the focal derivative gamma
 * base^(gamma - 1) stays bounded there), lambda outside [0, 1], a negative or non-finite tverskyAlpha, tverskyBeta, weight or
 * class weight read, flags != 0, a scratch that is not 16-byte aligned or smaller than mrirt_unified_loss_scratch_bytes(n)
 * (doubles: [min(ceil(n / 256), 256)] rows of 83 partial sums, the totals, the gradient's coefficients; aligned to 256 bytes;
 * monotone in n; 0 for a refused n). */
typedef struct MrirtUnifiedLoss {
    float classWeights[16];     /* first C read (Dice) */
    float gamma, lambda;        /* UNIFIED_FOCAL_GAMMA, UNIFIED_FOCAL_LAMBDA */
    float tverskyAlpha, tverskyBeta;   /* the notebook's 0.3, 0.7 */
    float uflWeight, diceWeight;       /* the notebook's 0.5, 0.5 */
    float tvWeight, boundaryWeight;
    uint32_t flags;             /* must be 0 */
} MrirtUnifiedLoss;
int64_t mrirt_unified_loss_scratch_bytes(int64_t n);
int mrirt_unified_loss(const float* logits, const int32_t* labels, const float* boundary_w /* [n] or NULL */, int64_t n,
                       uint32_t num_classes, const MrirtUnifiedLoss* cfg, float* loss, float* aux /* [8 + C] */,
                       float* dlogits /* [n][C] or NULL */, void* scratch, int64_t scratch_bytes, void* stream);
/* out[i] = fields[case_i][voxel_i], the voxel mrirt_inr_sample_batch draws for point i of (seed, batch_index) when n_tumour == 0
 * and mrirt_inr_sample_batch_mix draws otherwise (the same Philox words through the same functions; one launch).  fields: a
 * device table of cache->ncases device pointers to H W D floats each, in seg's voxel order (the boundary maps of
 * mrirt_boundary_weights, for one).  Refusals: the mixed sampler's, plus MRIRT_ERR_NULL for a NULL fields or out. */
int mrirt_inr_sample_field(const MrirtInrCache* cache, const MrirtInrTumourIndex* tumour, const float* const* fields, uint64_t seed,
                           uint64_t batch_index, int64_t n, int64_t n_tumour, float* out, void* stream);

/* The hybrid, uncertainty-guided sampler of the reference's notebooks/improved.ipynb (cell 9) and the coordinate noise of its
 * cell 12.  Device pointers (the structs excepted), launches on `stream`, no host synchronisation, no allocation, integer
 * atomics only, one writer per element: the same inputs give the same bits.  Every refusal happens before anything is launched,
 * MRIRT_ERR_NULL before MRIRT_ERR_ARG.
 *
 * Class index (load time).  index holds the flat offset (x W + y) D + z of every voxel whose label lies in 0..C-1, ordered by
 * class, then case, then ascending offset; offsets[k ncases + c] is the start of (class k, case c), offsets[C ncases] the
 * length.  Labels outside the range are in no list.  mrirt_inr_class_count writes counts[c][k] (int64, [ncases][C]); the caller
 * reads them once, forms the prefix sums in (class, case) order and sizes index.  mrirt_inr_class_index then fills index in
 * three launches (the counts per chunk of 4096 voxels and class, their scan, the emit): no workgroup waits for another, there is
 * no atomic append, and a slot outside its list's range is never written.  scratch: 16-byte aligned,
 * mrirt_inr_class_index_scratch_bytes(cache, C) bytes (uint32 [ncases][ceil(H W D / 4096)][C], aligned to 256 bytes; 0 for a
 * refused cache or C).  Refused: a NULL cache, counts, offsets, index or scratch (MRIRT_ERR_NULL); H W D >= 2^32, what
 * mrirt_inr_sample_batch refuses of the cache, C outside 1..16, a scratch that is misaligned or too small. */
typedef struct MrirtInrClassIndex {   /* mrirt_sizeof(22) */
    const uint32_t* index;
    const int64_t* offsets;           /* [numClasses * ncases + 1] */
    uint32_t numClasses, reserved;
} MrirtInrClassIndex;
int mrirt_inr_class_count(const MrirtInrCache* cache, uint32_t num_classes, int64_t* counts, void* stream);
int64_t mrirt_inr_class_index_scratch_bytes(const MrirtInrCache* cache, uint32_t num_classes);
int mrirt_inr_class_index(const MrirtInrCache* cache, uint32_t num_classes, const int64_t* offsets, uint32_t* index, void* scratch,
                          int64_t scratch_bytes, void* stream);
/* Exact selection of the k largest of n values, 1 <= k <= n <= 65536 (else MRIRT_ERR_ARG; NULL values or out first).  The values
 * are ordered by a 32-bit key that preserves their order: ~bits for a set sign bit, bits | 2^31 otherwise, so -0 lies below +0;
 * every NaN takes the one key 2^32 - 1 above +inf, as NumPy sorts NaN last.  Among equal keys the higher index ranks higher.
 * out is the k highest-ranking indices in ASCENDING INDEX order: sorted(np.argsort(key, kind="stable")[-k:]).  (The notebook's
 * np.argsort is not stable, so its tie order is unspecified; it returns the picks in entropy order, which its later shuffle
 * discards.)  One launch of one workgroup of 1024 threads, no global scratch: four radix passes over LDS histograms find the
 * k-th key most significant byte first, a workgroup scan ranks the keys equal to it and places the picks. */
int mrirt_select_largest(const float* values, int64_t n, int64_t k, uint32_t* out /* [k] */, void* stream);
/* The unit normals of the coordinate noise.  Point i draws Philox4x32-10 under key `seed` at counter (i, batch lo, batch hi, 2),
 * giving words r0..r3.  In fp64: u1 = (r0 + 1) 2^-32, u2 = r1 2^-32, R = sqrt(-2 log u1), z_x = R cos(2 pi u2), z_y = R sin(2 pi
 * u2); from r2, r3 likewise z_z = R' cos(2 pi u2').  Each is rounded once to fp32.  out: [n][3].  One launch.  Refused: a NULL
 * out; n outside 1..2^31-1. */
int mrirt_inr_normal3(uint64_t seed, uint64_t batch_index, int64_t n, float* out, void* stream);
/* The candidates the uncertainty is computed on: candidate j is mrirt_inr_sample_batch's draw at counter (j, batch lo, batch hi,
 * 1) -- word 3 = 1 keeps the stream apart from the batch's own, which uses 0 -- written as mrirt_inr_sample_batch writes its
 * rows (coords [n_cand][3], feats [n_cand][M], labels [n_cand]).  One launch.  Refusals: mrirt_inr_sample_batch's. */
int mrirt_inr_sample_candidates(const MrirtInrCache* cache, uint64_t seed, uint64_t batch_index, int64_t n_cand, float* coords,
                                float* feats, int32_t* labels, void* stream);
/* One hybrid micro-batch, in one launch.  With U = nUncertain, P = nPerClass, C = classes->numClasses (0 when P == 0), row i is
 *   i < U:            candidate picks[i] (any uint32 is a valid counter: a foreign picks cannot index outside a volume);
 *   U <= i < U + C P: a voxel of class k = (i - U) / P.  With r0..r3 the words of mrirt_inr_sample_batch's point i and total_k =
 *                     offsets[(k + 1) ncases] - offsets[k ncases] > 0: slot = offsets[k ncases] + floor(((r0 << 32) | r1) total_k
 *                     / 2^64), the voxel is index[slot], its case the list that holds slot (a binary search over offsets):
 *                     uniform over all class-k voxels of the cache, the distribution of the notebook's rejection loop, in one
 *                     counter-based draw.  With total_k == 0 the uniform draw of the same words (the notebook pads instead);
 *   otherwise:        mrirt_inr_sample_batch's row i, same bits.
 * The batch is not shuffled, and the remainder of the notebook's n_balanced // C goes to the uniform rows instead of shrinking
 * the batch.  labels, feats and field_out (fields[case][voxel], as mrirt_inr_sample_field) are those of the voxel.  Then, with
 * noiseSigma > 0, coords[i][a] = c + noiseSigma * z_a(i) in fp32, product and sum each rounded, z = mrirt_inr_normal3's for
 * (seed, batch_index, i); noiseSigma == 0 leaves the coordinates untouched.
 * Refused: MRIRT_ERR_NULL for a NULL cache, hybrid, coords, labels, feats with modalities, exactly one of fields / field_out,
 * picks with U > 0, classes or one of its pointers with P > 0; then what mrirt_inr_sample_batch refuses of the cache; then
 * MRIRT_ERR_ARG for n outside 1..2^31-1, U or P outside 0..n, C outside 1..16 or classes->reserved != 0 with P > 0, U + C P > n,
 * a noiseSigma that is negative or not finite, reserved != 0. */
typedef struct MrirtInrHybrid {       /* mrirt_sizeof(23) */
    int64_t nUncertain, nPerClass;
    const uint32_t* picks;            /* device [nUncertain]; may be NULL when nUncertain == 0 */
    float noiseSigma;                 /* >= 0, finite; 0: coordinates untouched */
    uint32_t reserved;                /* 0 */
} MrirtInrHybrid;
int mrirt_inr_sample_batch_hybrid(const MrirtInrCache* cache, const MrirtInrClassIndex* classes /* may be NULL when nPerClass == 0 */,
                                  const MrirtInrHybrid* hybrid, const float* const* fields /* or NULL */, uint64_t seed,
                                  uint64_t batch_index, int64_t n, float* coords, float* feats, int32_t* labels,
                                  float* field_out /* [n], required iff fields */, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Coordinate-injection INR: fused forward, and the per-sample render driven by it      */
/* ------------------------------------------------------------------------------------ */
/* Added within ABI 4: three symbols, no new struct.  csrc/inr_inject_fused.hip, csrc/brats_c5.hip; DESIGN.md section 27.
 * The evaluation forward of the section "Coordinate-injection INR" above as ONE launch: a workgroup keeps the whole network
 * in LDS (every W_l with its input padded to 4 and its output to 16, the biases, B) and each of its waves carries 16 rows
 * from coordinates to class without touching global memory in between.  Features, the order of every layer's products
 * (v_mfma_f32_16x16x4_f32 over k in increasing groups of four from +0, then + bias, then the ReLU) and the argmax are those of
 * mrirt_inject_forward without dropout: logits and classes are the same bits.  No dropout, no scratch, no float atomics, one
 * writer per output.
 * mrirt_inject_fused_lds_bytes: the dynamic LDS the launch asks for, or 0 when the fused path refuses the shape -- a desc
 *   mrirt_inject_forward refuses, or one whose layout exceeds 160 KiB (the notebook's shape takes 143,936 bytes; shapes with a
 *   256-wide layer mostly do not fit).  A refused shape is never served another way.
 * mrirt_inject_classify: coords [n_max][3], mods [n_max][numMods] (may be NULL when numMods == 0), count_dev NULL or a device
 *   word: the call processes min(*count_dev, n_max) rows (n_max without count_dev), read by the kernel itself -- no host
 *   synchronisation; rows at or beyond the count are neither read nor written.  argmax [n_max] int16 and logits [n_max][C]:
 *   either may be NULL, not both.  Refused before any HIP call: MRIRT_ERR_NULL for a NULL desc, B, w, b, coords, mods (unless
 *   numMods == 0) or both outputs; MRIRT_ERR_ARG for a desc mrirt_inject_forward refuses, a shape whose
 *   mrirt_inject_fused_lds_bytes is 0, n_max outside 1 .. 2^31 - 1.
 * mrirt_render_brats_inject: mrirt_render_brats_inr with this network: the same plan / emit / composite launches, the same
 *   scratch of mrirt_brats_inr_scratch_bytes(params, chunk_steps) bytes, the same pass bound, the same three stats_dev
 *   counters and the same refusals, each before anything touches the scratch; the classifier of a pass is the fused forward
 *   over the pass's coordinates and its four z-scored modalities, the batch size read from the device.  Additionally refused:
 *   MRIRT_ERR_NULL for a NULL desc, B, w or b; MRIRT_ERR_ARG for numMods != 4, a shape the fused path refuses, and
 *   imageSize[0] imageSize[1] chunk_steps >= 2^31.  The frame is the same bits as marching with the class stream
 *   mrirt_inject_forward gives for every sample (mrirt_brats_sample_counts, mrirt_brats_emit_samples,
 *   mrirt_render_brats_stream). */
int64_t mrirt_inject_fused_lds_bytes(const MrirtInjectDesc* desc);
int mrirt_inject_classify(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords,
                          const float* mods, int64_t n_max, const uint32_t* count_dev, int16_t* argmax, float* logits,
                          void* stream);
int mrirt_render_brats_inject(const MrirtBratsParams* params, const MrirtRenderExt* ext, const void* const vol[4],
                              const void* labels, const MrirtInjectDesc* desc, const float* B, const float* w, const float* b,
                              const float zmu[4], const float zsigma[4], uint32_t chunk_steps, void* scratch,
                              int64_t scratch_bytes, void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Misc                                                                                  */
/* ------------------------------------------------------------------------------------ */
int mrirt_abi_version(void);
const char* mrirt_status_string(int status);
int mrirt_last_hip_error(void);            /* hipError_t of the last failed HIP call on this thread */
uint32_t mrirt_sizeof(uint32_t which);     /* 0 BratsParams, 1 RenderExt, 2 VolumeParams, 3 SdfParams, 4 InrDesc, 5 Skip,
                                              6 MeshParams, 7 InrCache, 8 AdamW, 9 InrTrainCfg, 10 InrTrainState,
                                              11 Muon, 13 InrLossExt, 14 InrTumourIndex, 15 InrTrainExt, 17 InjectDesc,
                                              18 InjectDropout, 20 UnifiedLoss, 22 InrClassIndex, 23 InrHybrid; 12, 16,
                                              19 and 21 are unassigned and stay 0, as every index beyond 23 */
/* Opt-in diagnostics (host only; the library installs nothing by itself): a SIGABRT handler that writes the native
 * backtrace of the aborting thread and, when file descriptor 2 has been redirected into a regular file (a test runner's
 * capture), the tail of that file to `fd` — a descriptor the caller duplicated before the redirection — and then chains
 * to the handler that was installed before it.  The ROCm runtime reports GPU faults as a line on stderr + abort() from
 * its event thread; under a capturing runner that line is otherwise lost with the process.                              */
int mrirt_install_abort_trace(int fd);

#ifdef __cplusplus
}
#endif
#endif /* MRIRT_H */
