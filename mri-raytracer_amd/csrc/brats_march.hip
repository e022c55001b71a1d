// K1: the BraTS volume ray-marcher — hand-written gfx950 HIP replacement for the Slang compute
// shader `brats_main` (reference: inr/viewer/brats_rt.slang:85-168; helpers :36-83).
//
// One lane = one ray; one wave64 = an 8x8 pixel packet (the reference's numthreads(8,8,1)
// group).  The march loop is a divergent loop: the wave's EXEC mask IS the ballot of live rays,
// and the wave leaves the loop (s_cbranch_execz) when its last lane has terminated (t >= t1 or
// T <= 0.01), so every lane stops accumulating exactly where the scalar shader does.
//
// What bounds it (profiles/r01_*): not HBM bytes.  With dword gathers it was the vector
// L1's tag pipeline (~36 line look-ups per wave-level gather); the shaded float4 kernel still saturates
// it (0.99 look-ups per clock per CU: a sample's cell straddles ~3.4 of the 128-B lines and the kernel makes
// 3.75 look-ups per sample) with VALU issue at 83 %; the unshaded QUAD kernel is VALU-bound (99.8 %) while
// drawing 4-4.6 TB/s from HBM.  How it got there:
//   * layouts where every gather brings 16 useful bytes from a 128-B 2x2x2-voxel brick
//     (VG = value + lattice gradient, QUAD = the four xy neighbours);
//   * a software-pipelined loop (brats_march_pipe_kernel): the gathers of step k+1 are issued before
//     step k is composited.  They are speculative only in that the ray may end at step k; the
//     addresses are clamped into the grid, so the extra fetch is harmless;
//   * one packet per workgroup (64 threads), so a finished packet's wave slot refills at once, and
//     16-pixel bands of packets interleaved over the 8 XCDs (every XCD gets the same mix of long and short rays);
//   * instruction diet for STRICT math: Markstein divisions, a trimmed fp64 exp with SGPR constants,
//     packed-pair trilinear blends, 32-bit cell offsets, specialisations for gamma == 1 / no overlays.
//
// This unit holds the three register-gather march kernels (generic, pipelined, rolling) with the skipping march, the plan
// that picks one (plan_k1 / launch_plan), prepare() and the K1 entry points.  The pipeline's Stage, the skipping march's map
// window and wave reductions are brats_stage.h's (shared with brats_tf.hip, whose table lookup is the EVENT of Stage and of
// composite(); here it is GreyRamp, the default).  Its neighbours, joined by brats_host.h:
//   brats_skip.hip  the pre-pass of exact empty-space skipping (the map's index arithmetic: skip_map.h)
//   brats_order.hip the builder of the dispatch order: long workgroups first, by the steps the last frames recorded (k1_order.h)
//   brats_c5.hip    C5, the per-sample INR render (sample counting, emission, the chunked passes)
//   brats_slab.hip, brats_ring.hip  the LDS marches the plan can select
//
// Template axes: STRICT (bit-faithful to the oracle / FAST: FMA + hardware exp2, rcp), LAYOUT
// (0 linear, 1 4x4x2 fp32 bricks, 2 VG, 3 QUAD), SHADE (lattice-gradient Blinn-Phong extension); the
// pipelined kernel adds NCH (modalities), GAMMA1, LABELS, SKIP (exact empty-space skipping).
#include "brats_host.h"
#include "brats_stage.h"
#include "k1_order.h"

namespace mrirt {

// ---------------------------------------------------------------------------------------
// General kernel: any subset of the four modalities, gathers issued and consumed per step.
// ---------------------------------------------------------------------------------------
template <bool STRICT, int LAYOUT, bool SHADE>
__global__ __launch_bounds__(256) void brats_march_kernel(const K1Args a) {
    using Mm = M<STRICT>;
    __shared__ float4 lutShared[16];
    const float4* lutS = stage_lut(a, lutShared);
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
        const int64_t streamBase = a.classStream != nullptr ? a.rayOffsets[(int64_t)py * a.map.width + px] : 0;
        while (t < t1 && r.T > a.ert) {
            Cell s;
            locate<STRICT>(a, ro, rd, t, s);
            float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
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
            Labels lb;
            fetch_labels_stream(a, s, lb, streamBase + r.nLive); // nLive == index of this step along the ray
            composite<STRICT, SHADE>(a, rd, lb, v, g, r, lutS);
            t += a.stepSize;
        }
    }
    finish(a, kind, oidx, r);
}

// ---------------------------------------------------------------------------------------
// Pipelined kernel: NCH enabled modalities (compacted on the host into a.chan[]).  Two stages
// ping-pong so that while stage A is blended and composited, stage B's gathers (the NEXT step:
// intensities of every enabled modality plus the label fetches) are already in flight; the
// compiler then waits with vmcnt(#gathers of one stage) instead of vmcnt(0).
// ---------------------------------------------------------------------------------------
// LABELS == false: neither overlay is shown, so the stage carries no label words and pIdx dies after
// locate() — about ten VGPRs less across the two stages, which is what lets the kernel fit 4 waves/SIMD.
// SKIP: exact empty-space skipping (march_skip below).  A sample whose 8^3 macro cell is flagged (per launch:
// no enabled modality can lift the transfer function above 0 there and no shown label grid has a label there —
// skip_mask_kernel, brats_skip.hip; a.skipDist holds the flags as an empty-radius map, byte != 0 = flagged) still counts as a
// march step, but composites nothing: the frame and the counters are the same bits as without skipping.
// Second level (a.leap): the map byte r of a sample's macro cell says that every macro cell within Chebyshev distance
// r - 1 is flagged too, so the ray may move 8 (r - 1) voxels along every axis and still be in flagged cells.  When every
// live ray of the packet is in a flagged cell, the packet takes the smallest of its lanes' budgets at
// once: `++nLive; t += stepSize` per step — the march's own running sum and counter, no locate / fetch — and re-primes
// the pipeline where it lands.  Every leapt sample is one the first level would have skipped: same frame, same counters.

// The skipping march (exact empty-space skipping, both levels).  Every lane of the wave stays in the loops; a ray that
// has finished (or never marched) rides along as `!alive`: it counts as empty with unlimited room, issues its gathers
// at cell 0 and composites nothing.  The march alternates between
//   an EMPTY run  — every live ray's sample is flagged: nothing is fetched; with a.leap the packet takes the smallest of
//                   its lanes' budgets (from the map byte: 8 (r - 1) - 1 voxels of room along every axis) in one go; and
//   a DENSE run   — the two-stage pipeline of the plain kernel, gathers always issued (flagged samples at cell 0), left
//                   when the whole packet's next sample is flagged.
// Per step the arithmetic that decides anything (t, the while-condition, the compositing) is the plain kernel's.
// The class stream of C5 is not supported here (the launchers never combine the two).
template <bool STRICT, int LAYOUT, bool SHADE, int NCH, bool GAMMA1, bool LABELS>
__device__ __forceinline__ void march_skip(const K1Args& a, const WaveGrid<LAYOUT>& wg, const float ro[3], const float rd[3],
                                           float t0, float t1, bool marches, RayState& r, const float4* lutS) {
    bool alive = marches;
    if (__ballot(alive) == 0) return;
    float t = t0;
    Stage<LAYOUT, SHADE, NCH, LABELS, true> A, B;
    MapWindow win;
    win.reset();
    // steps per voxel of room along the fastest axis (index-space advance per step = rd / voxelSize * stepSize)
    const float stepsPerVoxel = __builtin_amdgcn_rcpf(fmaxf(fmaxf(fabsf(rd[0] * a.vox[0].r), fabsf(rd[1] * a.vox[1].r)),
                                                            fabsf(rd[2] * a.vox[2].r)) * a.stepSize);
    locate<STRICT>(a, ro, rd, t, A.s);
    uint32_t dA = win.lookup(a, A.s, rd, alive);
    while (true) {
        // invariant: A.s / dA describe the sample at t; for live rays (t < t1 && T > ert) holds
        if (__ballot(alive && dA == 0u) == 0) {                      // every live ray's sample is flagged
            uint32_t n = 1u;
            if (a.leap != 0u) {
                // samples 0 (this one) .. m stay within 8 (dA - 1) - 1 voxels of it along every axis: m + 1 steps are free
                const uint32_t nl = !alive ? 255u : dA >= 2u ? min((uint32_t)((float)(8u * (dA - 1u) - 1u) * stepsPerVoxel), 254u) + 1u : 1u;
                n = wave_min8(nl);
            }
            for (uint32_t i = 0; i < n; ++i) {                       // wave-uniform trip count
                const bool go = alive && t < t1;
                r.nLive += go ? 1u : 0u;
                if (a.debugFlags & 1u) r.nShaded += go ? 1u : 0u;    // (diagnostic, as in Stage::consume)
                t = go ? t + a.stepSize : t;
            }
            alive = alive && t < t1;
            if (__ballot(alive) == 0) break;
            locate<STRICT>(a, ro, rd, t, A.s);
            dA = win.lookup(a, A.s, rd, alive);
            continue;
        }
        A.classify(alive ? dA : 1u);
        A.issue(a, wg);
        bool leave = false;
        while (true) {
            float tn = t + a.stepSize;
            locate<STRICT>(a, ro, rd, tn, B.s);
            uint32_t dB = win.lookup(a, B.s, rd, alive);
            B.classify(alive ? dB : 1u);
            leave = __ballot(alive && dB == 0u) == 0;                // the packet's next sample is flagged throughout
            B.issue(a, wg);                                          // (issued regardless: see Stage::issue)
            if (alive) A.template consume<STRICT, GAMMA1>(a, rd, r, lutS);
            t = alive ? tn : t;
            alive = alive && t < t1 && r.T > a.ert;
            if (leave || __ballot(alive) == 0) { A.s = B.s; dA = dB; break; }
            tn = t + a.stepSize;
            locate<STRICT>(a, ro, rd, tn, A.s);
            dA = win.lookup(a, A.s, rd, alive);
            A.classify(alive ? dA : 1u);
            leave = __ballot(alive && dA == 0u) == 0;
            A.issue(a, wg);
            if (alive) B.template consume<STRICT, GAMMA1>(a, rd, r, lutS);
            t = alive ? tn : t;
            alive = alive && t < t1 && r.T > a.ert;
            if (leave || __ballot(alive) == 0) break;                // A.s / dA already describe the sample at t
        }
        if (__ballot(alive) == 0) break;
    }
}

// TAG: the same code under a second symbol (kernelVariant bit 15).  bench.py's side measurements — tile shares, frames in flight —
// launch the kernel it benches at other sizes and overlapped; under the tag a profiler's per-kernel statistics keep them apart
// from the benched launches.  Instantiated for the benched configuration only (pipe_kernel).
template <bool STRICT, int LAYOUT, bool SHADE, int NCH, bool GAMMA1, bool LABELS, bool SKIP, bool CELLS = false, bool TAG = false>
__global__ __launch_bounds__(256, (LABELS || SKIP) ? 3 : 4) void brats_march_pipe_kernel(const K1Args a) {
    __shared__ float4 lutShared[LABELS ? 16 : 1];
    const float4* lutS = nullptr;
    if constexpr (LABELS) lutS = stage_lut(a, lutShared);
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    const bool marches = kind == 1 && setup_ray(a, px, py, ro, rd, t0, t1) && t0 < t1 && 1.0f > a.ert;   // the while-condition at entry
    WaveGrid<LAYOUT> wg;
    if constexpr (LAYOUT == 4) wg.f = a.vga.ax[vga_pick_axis(a, ro, rd, marches)];      // every lane votes: outside the branch
    else wg.g = &a.grid;
    if constexpr (SKIP) {
        march_skip<STRICT, LAYOUT, SHADE, NCH, GAMMA1, LABELS>(a, wg, ro, rd, t0, t1, marches, r, lutS);
    } else if (marches) {
        // Two stages, each consumed and then re-issued TWO steps ahead:   consume A(k); issue A(k+2); consume B(k+1); issue B(k+3).
        // (Round 2 had "issue B(k+1); consume A(k)": hipcc then guarded the address arithmetic that precedes B's gathers —
        // temporaries in registers it also uses as B's load destinations — with s_waitcnt vmcnt(7) .. vmcnt(1) at the top of
        // every trip, i.e. it waited for A's gathers BEFORE issuing B's, and half of the overlap was gone: seen in the ISA of
        // every pipelined kernel.  In this order every wait sits in front of the blend that needs it and nothing else.)
        // t runs exactly as in the shader: t_{k+1} = t_k + stepSize (brats_rt.slang:164), one running fp32 sum.
        Stage<LAYOUT, SHADE, NCH, LABELS, SKIP, CELLS> A, B;
        constexpr int kN = Stage<LAYOUT, SHADE, NCH, LABELS, SKIP, CELLS>::kLoads;
        // ONE static issue site and ONE wait per stage: a second site (a prologue that primes the stages) makes the stage's
        // registers a phi at the loop header, and the copies the allocator resolves phis with would read gather destinations
        // that are still in flight (tools/check_async_loads.py found exactly that).  So the pipeline fills inside the loop:
        // the first trip skips both consumes (n counts the steps issued so far).
        float tI = t0;                                           // time of the next sample to ISSUE (the running sum)
        float tA = t0, tB = t0;                                  // time of the sample each stage holds
        uint32_t n = 0;
        while (true) {
            if (n != 0u) {
                A.template arrive<kN>(a);                        // B's kN loads may still be in flight
                A.template consume<STRICT, GAMMA1>(a, rd, r, lutS);
                if (!(tB < t1 && r.T > a.ert)) break;            // brats_rt.slang:117 for the next sample (held by B)
            }
            tA = tI;
            locate<STRICT>(a, ro, rd, tA, A.s);                  // beyond the ray's end the sample is speculative: clamped addresses
            A.classify(0u);
            A.issue_async(a, wg);
            tI += a.stepSize;
            if (n != 0u) {
                B.template arrive<kN>(a);
                B.template consume<STRICT, GAMMA1>(a, rd, r, lutS);
                if (!(tA < t1 && r.T > a.ert)) break;
            }
            tB = tI;
            locate<STRICT>(a, ro, rd, tB, B.s);
            B.classify(0u);
            B.issue_async(a, wg);
            tI += a.stepSize;
            n = 1u;
        }
        // the speculative gathers of the stage that was not consumed are still in flight: their destinations must stay
        // untouched until they land (the registers are dead to the compiler from here on)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    finish(a, kind, oidx, r);
}

// ---------------------------------------------------------------------------------------
// Rolling pipeline for the float4 voxel layouts (VG / VGA) with 2..4 modalities — the viewer's shaded
// four-modality frame.  A stage of the kernel above holds every modality's gathers of a step (8 float4 = 32 registers
// per modality, two stages), which only fits for one modality; here the unit in flight is one (step, modality) PAIR:
// while pair k is blended and accumulated, pair k+1's eight gathers are out — the next modality of the same cell, or
// modality 0 of the next step's cell (speculative, clamped addresses).  Two tap sets whatever NCH; the label
// fetches travel with modality 0.  Same arithmetic in the same order as the shader's modality loop.
// ---------------------------------------------------------------------------------------
// SKIP (no overlays): exact empty-space skipping at PACKET granularity — while every live ray of the packet sits in a flagged
// macro cell nothing is fetched and the packet leaps (the empty run of march_skip, verbatim); otherwise the rolling pipeline
// runs as usual, flagged samples included (their val <= 0 composites nothing: same bits either way).  Every lane stays in
// the loops (MapWindow's cross-lane reads need the whole wave); finished rays ride along as !alive.
template <bool STRICT, int LAYOUT, bool SHADE, int NCH, bool GAMMA1, bool LABELS, bool SKIP = false>
__global__ __launch_bounds__(256, 2) void brats_march_roll_kernel(const K1Args a) {
    static_assert(!(SKIP && LABELS), "the skipping rolling kernel draws no overlays");
    using Mm = M<STRICT>;
    __shared__ float4 lutShared[LABELS ? 16 : 1];
    const float4* lutS = nullptr;
    if constexpr (LABELS) lutS = stage_lut(a, lutShared);
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    float ro[3] = { 0.0f, 0.0f, 0.0f }, rd[3] = { 0.0f, 0.0f, 1.0f }, t0 = 0.0f, t1 = 0.0f;
    const bool marches = kind == 1 && setup_ray(a, px, py, ro, rd, t0, t1) && t0 < t1 && 1.0f > a.ert;
    WaveGrid<LAYOUT> wg;
    if constexpr (LAYOUT == 4) wg.f = a.vga.ax[vga_pick_axis(a, ro, rd, marches)];
    else wg.g = &a.grid;
    if constexpr (SKIP) {
        bool alive = marches;
        if (__ballot(alive) != 0) {
            float t = t0;
            MapWindow win;
            win.reset();
            const float stepsPerVoxel = __builtin_amdgcn_rcpf(fmaxf(fmaxf(fabsf(rd[0] * a.vox[0].r), fabsf(rd[1] * a.vox[1].r)),
                                                                    fabsf(rd[2] * a.vox[2].r)) * a.stepSize);
            Taps<LAYOUT, SHADE> tp[2];
            Cell cs[2], c0;
            locate<STRICT>(a, ro, rd, t, c0);
            uint32_t d0 = win.lookup(a, c0, rd, alive);
            while (true) {
                // invariant: c0 / d0 describe the sample at t; for live rays (t < t1 && T > ert) holds
                if (__ballot(alive && d0 == 0u) == 0) {                  // every live ray's sample is flagged: the empty run of march_skip
                    uint32_t n = 1u;
                    if (a.leap != 0u) {
                        const uint32_t nl = !alive ? 255u : d0 >= 2u ? min((uint32_t)((float)(8u * (d0 - 1u) - 1u) * stepsPerVoxel), 254u) + 1u : 1u;
                        n = wave_min8(nl);
                    }
                    for (uint32_t i = 0; i < n; ++i) {
                        const bool go = alive && t < t1;
                        r.nLive += go ? 1u : 0u;
                        if (a.debugFlags & 1u) r.nShaded += go ? 1u : 0u;      // (diagnostic: samples not fetched, as Stage::consume)
                        t = go ? t + a.stepSize : t;
                    }
                    alive = alive && t < t1;
                    if (__ballot(alive) == 0) break;
                    locate<STRICT>(a, ro, rd, t, c0);
                    d0 = win.lookup(a, c0, rd, alive);
                    continue;
                }
                // dense run: the rolling pipeline from the sample at t, left when the whole packet's next sample is flagged
                cs[0] = c0;
                tp[0].template issue<false>(wg.base(a.vol[a.chan[0]]), wg.dims(), cs[0]);
                bool out = false;
                while (!out) {
#pragma unroll
                    for (int sp = 0; sp < 2; ++sp) {
                        if (out) break;
                        float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
                        const float tn = t + a.stepSize;
                        uint32_t dN = 0u;
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const int k = sp * NCH + c;
                            if (c + 1 < NCH) {
                                tp[(k + 1) & 1].template issue<false>(wg.base(a.vol[a.chan[c + 1]]), wg.dims(), cs[sp]);
                            } else {
                                locate<STRICT>(a, ro, rd, tn, cs[sp ^ 1]);
                                dN = win.lookup(a, cs[sp ^ 1], rd, alive);
                                tp[(k + 1) & 1].template issue<false>(wg.base(a.vol[a.chan[0]]), wg.dims(), cs[sp ^ 1]);   // (speculative: dropped on leaving)
                            }
                            float sv, gm[3];
                            tp[k & 1].template eval<STRICT>(cs[sp], sv, gm);
                            const float w = a.weight[a.chan[c]];
                            v = Mm::mad(sv, w, v);
                            if constexpr (SHADE) {
#pragma unroll
                                for (int q = 0; q < 3; ++q) g[q] = Mm::mad(gm[q], w, g[q]);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if (alive) { const Labels none = { 0u, 0u }; composite<STRICT, SHADE, GAMMA1, false>(a, rd, none, v, g, r); }
                        t = alive ? tn : t;
                        alive = alive && t < t1 && r.T > a.ert;
                        if (__ballot(alive && dN == 0u) == 0 || __ballot(alive) == 0) { c0 = cs[sp ^ 1]; d0 = dN; out = true; }
                    }
                }
                if (__ballot(alive) == 0) break;
            }
        }
    } else if (marches) {
        float t = t0;
        Taps<LAYOUT, SHADE> tp[2];                                  // pair k lives in tp[k & 1]
        Cell cs[2];                                                 // cell of the step a pair belongs to: step parity
        Labels lb[2];
        locate<STRICT>(a, ro, rd, t, cs[0]);
        tp[0].template issue<false>(wg.base(a.vol[a.chan[0]]), wg.dims(), cs[0]);
        if constexpr (LABELS) fetch_labels(a, cs[0], lb[0]);
        bool done = false;
        while (!done) {
            // two steps per trip: 2 NCH pairs, so the buffer parity of a pair is a compile-time value
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                if (done) break;
                float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
                const float tn = t + a.stepSize;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int k = sp * NCH + c;                     // pair index inside the trip
                    // request pair k + 1
                    if (c + 1 < NCH) {
                        tp[(k + 1) & 1].template issue<false>(wg.base(a.vol[a.chan[c + 1]]), wg.dims(), cs[sp]);
                    } else {
                        locate<STRICT>(a, ro, rd, tn, cs[sp ^ 1]);  // the next step's cell (the ray may end here: harmless)
                        tp[(k + 1) & 1].template issue<false>(wg.base(a.vol[a.chan[0]]), wg.dims(), cs[sp ^ 1]);
                        if constexpr (LABELS) fetch_labels(a, cs[sp ^ 1], lb[sp ^ 1]);
                    }
                    // consume pair k: brats_rt.slang:123-130, ascending modality order
                    float sv, gm[3];
                    tp[k & 1].template eval<STRICT>(cs[sp], sv, gm);
                    const float w = a.weight[a.chan[c]];
                    v = Mm::mad(sv, w, v);
                    if constexpr (SHADE) {
#pragma unroll
                        for (int q = 0; q < 3; ++q) g[q] = Mm::mad(gm[q], w, g[q]);
                    }
                    // one pair ahead, no more: left alone the scheduler hoists every pair's gathers of the trip to its top
                    // (8 x 32 registers) and spills
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (LABELS) composite<STRICT, SHADE, GAMMA1>(a, rd, lb[sp], v, g, r, lutS);
                else { const Labels none = { 0u, 0u }; composite<STRICT, SHADE, GAMMA1, false>(a, rd, none, v, g, r); }
                t = tn;
                done = !(t < t1 && r.T > a.ert);
            }
        }
    }
    finish(a, kind, oidx, r);
}

// What a K1 launch runs (plan_k1 decides, launch_plan launches): the kernel family and the template arguments of its kernel.
struct K1Plan {
    int status;            // MRIRT_OK, or what the render call returns instead of launching (MRIRT_ERR_LAYOUT)
    int family;            // MrirtKernelFamily; MRIRT_KERNEL_NONE: nothing to launch (a rank that owns no tile)
    bool strict;           // STRICT: MRIRT_MATH_STRICT
    uint32_t layout;       // LAYOUT: MRIRT_LAYOUT_* of the intensity grids
    bool shade;            // SHADE
    int nch;               // NCH of the pipelined / rolling kernels
    bool gamma1;           // GAMMA1: STRICT with gamma == 1
    bool labels;           // LABELS: the kernel carries the label state
    bool skipping;         // SKIP: the kernel marches with the empty-radius map (K1Args::skipDist)
    bool cells;            // CELLS: one label-cell gather per sample (MRIRT_LAYOUT_LABCELL)
    bool tag;              // TAG: the tagged twin (kernelVariant bit 15)
    bool leap;             // K1Args::leap of a skipping launch
};

using K1Kernel = void (*)(K1Args);

// STRICT stands in for `true` and !STRICT for `false` where only STRICT plans take a branch: FAST instantiates no kernel it
// never launches
template <bool STRICT, int LAYOUT, bool SHADE, int NCH>
static K1Kernel pipe_kernel(const K1Plan& pl) {
    if constexpr (LAYOUT == MRIRT_LAYOUT_QUAD || LAYOUT == MRIRT_LAYOUT_MOD4) {
        if (pl.cells) return pl.gamma1 ? brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, true, false, true>
                                       : brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, false, true, false, true>;
    }
    if constexpr (LAYOUT != MRIRT_LAYOUT_LINEAR) {
        if (pl.skipping) return !pl.gamma1 ? brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, false, true, !STRICT>
                              : pl.labels ? brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, true, true>
                                          : brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, !STRICT, true>;
    }
    if constexpr (STRICT && LAYOUT == MRIRT_LAYOUT_VGA && SHADE && NCH == 1) {
        if (pl.tag) return brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, !STRICT, false, false, true>;
    }
    return !pl.gamma1 ? brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, false, true, false>
         : pl.labels ? brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, true, false>
                     : brats_march_pipe_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, !STRICT, false>;
}

template <bool STRICT, int LAYOUT, bool SHADE, int NCH>
static K1Kernel roll_kernel(const K1Plan& pl) {
    if (pl.skipping) return brats_march_roll_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, false, true>;   // (STRICT: gamma == 1)
    return pl.gamma1 ? brats_march_roll_kernel<STRICT, LAYOUT, SHADE, NCH, STRICT, !STRICT>
                     : brats_march_roll_kernel<STRICT, LAYOUT, SHADE, NCH, false, true>;
}

template <bool STRICT, int LAYOUT, bool SHADE>
static K1Kernel layout_kernel(const K1Plan& pl) {
    if constexpr (LAYOUT == MRIRT_LAYOUT_VG || LAYOUT == MRIRT_LAYOUT_VGA) {
        if (pl.family == MRIRT_KERNEL_PIPELINED) return pipe_kernel<STRICT, LAYOUT, SHADE, 1>(pl);
        if (pl.family == MRIRT_KERNEL_ROLLING)
            return pl.nch == 2 ? roll_kernel<STRICT, LAYOUT, SHADE, 2>(pl) : pl.nch == 3 ? roll_kernel<STRICT, LAYOUT, SHADE, 3>(pl)
                                                                          : roll_kernel<STRICT, LAYOUT, SHADE, 4>(pl);
    }
    if constexpr ((LAYOUT == MRIRT_LAYOUT_LINEAR || LAYOUT == MRIRT_LAYOUT_QUAD) && !SHADE) {
        if (pl.family == MRIRT_KERNEL_PIPELINED)
            return pl.nch == 1 ? pipe_kernel<STRICT, LAYOUT, SHADE, 1>(pl) : pl.nch == 2 ? pipe_kernel<STRICT, LAYOUT, SHADE, 2>(pl)
                 : pl.nch == 3 ? pipe_kernel<STRICT, LAYOUT, SHADE, 3>(pl) : pipe_kernel<STRICT, LAYOUT, SHADE, 4>(pl);
    }
    if constexpr (LAYOUT == MRIRT_LAYOUT_MOD4) return pipe_kernel<STRICT, LAYOUT, SHADE, 4>(pl);
    else return brats_march_kernel<STRICT, LAYOUT, SHADE>;
}

// the plan's kernel, launched: no decision is made here
template <bool STRICT>
static int launch_plan(const K1Plan& pl, const K1Args& a, hipStream_t s) {
    if (pl.status != MRIRT_OK || pl.family == MRIRT_KERNEL_NONE) return pl.status;
    if (pl.family == MRIRT_KERNEL_SLAB) return launch_slab_march(a, STRICT, pl.shade, s);
    if (pl.family == MRIRT_KERNEL_RING) return launch_ring_march(a, STRICT, pl.shade, s);
    K1Kernel k = nullptr;
    switch (pl.layout) {                                            // (QUAD and MOD4 plans are unshaded)
        case MRIRT_LAYOUT_LINEAR: k = pl.shade ? layout_kernel<STRICT, 0, true>(pl) : layout_kernel<STRICT, 0, false>(pl); break;
        case MRIRT_LAYOUT_BRICK:  k = pl.shade ? layout_kernel<STRICT, 1, true>(pl) : layout_kernel<STRICT, 1, false>(pl); break;
        case MRIRT_LAYOUT_VG:     k = pl.shade ? layout_kernel<STRICT, 2, true>(pl) : layout_kernel<STRICT, 2, false>(pl); break;
        case MRIRT_LAYOUT_QUAD:   k = layout_kernel<STRICT, 3, false>(pl); break;
        case MRIRT_LAYOUT_VGA:    k = pl.shade ? layout_kernel<STRICT, 4, true>(pl) : layout_kernel<STRICT, 4, false>(pl); break;
        case MRIRT_LAYOUT_MOD4:   k = layout_kernel<STRICT, MRIRT_LAYOUT_MOD4, false>(pl); break;
        default: return MRIRT_ERR_LAYOUT;
    }
    void* args[] = { const_cast<K1Args*>(&a) };
    return launch_k1(reinterpret_cast<const void*>(k), a, args, 0, s);
}

// the workgroup size and the XCD banding of a K1 launch: prepare()'s pixel map, and what mrirt_order_words sizes the
// dispatch-order tables by
static int k1_pixel_map(PixelMap& m, const uint32_t imageSize[2], const MrirtRenderExt* ext, int64_t pitch_px) {
    const uint32_t layout = ext ? ext->layout : (uint32_t)MRIRT_LAYOUT_LINEAR;
    const uint32_t variant = ext ? ext->kernelVariant : 0u;
    // Workgroup = one 8 x 8 packet (64 threads: a finished packet's wave slot refills at once) — except on VGA grids, where
    // a 16 x 16 block of four packets measured 3.7 % faster (1.145 -> 1.10 ms at C3: the four waves' lines meet in one L1).
    // Variant bit 1 flips the choice; the LDS-staged kernel (bit 6) is written for one packet per workgroup.
    // ... while the launch has enough of them to go round: an eighth of the config-4 frame (one GPU of eight: 2048 workgroups of
    // 16 x 16 for 1024 resident ones) ends in a long tail of half-idle CUs — 0.616 ms against 0.500 ms with one-packet
    // workgroups (tools/tile_share_bench.py, profiles/r03_tile_share.txt); from 4096 upwards the big ones win (0.904 vs 0.918).
    uint64_t blocks16 = (uint64_t)((imageSize[0] + 15u) / 16u) * ((imageSize[1] + 15u) / 16u);
    if (ext && ext->tileSize != 0 && ext->tileWorld != 0)
        blocks16 = (uint64_t)mrirt_tiles_for_rank(imageSize[0], imageSize[1], ext->tileSize, ext->tileRank, ext->tileWorld) *
                   ((ext->tileSize + 15u) / 16u) * ((ext->tileSize + 15u) / 16u);
    const bool bigBlocks = ((variant & 2u) != 0u) != (layout == MRIRT_LAYOUT_VGA && (variant & (64u | 2048u)) == 0u && blocks16 >= 4096u);
    // XCD-interleaved bands one workgroup row high by default (8-px bands for 8 x 8 workgroups: config 2 0.606 -> 0.580 ms,
    // K1 at 512^3 level; variant bit 3: contiguous run per XCD; bits 4-5: 16 / 8 / 32 / 64 px)
    const uint32_t bandSel = (variant >> 4) & 3u;
    const uint32_t bandAsked = bandSel == 0 ? (bigBlocks ? 16u : 8u) : bandSel == 1 ? 16u : bandSel == 2 ? 32u : 64u;
    const uint32_t bandPx = (variant & 8u) ? 0u : bandAsked;
    return fill_pixel_map(m, imageSize[0], imageSize[1], pitch_px, ext,
                          bigBlocks ? 16u : 8u, (variant & 1u) ? 0u : 1u, bandPx,
                          // the per-band shift of the workgroup order (PixelMap::bandShift): config 2 0.591 -> 0.457 ms; on the
                          // 16-px workgroups of VGA grids it measured 1.3 % slower (C3), so those keep straight bands.  Bit 9 flips it.
                          ((variant & 512u) == 0u) != bigBlocks);
}

// kernelVariant (MrirtRenderExt): experiments, 0 = library default; every bit is decoded by prepare(), into K1Args::map, Prepared and
// K1Args::debugFlags (bits 7-10 -> debugFlags bits 0-3, bit 12 -> debugFlags bit 5, read by the kernels / brats_ring.hip)
//   bit 0: row-major instead of Morton lane order
//   bit 1: flip the choice of 64- / 256-thread workgroups (256 is the default on big VGA launches)
//   bit 2: no software pipelining (the generic kernel; no skipping)
//   bit 3: one contiguous run of workgroups per XCD instead of bands
//   bits 4-5: XCD band height: 0 = one workgroup row, 1 / 2 / 3 = 16 / 32 / 64 px
//   bit 6: the LDS-staged kernel of brats_slab.hip (VGA, one modality, no overlays, 64-thread workgroups)
//   bit 7: diagnostic counts in stats[1]: the slab kernel's LDS-served samples; the skipping kernels' samples NOT fetched
//          (flagged or leapt); the ring kernel's reads outside a window / samples not served by the ring
//   bit 8: skipping one step at a time (Prepared::leap false: no leaps); the slab kernel counts ring misses, the ring
//          kernel makes no plane fills (timing only)
//   bit 9: every band of an XCD starts at x = 0 (no per-band shift of the workgroup order: PixelMap::bandShift); the ring
//          kernel counts idle lane-rounds in stats[1]
//   bit 10: the ring kernel: every wave takes the gather march
//   bit 11: the plane-synchronous LDS ring kernel of brats_ring.hip (the slab kernel's launches; bit 6 wins)
//   bit 12: the ring kernel: three planes instead of four
//   bit 15: the tagged twin of the benched kernel (same code, another symbol: bench.py's side measurements)
// validate + fill the kernel arguments shared by every K1 and C5 entry point (declared in brats_host.h)
int prepare(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
            const void* labels, const void* preds, bool needVolumes, int64_t pitch_px,
            K1Args& a, Prepared& cfg) {
    if (!p || (needVolumes && !vol)) return MRIRT_ERR_NULL;
    for (int k = 0; k < 3; ++k) if (p->dims[k] < 2) return MRIRT_ERR_DIMS;
    const uint32_t layout = ext ? ext->layout : (uint32_t)MRIRT_LAYOUT_LINEAR;
    const uint32_t labLayout = ext ? ext->labelLayout : (uint32_t)MRIRT_LAYOUT_LINEAR;
    const uint32_t math = ext ? ext->math : (uint32_t)MRIRT_MATH_STRICT;
    const uint32_t fmt = ext ? ext->outFormat : (uint32_t)MRIRT_OUT_RGBA32F;
    const uint32_t variant = ext ? ext->kernelVariant : 0u;
    const bool labCells = labLayout == MRIRT_LAYOUT_LABCELL;              // both overlays' corner labels per cell: QUAD grids only
    const bool mod4 = layout == MRIRT_LAYOUT_MOD4;                       // all four modalities in one float4 grid (vol[0])
    if ((layout > MRIRT_LAYOUT_VGA && !mod4) || (labLayout > MRIRT_LAYOUT_BRICK && !labCells) || math > MRIRT_MATH_FAST || fmt > MRIRT_OUT_RGBA16F)
        return MRIRT_ERR_LAYOUT;
    if (labCells && layout != MRIRT_LAYOUT_QUAD && !mod4) return MRIRT_ERR_LAYOUT;
    if (labCells && mrirt_vec4_elems(p->dims) >= (int64_t)1 << 29) return MRIRT_ERR_DIMS;      // 32-bit byte offsets of 8-byte elements
    if (layout == MRIRT_LAYOUT_VGA)
        for (int c = 0; c < 3; ++c) if (vga_copy_elems(p->dims, c) >= (1ull << 28)) return MRIRT_ERR_DIMS;   // 32-bit byte offsets per copy
    if (mrirt_brick_elems(p->dims) >= (int64_t)1 << 32 || mrirt_vec4_elems(p->dims) >= (int64_t)1 << 32)
        return MRIRT_ERR_DIMS;                                           // 32-bit element offsets
    if (needVolumes) {
        for (int m = 0; m < (mod4 ? 1 : 4); ++m) if ((mod4 || p->volEnabled[m] != 0) && !vol[m]) return MRIRT_ERR_NULL;
        if ((p->showSeg != 0 || (labCells && p->showPred != 0)) && !labels) return MRIRT_ERR_NULL;
    }
    {
        // The march is `while (t < t1 && T > ert) { ...; t += stepSize; }` (brats_rt.slang:117-165) and the C5
        // count / emit loops have no transmittance exit at all: a step that is not a positive finite number, or
        // too small to move t in fp32 at the far end of the box, would spin a wave forever.  The reference UI
        // clamps its slider to >= 0.001 (brats_viewer.py:168); an API caller gets an error code instead of a
        // hung GPU.  Also bounded: the step count of the box diagonal (kMaxStepsPerRay), so that a frame is a
        // finite amount of work.
        const float h = p->stepSize;
        if (!(h > 0.0f) || !isfinite(h)) return MRIRT_ERR_ARG;
        double diag2 = 0.0, dist2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            if (!(p->voxelSize[k] > 0.0f) || !isfinite(p->voxelSize[k]) || !isfinite(p->volMin[k]) || !isfinite(p->eye[k]))
                return MRIRT_ERR_ARG;
            const double ext = (double)p->voxelSize[k] * (double)p->dims[k];
            const double c = (double)p->volMin[k] + 0.5 * ext - (double)p->eye[k];
            diag2 += ext * ext; dist2 += c * c;
        }
        double tMax = sqrt(dist2) + sqrt(diag2);                     // no sample lies farther along any ray
        if (ext && ext->cameraMode == 1u)                            // orthographic origins are offset from the eye
            tMax += fabs((double)ext->orthoHalfHeight) * (1.0 + (double)p->imageSize[0] / fmax(1.0, (double)p->imageSize[1]));
        if (p->farT > 0.0f && isfinite(p->farT)) tMax = fmin(tMax, (double)p->farT);
        const float tFar = (float)tMax;
        if (!isfinite(tFar) || !(tFar + h > tFar)) return MRIRT_ERR_ARG;          // t += stepSize must advance
        if (sqrt(diag2) / (double)h > (double)kMaxStepsPerRay) return MRIRT_ERR_ARG;
        // The strict exp clamps its argument with fmax / fmin, which drop a NaN (exp_f64_to_f32: NaN -> exp(-200) = 0, where the
        // oracle's (float)exp((double)NaN) is NaN).  Its argument is -(val * intensityAlpha) * stepSize with val in (0, 1] and
        // the step finite, so only a NaN intensityAlpha can put a NaN there: refused here rather than rendered differently.
        if (isnan(p->intensityAlpha)) return MRIRT_ERR_ARG;
        // ... and a camera that is not finite makes NaN rays (every pIdx a NaN): nothing to render, refused like the other
        // parameters that are not finite (fovY makes the rays in perspective mode only)
        if (!(ext && ext->cameraMode == 1u) && !isfinite(p->fovY)) return MRIRT_ERR_ARG;
        for (int k = 0; k < 3; ++k) if (!isfinite(p->U[k]) || !isfinite(p->V[k]) || !isfinite(p->W[k])) return MRIRT_ERR_ARG;
    }
    fill_camera(a.cam, p->eye, p->U, p->V, p->W, p->fovY, p->imageSize[0], p->imageSize[1], ext, false);
    int rc = k1_pixel_map(a.map, p->imageSize, ext, pitch_px);
    if (rc != MRIRT_OK) return rc;
    fill_grid_dims(a.grid, p->dims, (layout == MRIRT_LAYOUT_VGA || mod4) ? (uint32_t)MRIRT_LAYOUT_VG : layout);
    fill_vga_dims(a.vga, p->dims);
    fill_label_addr(a.lab, p->dims, labCells ? (uint32_t)MRIRT_LAYOUT_LINEAR : labLayout);
    for (int k = 0; k < 3; ++k) {
        a.bmin[k] = p->volMin[k];
        a.bmax[k] = p->volMin[k] + p->voxelSize[k] * (float)p->dims[k];
        a.vox[k] = make_udiv(p->voxelSize[k]);
        a.halfInvVoxel[k] = 0.5f / p->voxelSize[k];
        a.hiLin[k] = (float)p->dims[k] - 1.001f;
        a.hiLab[k] = (float)p->dims[k] - 1.0f;
        a.bg[k] = p->bgColor[k];
    }
    a.stepSize = p->stepSize; a.nearT = p->nearT; a.farT = p->farT;
    float wSum = 0.0f;
    a.nch = 0;
    for (int m = 0; m < 4; ++m) a.chan[m] = 0;
    for (int m = 0; m < 4; ++m) {
        a.enabled[m] = p->volEnabled[m];
        a.weight[m] = p->volWeight[m];
        a.vol[m] = vol ? vol[m] : nullptr;
        if (p->volEnabled[m] != 0) { wSum += p->volWeight[m]; a.chan[a.nch++] = (uint32_t)m; }   // shader's order
    }
    a.wsum = make_udiv(wSum);
    a.wwDiv = make_udiv(p->ww);
    a.tfLo = p->wl - p->ww * 0.5f;
    a.intensityAlpha = p->intensityAlpha; a.gamma = p->gamma;
    a.showSeg = p->showSeg; a.showPred = p->showPred;
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) a.lut[i][j] = p->lutColorAlpha[i][j];
    for (int i = 0; i < 8; ++i) {
        // brats_rt.slang:147,158 in the oracle's arithmetic: fp32 argument in the written order, exp correctly
        // rounded through fp64, fp32 subtraction
        const float xs = -a.lut[i][3] * a.stepSize;
        const float xp = xs * 1.5f;
        a.segAlpha[i] = 1.0f - (float)exp((double)xs);
        a.predAlpha[i] = 1.0f - (float)exp((double)xp);
    }
    a.ka = ext ? ext->ka : 0.0f; a.kd = ext ? ext->kd : 0.0f; a.ks = ext ? ext->ks : 0.0f;
    a.gradEps = ext ? ext->gradEps : 0.0f;
    a.specPow2 = ext ? ext->specPow2 : 0u;
    a.ert = (ext && ext->ertOverride) ? ext->ertThreshold : 0.01f;   // brats_rt.slang:117
    a.half = fmt == MRIRT_OUT_RGBA16F ? 1u : 0u;
    a.labels = labCells ? nullptr : static_cast<const uint32_t*>(labels);
    a.preds = labCells ? nullptr : static_cast<const uint32_t*>(preds);
    a.labCell = labCells ? static_cast<const uint2*>(labels) : nullptr;
    a.classStream = nullptr; a.rayOffsets = nullptr;
    a.skipDist = nullptr; a.mX = a.mXY = a.mY = a.mZ = 0; a.leap = 0;
    fill_exp_consts(a.ec);
    a.expSmall = (fabsf(p->intensityAlpha * p->stepSize) <= 0.125f) ? 1u : 0u;   // val is in [0, 1]
    a.out = nullptr; a.stats = nullptr;
    a.debugFlags = (variant >> 7) & 15u;
    if (variant & 4096u) a.debugFlags |= 32u;                          // ring kernel: three planes instead of four
    cfg.layout = layout; cfg.math = math;
    cfg.shade = ext && ext->shadeMode != 0;
    cfg.pipe = a.nch >= 1 && !(variant & 4u);
    // the LDS-staged kernel (brats_slab.hip): VGA grids, one modality, no overlays, one packet per workgroup
    cfg.slab = layout == MRIRT_LAYOUT_VGA && (variant & 64u) != 0 && cfg.pipe && a.nch == 1 && p->showSeg == 0 && p->showPred == 0 &&
               a.map.blockPx == 8;
    // the plane-synchronous LDS ring kernel (brats_ring.hip): the same launches
    cfg.ring = layout == MRIRT_LAYOUT_VGA && (variant & 2048u) != 0 && (variant & 64u) == 0 && cfg.pipe && a.nch == 1 && p->showSeg == 0 &&
               p->showPred == 0 && a.map.blockPx == 8 && p->dims[0] >= 16 && p->dims[1] >= 16 && p->dims[2] >= 16;
    cfg.leap = (variant & 256u) == 0u;
    cfg.tag = (variant & 32768u) != 0u;
    return MRIRT_OK;
}

// What a K1 launch may be offered for exact empty-space skipping
enum class SkipOffer {
    None,      // no MrirtSkip (mrirt_render_brats_ex): the only calls that take the LDS kernels, which have no skipping twin
    NoMap,     // a MrirtSkip that cannot serve this launch (skip_sound, or no scratch)
    Map,       // an empty-radius map, if the launch has a kernel that reads one
};

// Which kernel a K1 launch runs (pure: no side effects, no HIP call).
static K1Plan plan_k1(const K1Args& a, const Prepared& cfg, SkipOffer offer) {
    K1Plan pl = {};
    pl.status = MRIRT_OK;
    pl.strict = cfg.math == MRIRT_MATH_STRICT;
    pl.layout = cfg.layout;
    pl.shade = cfg.shade;
    pl.nch = (int)a.nch;
    const bool overlays = a.showSeg != 0 || a.showPred != 0;
    const bool wide = a.grid.wide != 0;                     // grids >= 4 GiB: 64-bit offsets, the generic kernel
    // the pipelined kernels address label words with 32-bit byte offsets (Stage::issue_async) and read no class stream
    // (Stage::issue)
    const uint64_t labelElems = (uint64_t)((a.grid.X + 3u) & ~3u) * ((a.grid.Y + 3u) & ~3u) * ((a.grid.Z + 1u) & ~1u);
    const bool labelsFit = !(overlays && labelElems >= (1ull << 30));
    const bool pipe = cfg.pipe && labelsFit && a.classStream == nullptr;
    int family = MRIRT_KERNEL_GENERIC;
    if (offer == SkipOffer::None && (cfg.slab || cfg.ring)) {
        family = cfg.slab ? MRIRT_KERNEL_SLAB : MRIRT_KERNEL_RING;
    } else if (cfg.layout == MRIRT_LAYOUT_VG || cfg.layout == MRIRT_LAYOUT_VGA) {
        // VG: 8 float4 per modality per stage -> one modality pipelined; more: rolling pairs, without overlays (with overlays the
        // generic kernel measured faster).  VGA: as VG; every copy is < 4 GiB by construction (prepare())
        const bool fits = pipe && (cfg.layout == MRIRT_LAYOUT_VGA || !wide);
        if (fits && a.nch == 1) family = MRIRT_KERNEL_PIPELINED;
        else if (fits && !overlays) family = MRIRT_KERNEL_ROLLING;
    } else if (cfg.layout == MRIRT_LAYOUT_LINEAR) {
        // the plain ABI: 4 register pairs per modality per stage -> up to four, unshaded; 32-bit byte offsets
        if (pipe && !cfg.shade && (uint64_t)a.grid.X * a.grid.Y * a.grid.Z < (1ull << 30)) family = MRIRT_KERNEL_PIPELINED;
    } else if (cfg.layout == MRIRT_LAYOUT_QUAD) {
        // 2 float4 per modality per stage -> up to four; no gradients
        if (cfg.shade) pl.status = MRIRT_ERR_LAYOUT;
        else if (pipe && !wide) family = MRIRT_KERNEL_PIPELINED;
    } else if (cfg.layout == MRIRT_LAYOUT_MOD4) {
        // the pipelined kernel over all four modalities or nothing (grids < 4 GiB, label grids < 2^30 elements, no gradients)
        if (cfg.shade || wide || !labelsFit || a.classStream != nullptr) pl.status = MRIRT_ERR_LAYOUT;
        else family = MRIRT_KERNEL_PIPELINED;
        pl.nch = 4;
    }
    if (pl.status != MRIRT_OK) {
        if (a.map.numBlocks == 0) pl.status = MRIRT_OK;     // (a rank that owns no tile launches nothing: nothing to refuse)
        return pl;
    }
    // the fp64 pow only matters for STRICT (FAST's is two instructions): specialise gamma == 1 there
    pl.gamma1 = pl.strict && a.gamma == 1.0f;
    // SKIP: the pipelined kernels of the float4 layouts and the rolling kernel, for gamma == 1 STRICT and for FAST; a map is
    // used only where the variant asks for the pipelined march (bit 2) and for no LDS kernel
    const bool skipKernel = (family == MRIRT_KERNEL_PIPELINED && cfg.layout != MRIRT_LAYOUT_LINEAR) || family == MRIRT_KERNEL_ROLLING;
    pl.skipping = offer == SkipOffer::Map && cfg.pipe && !cfg.slab && !cfg.ring && skipKernel && (!pl.strict || a.gamma == 1.0f);
    pl.leap = pl.skipping && cfg.leap;
    // label cells: the plain pipelined kernel with one label gather
    pl.cells = family == MRIRT_KERNEL_PIPELINED && a.labCell != nullptr && overlays && !pl.skipping;
    // the label state is dropped where no overlay is shown: STRICT gamma == 1 only (FAST already fits), and in the skipping
    // rolling kernel, which draws no overlays
    pl.labels = (overlays || !pl.gamma1) && !(family == MRIRT_KERNEL_ROLLING && pl.skipping);
    pl.tag = cfg.tag && family == MRIRT_KERNEL_PIPELINED && cfg.layout == MRIRT_LAYOUT_VGA && cfg.shade && a.nch == 1 &&
             pl.gamma1 && !pl.labels && !pl.skipping;
    pl.family = a.map.numBlocks == 0 ? (int)MRIRT_KERNEL_NONE : family;   // (a rank that owns no tile launches nothing)
    return pl;
}

}  // namespace mrirt

using namespace mrirt;

// Can a map serve this launch?  Skipping is sound only where "upper bound <= window floor" implies "contributes nothing":
// positive window width and gamma (pow(0, g) = 0), non-negative weights (monotone sum), a bound for every enabled modality
// and a label summary for every shown overlay; macro coordinates travel through 8-bit wave reductions.  Whether the launch
// has a kernel that reads the map is plan_k1's question.
static bool skip_sound(const MrirtBratsParams* p, const K1Args& a, const MrirtSkip* skip) {
    bool ok = p->ww > 0.0f && p->gamma > 0.0f;
    for (int k = 0; k < 3; ++k) ok = ok && (p->dims[k] + 7) / 8 <= 256;
    for (uint32_t c = 0; c < a.nch && ok; ++c)
        ok = skip->macroUb[a.chan[c]] != nullptr && a.weight[a.chan[c]] >= 0.0f;
    if (p->showSeg != 0 && !skip->macroSeg) ok = false;
    if (p->showPred != 0 && !skip->macroPred) ok = false;
    return ok;
}

// prepare() + plan_k1() of mrirt_render_brats_ex / _skip, with every check they make before launching anything
static int plan_render(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4], const void* labels,
                       const void* preds, const MrirtSkip* skip, int64_t pitch_px, K1Args& a, K1Plan& pl) {
    Prepared cfg;
    const int rc = prepare(p, ext, vol, labels, preds, true, pitch_px, a, cfg);
    if (rc != MRIRT_OK) return rc;
    if (p->showPred != 0 && !preds && a.labCell == nullptr) return MRIRT_ERR_NULL;
    const SkipOffer offer = skip == nullptr ? SkipOffer::None
                          : skip_sound(p, a, skip) && skip->mask != nullptr ? SkipOffer::Map : SkipOffer::NoMap;
    pl = plan_k1(a, cfg, offer);
    if (pl.skipping && (int64_t)skip->maskWords < mrirt_skip_mask_words(p->dims)) return MRIRT_ERR_ARG;
    return pl.status;
}

// Does a launch of this plan take a dispatch order (MrirtOrder)?  The pipelined and rolling kernels over the whole frame,
// marching without an empty-radius map: the launches whose workgroups run for as long as their rays are, in rounds.
static bool order_applies(const K1Plan& pl, const K1Args& a) {
    return (pl.family == MRIRT_KERNEL_PIPELINED || pl.family == MRIRT_KERNEL_ROLLING) && !pl.skipping && a.map.tileSize == 0;
}

extern "C" int mrirt_render_brats_ordered(const MrirtBratsParams* p, const MrirtRenderExt* ext,
                                          const void* const vol[4], const void* labels, const void* preds,
                                          const MrirtSkip* skip, const MrirtOrder* order, void* out_rgba, int64_t pitch_px,
                                          uint64_t* stats_dev, void* stream) {
    K1Args a;
    K1Plan pl;
    const int rc = plan_render(p, ext, vol, labels, preds, skip, pitch_px, a, pl);
    if (rc != MRIRT_OK) return rc;
    // (a rank that owns no tile has no block to write: its compact buffer is empty, and an empty buffer has no address)
    if (!out_rgba && a.map.numBlocks != 0) return MRIRT_ERR_NULL;
    a.out = out_rgba;
    a.stats = stats_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (a rank that owns no tile still builds the map: "this call returned MRIRT_OK" must mean "skip->mask holds the map",
    // which is what a caller's mapReady on the next frame rests on)
    if (pl.skipping) {
        const int rcMap = launch_skip_prepass(p, skip, pl.strict, s, a);     // brats_skip.hip: the map, and a.skipDist / a.mX.. pointing at it
        if (rcMap != MRIRT_OK) return rcMap;
        a.leap = pl.leap ? 1u : 0u;
    }
    if (order != nullptr && order_applies(pl, a)) {
        if (!order->order || !order->steps) return MRIRT_ERR_NULL;
        if (order->classes > kOrderMaxClasses || (uint64_t)order->words < (uint64_t)a.map.chunk * kXcds) return MRIRT_ERR_ARG;
        a.map.order = order->order;
        a.map.steps = order->steps;
        if (order->classes != 0) {                                           // (0: the caller's own table)
            if (launch_order_build == nullptr) return MRIRT_ERR_ARG;         // (a program linked without brats_order.hip)
            const int rcOrder = launch_order_build(a, order->classes, s);    // brats_order.hip
            if (rcOrder != MRIRT_OK) return rcOrder;
        }
    }
    return pl.strict ? launch_plan<true>(pl, a, s) : launch_plan<false>(pl, a, s);
}

extern "C" int mrirt_render_brats_skip(const MrirtBratsParams* p, const MrirtRenderExt* ext,
                                       const void* const vol[4], const void* labels, const void* preds,
                                       const MrirtSkip* skip, void* out_rgba, int64_t pitch_px,
                                       uint64_t* stats_dev, void* stream) {
    return mrirt_render_brats_ordered(p, ext, vol, labels, preds, skip, nullptr, out_rgba, pitch_px, stats_dev, stream);
}

// 1: mrirt_render_brats_ordered with these arguments orders its launch by the scratch it is given; 0: it ignores the scratch
extern "C" int mrirt_brats_order_applicable(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                            const void* labels, const void* preds, const MrirtSkip* skip) {
    K1Args a;
    K1Plan pl;
    const int rc = plan_render(p, ext, vol, labels, preds, skip, p ? (int64_t)p->imageSize[0] : 0, a, pl);
    if (rc != MRIRT_OK) return rc;
    return order_applies(pl, a) ? 1 : 0;
}

// words of MrirtOrder's tables: the workgroups of the untiled launch, padded as the launch pads them (chunk * 8)
extern "C" int64_t mrirt_order_words(const uint32_t imageSize[2], const MrirtRenderExt* ext) {
    PixelMap m;
    if (!imageSize || (ext && ext->tileSize != 0)) return 0;
    if (k1_pixel_map(m, imageSize, ext, (int64_t)imageSize[0]) != MRIRT_OK) return 0;
    return (int64_t)m.chunk * kXcds;
}

extern "C" int mrirt_render_brats_ex(const MrirtBratsParams* p, const MrirtRenderExt* ext,
                                     const void* const vol[4], const void* labels, const void* preds,
                                     void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream) {
    return mrirt_render_brats_skip(p, ext, vol, labels, preds, nullptr, out_rgba, pitch_px, stats_dev, stream);
}

// 1: mrirt_render_brats_skip with these arguments builds (or reuses) an empty-radius map and marches with it; 0: it is the
// plain launch and never touches skip->mask (callers then need no scratch); < 0: the status the render call would return.
extern "C" int mrirt_brats_skip_applicable(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                           const void* labels, const void* preds, const MrirtSkip* skip) {
    if (!skip) return 0;
    K1Args a;
    Prepared cfg;
    const int rc = prepare(p, ext, vol, labels, preds, true, p ? (int64_t)p->imageSize[0] : 0, a, cfg);
    if (rc != MRIRT_OK) return rc;
    return skip_sound(p, a, skip) && plan_k1(a, cfg, SkipOffer::Map).skipping ? 1 : 0;
}

// Which kernel family the render call with these arguments launches (host-only, nothing is launched): MrirtKernelFamily,
// possibly with MRIRT_KERNEL_SKIPPING / MRIRT_KERNEL_LABEL_CELLS or'ed in; < 0: the status the render call would return.
extern "C" int mrirt_brats_kernel_family(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                         const void* labels, const void* preds, const MrirtSkip* skip) {
    K1Args a;
    K1Plan pl;
    const int rc = plan_render(p, ext, vol, labels, preds, skip, p ? (int64_t)p->imageSize[0] : 0, a, pl);
    if (rc != MRIRT_OK) return rc;
    if (pl.family == MRIRT_KERNEL_NONE) return MRIRT_KERNEL_NONE;
    return pl.family | (pl.skipping ? MRIRT_KERNEL_SKIPPING : 0) | (pl.cells ? MRIRT_KERNEL_LABEL_CELLS : 0);
}

extern "C" int mrirt_render_brats(const MrirtBratsParams* params, const float* const vol[4],
                                  const uint32_t* labels, const uint32_t* preds,
                                  float* out_rgba, int64_t pitch_px, void* stream) {
    if (!vol) return MRIRT_ERR_NULL;
    const void* v[4] = { vol[0], vol[1], vol[2], vol[3] };
    return mrirt_render_brats_ex(params, nullptr, v, labels, preds, out_rgba, pitch_px, nullptr, stream);
}

extern "C" int mrirt_render_brats_stream(const MrirtBratsParams* p, const MrirtRenderExt* ext,
                                         const void* const vol[4], const void* labels,
                                         const int16_t* classes, const int64_t* offsets,
                                         void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream) {
    if (!out_rgba || !classes || !offsets) return MRIRT_ERR_NULL;
    if (ext && ext->tileSize != 0) return MRIRT_ERR_ARG;         // whole-frame only
    K1Args a;
    Prepared cfg;
    int rc = prepare(p, ext, vol, labels, nullptr, true, pitch_px, a, cfg);
    if (rc != MRIRT_OK) return rc;
    if (a.labCell != nullptr) return MRIRT_ERR_LAYOUT;           // (the class stream replaces gPreds; label cells carry both grids)
    if (p->showPred == 0) return MRIRT_ERR_ARG;
    a.classStream = classes; a.rayOffsets = offsets;             // (plan_k1: the generic kernel, which reads the stream)
    a.out = out_rgba; a.stats = stats_dev;
    const K1Plan pl = plan_k1(a, cfg, SkipOffer::None);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return pl.strict ? launch_plan<true>(pl, a, s) : launch_plan<false>(pl, a, s);
}
