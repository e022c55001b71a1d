// The pieces of the K1 register-gather march that brats_march.hip (grey ramp) and brats_tf.hip (RGBA table) share beyond
// brats_device.h: the wave reductions and the map window of the skipping march, and the pipeline's Stage.  What a sample's
// intensity does to the ray is the EVENT of composite() and of Stage (brats_device.h: GreyRamp; brats_tf.h: TableEvent).
#pragma once
#include <type_traits>
#include "brats_device.h"
#include "skip_map.h"

namespace mrirt {

// smallest / largest value (0..255) over the wave: eight ballots each (every lane takes part)
__device__ __forceinline__ uint32_t wave_min8(uint32_t v) {
    uint64_t cand = ~0ull;
    uint32_t m = 0;
#pragma unroll
    for (int b = 7; b >= 0; --b) {
        const uint64_t zero = __ballot(((v >> b) & 1u) == 0u) & cand;
        if (zero != 0) cand = zero; else m |= 1u << b;
    }
    return m;
}
__device__ __forceinline__ uint32_t wave_max8(uint32_t v) { return 255u - wave_min8(255u - v); }

// The packet's window on the distance map: the bytes of a 4 x 4 x 4 block of macro cells, one per lane, read back
// with ds_bpermute — a cross-lane move that does not touch vmcnt, so classifying a sample never waits on (or drains)
// the gathers in flight.  The block is moved (64 byte loads and one full wait) only when a live ray's sample leaves it,
// every ten steps or so; it is placed with the packet's extreme cell at the trailing edge of each axis.  ds_bpermute
// returns 0 from lanes that are switched off, which is why the skipping march keeps every lane of the wave in its
// loops (finished rays ride along as `!alive`) instead of letting them exit.  The window's index arithmetic (window_origin,
// window_holds, window_slot, window_fetch_index) is skip_map.h's: host + device.
struct MapWindow {
    uint32_t bytes;                  // lane l: the map byte of macro cell origin + (l & 3, (l >> 2) & 3, l >> 4)
    uint32_t ox, oy, oz;             // wave-uniform
    __device__ __forceinline__ void reset() { bytes = 0u; ox = oy = oz = 0x40000000u; }
    // the map byte of the sample's macro cell; `alive` = this lane's sample matters
    __device__ __forceinline__ uint32_t lookup(const K1Args& a, const Cell& s, const float rd[3], bool alive) {
        const uint32_t cx = s.ix >> 3, cy = s.iy >> 3, cz = s.iz >> 3;
        bool in = window_holds(cx, cy, cz, ox, oy, oz);
        if (__ballot(alive && !in) != 0) {                           // wave-uniform
            const uint32_t lane = threadIdx.x & 63u;
            // trailing edge per axis, by the first live lane's direction of travel (the packet's rays are near-parallel)
            const int first = __ffsll((long long)__ballot(alive)) - 1;
            const bool px = __shfl(rd[0], first) >= 0.0f, py = __shfl(rd[1], first) >= 0.0f, pz = __shfl(rd[2], first) >= 0.0f;
            // (one reduction per axis, the one its direction needs: eight ballots each — px / py / pz are wave-uniform)
            ox = px ? window_origin(true, wave_min8(alive ? cx : 255u), 0u) : window_origin(false, 0u, wave_max8(alive ? cx : 0u));
            oy = py ? window_origin(true, wave_min8(alive ? cy : 255u), 0u) : window_origin(false, 0u, wave_max8(alive ? cy : 0u));
            oz = pz ? window_origin(true, wave_min8(alive ? cz : 255u), 0u) : window_origin(false, 0u, wave_max8(alive ? cz : 0u));
            uint32_t v = a.skipDist[window_fetch_index(ox, oy, oz, lane, a.mX, a.mY, a.mZ, a.mXY)];
            asm volatile("" : "+v"(v));                             // the wait for this load belongs inside the branch
            bytes = v;
            in = window_holds(cx, cy, cz, ox, oy, oz);
        }
        const uint32_t d = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(window_slot(cx, cy, cz, ox, oy, oz) << 2), (int)bytes);
        // a ray that strays from the packet (more than 4 macro cells wide: a tiny image over a large volume) is simply
        // not skipped: 0 = fetch and composite, always correct
        return in ? d : 0u;
    }
};

// CELLS (QUAD grids): the labels come from the MRIRT_LAYOUT_LABCELL grid — ONE 8-byte gather at the cell's own offset for both
// overlays instead of two nearest-voxel gathers (the plain pipelined kernel counts its loads at compile time, hence a template axis;
// the skipping and generic kernels take the same grid through fetch_labels at run time).
// EVENT: what composite() does with the sample's intensity (GreyRamp; the table kernels' TableEvent, brats_tf.h).  The table
// kernels' stages are instances of the existing axes: MOD4 without overlays = LABELS false (8 loads), MOD4 with label cells =
// LABELS and CELLS (9 loads), VGA shaded with one modality = NCH 1, LABELS false (8 loads).
template <int LAYOUT, bool SHADE, int NCH, bool LABELS, bool SKIP, bool CELLS = false, class EVENT = GreyRamp>
struct Stage {
    // MOD4: ONE tap set — the VG grid's eight float4 corners carry all four modalities (which of them are enabled is a run-time
    // property of the frame: a.enabled[], one kernel whatever the viewer's check boxes say; NCH is not used)
    static constexpr bool kMod4 = LAYOUT == MRIRT_LAYOUT_MOD4;
    static_assert(!(kMod4 && SHADE), "MOD4 grids carry no gradients");
    using TapSet = typename std::conditional<kMod4, Taps<2, true>, Taps<kMod4 ? 2 : LAYOUT, SHADE>>::type;
    static constexpr int kSets = kMod4 ? 1 : NCH;
    Cell s;
    TapSet taps[kSets];
    Labels lb;
    u32x2 cw;                        // CELLS: the cell's two label words, in flight with the taps
    uint32_t csh;                    // ... and which nibble of them is this sample's
    uint32_t dist;                   // SKIP: the map byte of the sample's macro cell (0 = fetch and composite)
    bool empty;
    __device__ __forceinline__ void classify(uint32_t d) { dist = d; empty = SKIP && d != 0u; }
    // (The class stream of the whole-ray C5 form is NOT read here: its per-lane "does that sample exist" test put the label
    // loads into a divergent branch, and a load the compiler cannot count past turns every vmcnt of the loop into 0 — for the
    // plain kernels too.  mrirt_render_brats_stream takes the generic kernel.)
    // ---- the asynchronous form (plain pipelined kernels: !SKIP): gathers the compiler does not count, one explicit wait ----
    static constexpr int kTapLoads = kSets * (LAYOUT == 3 ? 2 : LAYOUT == 0 ? 4 : 8);
    static constexpr int kLoads = kTapLoads + (LABELS ? (CELLS ? 1 : 2) : 0);   // vector-memory instructions issue_async() emits
    __device__ __forceinline__ void issue_async(const K1Args& a, const WaveGrid<LAYOUT>& wg) {
        CellOffsets k;
        if constexpr (LAYOUT == 4) k = flat_cell(wg.f, s.ix, s.iy, s.iz);
        else if constexpr (LAYOUT == 0) { k.o = s.ix + s.iy * wg.g->sY + s.iz * wg.g->sZ; k.dx = 1u; k.dy = wg.g->sY; k.dz = wg.g->sZ; }
        else k = vec4_cell(*wg.g, s.ix, s.iy, s.iz);
        if constexpr (kMod4) {
            taps[0].issue_async(wg.base(a.vol[0]), k);
        } else {
#pragma unroll
            for (int c = 0; c < NCH; ++c) taps[c].issue_async(wg.base(a.vol[a.chan[c]]), k);
        }
        if constexpr (LABELS && CELLS) {
            static_assert(LAYOUT == 3 || kMod4, "label cells are stored in the QUAD (= VG = MOD4) grid's element order");
            async_load_words2(cw, a.labCell, k.o << 3);
            csh = label_corner_shift(a, s);
        } else if constexpr (LABELS) {
            // both label gathers are ALWAYS issued (a hidden overlay reads word 0 of the first modality and is masked in
            // arrive()): the count the wait rests on must not depend on the overlays
            const uint32_t ix = (uint32_t)roundf(clampf(s.q[0], 0.0f, a.hiLab[0]));
            const uint32_t iy = (uint32_t)roundf(clampf(s.q[1], 0.0f, a.hiLab[1]));
            const uint32_t iz = (uint32_t)roundf(clampf(s.q[2], 0.0f, a.hiLab[2]));
            const uint32_t off = a.lab.off(ix, iy, iz) << 2;               // sampleLabel, brats_rt.slang:78-83 (label grids < 4 GiB: plan_k1())
            const void* dummy = a.vol[a.chan[0]];
            async_load_u32(lb.seg, a.showSeg != 0 ? (const void*)a.labels : dummy, a.showSeg != 0 ? off : 0u);
            async_load_u32(lb.pred, a.showPred != 0 ? (const void*)a.preds : dummy, a.showPred != 0 ? off : 0u);
        }
    }
    // every load of this stage has landed; YOUNGER = vector-memory instructions issued after them (the other stage's)
    template <int YOUNGER>
    __device__ __forceinline__ void arrive(const K1Args& a) {
        if constexpr (LAYOUT == 3) {
            // exactly this stage's registers as in/out operands (an operand listed twice would be COPIED into a second
            // register in front of the asm: a read of a gather destination that has not landed)
            f32x4 q[2 * NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) { q[2 * c] = __builtin_bit_cast(f32x4, taps[c].q0); q[2 * c + 1] = __builtin_bit_cast(f32x4, taps[c].q1); }
            if constexpr (NCH == 1) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(q[0]), "+v"(q[1]) : "n"(YOUNGER));
            if constexpr (NCH == 2) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2 % (2 * NCH)]), "+v"(q[3 % (2 * NCH)]) : "n"(YOUNGER));
            if constexpr (NCH == 3) asm volatile("s_waitcnt vmcnt(%6)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2 % (2 * NCH)]), "+v"(q[3 % (2 * NCH)]),
                                                 "+v"(q[4 % (2 * NCH)]), "+v"(q[5 % (2 * NCH)]) : "n"(YOUNGER));
            if constexpr (NCH == 4) asm volatile("s_waitcnt vmcnt(%8)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2 % (2 * NCH)]), "+v"(q[3 % (2 * NCH)]),
                                                 "+v"(q[4 % (2 * NCH)]), "+v"(q[5 % (2 * NCH)]), "+v"(q[6 % (2 * NCH)]), "+v"(q[7 % (2 * NCH)]) : "n"(YOUNGER));
#pragma unroll
            for (int c = 0; c < NCH; ++c) { taps[c].q0 = __builtin_bit_cast(float4, q[2 * c]); taps[c].q1 = __builtin_bit_cast(float4, q[2 * c + 1]); }
        } else if constexpr (LAYOUT == 0) {
            // four register pairs per modality; an asm statement takes 30 operands, so the wait names the first two modalities'
            // pairs and a second, empty statement (volatile: it stays behind the wait) names the rest
            f32x2 q[4 * NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) q[4 * c + i] = taps[c].p[i];
            constexpr int N = 4 * NCH;
            if constexpr (NCH == 1) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : "n"(YOUNGER));
            else asm volatile("s_waitcnt vmcnt(%8)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4 % N]), "+v"(q[5 % N]), "+v"(q[6 % N]), "+v"(q[7 % N]) : "n"(YOUNGER));
            if constexpr (NCH == 3) asm volatile("" : "+v"(q[8 % N]), "+v"(q[9 % N]), "+v"(q[10 % N]), "+v"(q[11 % N]));
            if constexpr (NCH == 4) asm volatile("" : "+v"(q[8 % N]), "+v"(q[9 % N]), "+v"(q[10 % N]), "+v"(q[11 % N]), "+v"(q[12 % N]), "+v"(q[13 % N]), "+v"(q[14 % N]), "+v"(q[15 % N]));
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) taps[c].p[i] = q[4 * c + i];
        } else {
            static_assert(LAYOUT == 3 || NCH == 1 || kMod4, "VG / VGA stages hold one modality");
            taps[0].template arrive<YOUNGER>();
        }
        if constexpr (LABELS && CELLS) {
            u32x2 w = cw;
            asm volatile("" : "+v"(w));                                     // (the label words arrived with the taps: same wait)
            labels_from_cell(a, w.x, w.y, csh, lb);
        } else if constexpr (LABELS) {
            uint32_t ls = lb.seg, lp = lb.pred;
            asm volatile("" : "+v"(ls), "+v"(lp));                          // (the label words arrived with the taps: same wait)
            lb.seg = a.showSeg != 0 ? ls : 0u;
            lb.pred = a.showPred != 0 ? lp : 0u;
        }
    }
    __device__ __forceinline__ void issue(const K1Args& a, const WaveGrid<LAYOUT>& wg) {
        // SKIP: a sample that fetches nothing still ISSUES its gathers, all at cell (0,0,0) — loads inside a branch would
        // make every later s_waitcnt vmcnt conservative (the counter retires in order; a load that may or may not have
        // been issued cannot be counted past), i.e. vmcnt(0) everywhere and no pipelining at all: measured 1.8x on a
        // dense volume.  Lanes on one line cost one tag look-up per quad.
        Cell c0 = s;
        if (SKIP && empty) { c0.ix = 0u; c0.iy = 0u; c0.iz = 0u; }
#pragma unroll
        for (int c = 0; c < kSets; ++c) taps[c].template issue<false>(wg.base(a.vol[kMod4 ? 0 : a.chan[c]]), wg.dims(), c0);   // grid (copy) < 4 GiB (plan_k1())
        if constexpr (LABELS) fetch_labels(a, s, lb);
    }
    template <bool STRICT, bool GAMMA1>
    __device__ __forceinline__ void consume(const K1Args& a, const float rd[3], RayState& r, const float4* lutS = nullptr,
                                            const EVENT ev = EVENT()) const {
        using Mm = M<STRICT>;
        if (SKIP && empty) {
            ++r.nLive;
            if (a.debugFlags & 1u) ++r.nShaded;          // diagnostic (kernelVariant bit 7): stats[1] = shaded + samples NOT fetched
            return;
        }
        float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
        if constexpr (kMod4) {
            // the shader's modality loop (brats_rt.slang:121-130) over the four components, ascending, enabled ones only
            float sv[4], rest[3];
            taps[0].template eval<STRICT>(s, sv[0], rest);
            sv[1] = rest[0]; sv[2] = rest[1]; sv[3] = rest[2];
#pragma unroll
            for (int m = 0; m < 4; ++m) if (a.enabled[m] != 0) v = Mm::mad(sv[m], a.weight[m], v);       // uniform branches
        } else
#pragma unroll
        for (int c = 0; c < NCH; ++c) {                      // ascending modality order, as the shader
            float sv, gm[3];
            taps[c].template eval<STRICT>(s, sv, gm);
            const float w = a.weight[a.chan[c]];
            if (!EVENT::kSeesZeroSign && NCH == 1 && w == 1.0f) {
                // the viewer's weights are 1 (brats_viewer.py:130): 0 + s*1 == s up to the sign of a zero, and no
                // later step can tell -0 from +0 (val > 0, |g|, g.d are all blind to it) — a uniform branch, no math.
                // (Grey ramp only: through a table the sign reaches f, a lerp from a row that holds -0, and the frame, and
                // the table's pipelined kernels are held bit-equal to its generic kernel: kSeesZeroSign keeps them on the mad.)
                v = sv;
                if constexpr (SHADE) { g[0] = gm[0]; g[1] = gm[1]; g[2] = gm[2]; }
            } else {
                v = Mm::mad(sv, w, v);
                if constexpr (SHADE) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) g[k] = Mm::mad(gm[k], w, g[k]);
                }
            }
        }
        if constexpr (LABELS) {
            composite<STRICT, SHADE, GAMMA1>(a, rd, lb, v, g, r, lutS, ev);
        } else {
            const Labels none = { 0u, 0u };
            composite<STRICT, SHADE, GAMMA1, false>(a, rd, none, v, g, r, nullptr, ev);
        }
    }
};

}  // namespace mrirt
