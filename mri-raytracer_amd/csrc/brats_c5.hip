// C5: the per-sample INR render of K1's rays — every sample point of the march is classified by the tiny MLP (inr_mlp.hip and its kernel units)
// and composited with the class as the prediction overlay.  Build-defined extension.  Two forms:
//   whole-ray: mrirt_brats_sample_counts + mrirt_brats_emit_samples write every sample's MLP inputs, the caller classifies
//              them, and mrirt_render_brats_stream (brats_march.hip: the generic kernel) marches with the class stream;
//   chunked:   mrirt_render_brats_inr (and mrirt_render_brats_inject of inr_inject_fused.hip, on the same frame loop), ERT-aware, `chunk` steps per pass (see "C5, chunked" below).
// The rays, the cell arithmetic, the gathers and the compositing step are the march's own (brats_device.h); prepare() is
// brats_march.hip's (brats_host.h).
#include "brats_host.h"

namespace mrirt {

// ---------------------------------------------------------------------------------------
// C5 (per-sample INR query): sample counting and MLP-input emission.  Build-defined extension.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_count_kernel(const K1Args a, uint32_t* __restrict__ counts) {
    uint32_t px, py;
    int64_t oidx;
    if (map_pixel(a.map, px, py, oidx) != 1) return;
    float ro[3], rd[3], t0, t1;
    uint32_t n = 0;
    if (setup_ray(a, px, py, ro, rd, t0, t1))
        for (float t = t0; t < t1; t += a.stepSize) ++n;            // the same fp32 accumulation as the march
    counts[(int64_t)py * a.map.width + px] = n;
}

struct EmitArgs {
    UDiv zsigma[4];
    float zmu[4];
    double dimM1[3];             // dim - 1 (fp64 divide: the same expression as predict_volume)
    double rdimM1[3];            // RN(1 / (dim - 1)): Markstein's exact quotient in three fp64 instructions
    const int64_t* offsets;
    float* coords;
    float4* feats;
    float* mix;                  // C5 passes: the sample's weighted intensity (float per row), or with shading
                                 // (intensity, gradient) as float4 per row; and its seg label when showSeg
    uint32_t* seg;
    const float4* geom;          // chunked C5: per pixel (rd, t1), (ro, hit) — written once by the plan kernel
};

// MLP inputs of the sample at index-space cell `s` -> row `row` of coords / feats (shared by the one-pass and
// the chunked emission)
template <bool STRICT, int LAYOUT>
__device__ __forceinline__ void emit_row(const K1Args& a, const EmitArgs& e, const Cell& s, int64_t row, float sv[4]) {
    using Mm = M<STRICT>;
    float z[4];
    if constexpr (LAYOUT == MRIRT_LAYOUT_MOD4) {
        // the four modalities are the four components of ONE float4 grid: the VG grid's eight corner gathers, and the blend
        // its shaded form applies to (v, dx, dy, dz) — each component is sampleLinear's trilinear expression, bit for bit
        Taps<2, true> taps;
        taps.template issue<true>(a.vol[0], a.grid, s);
        float g[3];
        taps.template eval<STRICT>(s, sv[0], g);
        sv[1] = g[0]; sv[2] = g[1]; sv[3] = g[2];
    } else {
        Taps<LAYOUT, false> taps[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) taps[m].template issue<true>(a.vol[m], a.grid, s);      // all gathers in flight first (layouts 0..3)
#pragma unroll
        for (int m = 0; m < 4; ++m) taps[m].template eval<STRICT>(s, sv[m], nullptr);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float v = sv[m];
        z[m] = STRICT ? Mm::divu_data(v - e.zmu[m], e.zsigma[m]) : (v - e.zmu[m]) * e.zsigma[m].r;
    }
    struct __attribute__((packed, aligned(4))) Coord3 { float x, y, z; };      // one 12-byte store (global memory takes it 4-byte aligned)
    float c3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {    // fp64, one rounding: predict_volume's coordinate at lattice points
        // x / (dim - 1) exactly (Markstein: dim - 1 is a small integer, its significand is never all ones)
        const double x = (double)clampf(s.q[k], 0.0f, a.hiLab[k]);
        const double q0 = x * e.rdimM1[k];
        const double q = __builtin_fma(__builtin_fma(-q0, e.dimM1[k], x), e.rdimM1[k], q0);
        c3[k] = (float)(q * 2.0 - 1.0);
    }
    reinterpret_cast<Coord3*>(e.coords)[row] = Coord3{ c3[0], c3[1], c3[2] };
    e.feats[row] = make_float4(z[0], z[1], z[2], z[3]);
}

template <bool STRICT, int LAYOUT>
__global__ __launch_bounds__(256) void emit_samples_kernel(const K1Args a, const EmitArgs e) {
    uint32_t px, py;
    int64_t oidx;
    if (map_pixel(a.map, px, py, oidx) != 1) return;
    float ro[3], rd[3], t0, t1;
    if (!setup_ray(a, px, py, ro, rd, t0, t1)) return;
    int64_t row = e.offsets[(int64_t)py * a.map.width + px];
    for (float t = t0; t < t1; t += a.stepSize, ++row) {
        Cell s;
        locate<STRICT>(a, ro, rd, t, s);
        float sv[4];
        emit_row<STRICT, LAYOUT>(a, e, s, row, sv);
    }
}

// ---------------------------------------------------------------------------------------
// C5, chunked and ERT-aware ("all LIVE sample points", north star): the march advances `chunk` steps per pass.
//   plan:      every ray still alive (t < t1 and T > ert after the previous pass) counts its next <= chunk steps and
//              its wave takes a row range of the pass's batch (one atomic per wave); the batch size stays in device
//              memory (no host round trip);
//   emit:      one thread per row of the batch writes that sample's MLP inputs and what the compositor needs of it
//              besides the class (weighted intensity, gradient when shading, seg label);
//   classify:  mrirt's MFMA forward over that batch (inr_forward_dev_n of inr_mlp.hip, point count read from the device word);
//   composite: the same rays composite those steps from the per-row records, exactly as brats_main does (ERT tested
//              before every step), park their state (t, T, C) — and plan the NEXT pass (the plan kernel itself only
//              runs for the first one).
// A ray that terminates inside a pass has at most chunk - 1 samples classified in vain; a ray that is dead
// costs nothing in later passes.  The frame is the same bits as the one-pass form (the MLP is batch-position
// invariant), which tests/test_gpu_inr_render.py holds it to.
// ---------------------------------------------------------------------------------------
struct C5Ray { float t, T, C0, C1, C2; uint32_t off, cnt, pad; };      // 32 B per pixel; off = first row of the ray's WAVE

// Row numbering of one wave's samples inside a pass's batch, shared by the plan and composite kernels (which run
// the same pixel -> lane map): step k of the wave's rays occupies consecutive rows, in lane order, after the rows of
// steps 0..k-1.  `step(takes)` must be called by every lane of the wave, once per k: it returns false when no lane
// takes step k, and otherwise leaves this lane's row for that step in `row` (meaningful where takes is true).
struct C5Rows {
    uint32_t next, row;
    __device__ explicit C5Rows(uint32_t waveBase) : next(waveBase), row(0u) {}
    __device__ __forceinline__ bool step(bool takes) {
        const uint64_t m = __ballot(takes);
        if (m == 0) return false;
        row = next + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        next += (uint32_t)__popcll(m);
        return true;
    }
};

// The planning step of one pass, for the wave's 64 rays at once (shared by the plan kernel — first pass — and the
// composite kernel, which plans the NEXT pass for the rays it has just advanced: one launch and one round trip of the
// ray records less per pass).  `r` holds the ray's (t, T, C); `goes` = it hit the box and is above the ERT threshold.
__device__ __forceinline__ void c5_plan_rows(const K1Args& a, bool mine, int64_t pix, C5Ray r, bool goes, float t1,
                                             C5Ray* __restrict__ rays, uint2* __restrict__ rowOwner,
                                             uint32_t* __restrict__ counter, uint32_t chunk) {
    uint32_t cnt = 0;
    if (mine && goes) {
        float t = r.t;
        for (; cnt < chunk && t < t1; ++cnt) t += a.stepSize;               // the march's own running sum
    }
    // the wave's row range inside the pass's batch: one atomic per wave
    uint32_t total = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0 && total != 0) base = atomicAdd(counter, total);
    base = __shfl(base, 0);
    if (mine) {
        r.off = base;
        r.cnt = cnt;
        rays[pix] = r;
    }
    // rows in (step, lane) order: the wave's rays that take step k are neighbours in the batch, as they are in the volume
    // each row records its pixel and its t (the running sum again: the emission needs neither the ray record nor k)
    C5Rows rows(base);
    float t = r.t;
    for (uint32_t k = 0; rows.step(cnt > k); ++k, t += a.stepSize)
        if (cnt > k) rowOwner[rows.row] = make_uint2((uint32_t)pix, __float_as_uint(t));   // stores only: nothing waits on them
}

// The ray of every pixel is set up ONCE per frame, here: origin, direction, exit distance and whether it marches go to
// `geom` (two float4 per pixel), which the emission reads per row and the composite kernel per ray and pass.  Setting the ray
// up again for each of its samples was a quarter of the emission's instructions (11 IEEE divisions and two square roots
// against the sample's own three).
__global__ __launch_bounds__(256) void c5_plan_kernel(const K1Args a, C5Ray* __restrict__ rays, float4* __restrict__ geom,
                                                      uint2* __restrict__ rowOwner, uint32_t* __restrict__ counter, uint32_t chunk) {
    uint32_t px, py;
    int64_t oidx;
    const bool mine = map_pixel(a.map, px, py, oidx) == 1;
    C5Ray r = { 0.0f, 1.0f, a.bg[0], a.bg[1], a.bg[2], 0u, 0u, 0u };
    const int64_t pix = mine ? (int64_t)py * a.map.width + px : 0;
    float t1 = 0.0f;
    bool goes = false;
    if (mine) {
        float ro[3], rd[3], t0;
        const bool hit = setup_ray(a, px, py, ro, rd, t0, t1);
        goes = hit && r.T > a.ert;
        r.t = t0;
        geom[2 * pix] = make_float4(rd[0], rd[1], rd[2], t1);                     // what every reader needs
        geom[2 * pix + 1] = make_float4(ro[0], ro[1], ro[2], hit ? 1.0f : 0.0f);  // (perspective: the origin is the eye — read only under an orthographic camera)
    }
    c5_plan_rows(a, mine, pix, r, goes, t1, rays, rowOwner, counter, chunk);
}

// One thread per ROW of the pass's batch (not per ray): the emission of a pass is ~10^6 independent samples, each
// of them eight gathers and a few hundred flops, and a per-ray loop serialises a ray's 32 behind one another's
// memory latency with one wave per SIMD slot to hide it (measured: 0.18 ms per pass at 512^2, 1.6 ms of a
// 10.5 ms frame).  The rows of a wave are the same step of neighbouring rays (C5Rows), so the gathers stay as
// coherent as the march's own and the stores are contiguous; the plan recorded each row's pixel and t.
#ifndef MRIRT_EMIT_RUN
#define MRIRT_EMIT_RUN 8
#endif
constexpr uint32_t kEmitRun = MRIRT_EMIT_RUN;
template <bool STRICT, int LAYOUT, bool SHADE>
__global__ __launch_bounds__(256) void c5_emit_kernel(const K1Args a, const EmitArgs e, const uint2* __restrict__ rowOwner,
                                                      const uint32_t* __restrict__ counter) {
    using Mm = M<STRICT>;
    const uint32_t n = *counter, nGroups = (n + 255u) >> 8;
    // a workgroup takes kEmitRun consecutive 256-row groups at a time: the rows of a wave's rays follow one another step by
    // step (C5Rows), so a run is ~kEmitRun * 4 consecutive steps of the same 64 rays on one CU.  (Measured level with a plain
    // grid stride — runs of 1 / 4 / 8 groups 219 / 214 / 219 us per pass, 24: 232 — the emission is bound by the number of
    // its vector-memory instructions, not by where their lines are; kept at 8.)
    for (uint32_t g0 = blockIdx.x * kEmitRun; g0 < nGroups; g0 += gridDim.x * kEmitRun)
    for (uint32_t j = 0; j < kEmitRun && g0 + j < nGroups; ++j) {
        const uint32_t row = ((g0 + j) << 8) + threadIdx.x;
        if (row >= n) break;
        const uint2 own = rowOwner[row];
        const float4 ga = e.geom[2 * (size_t)own.x];
        float ro[3] = { a.cam.eye[0], a.cam.eye[1], a.cam.eye[2] };               // perspective: primary_ray's origin
        if (a.cam.mode != 0) { const float4 gb = e.geom[2 * (size_t)own.x + 1]; ro[0] = gb.x; ro[1] = gb.y; ro[2] = gb.z; }   // uniform
        const float rd[3] = { ga.x, ga.y, ga.z };
        const float t = __uint_as_float(own.y);
        Cell s;
        locate<STRICT>(a, ro, rd, t, s);
        float sv[4];
        emit_row<STRICT, LAYOUT>(a, e, s, (int64_t)row, sv);
        // what the composite pass needs of this sample besides its class: brats_rt.slang:121-141's weighted
        // intensity (and gradient) over the enabled modalities, in the march's own order, and the seg label
        float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (a.enabled[m] != 0) {
                if constexpr (SHADE) {
                    Taps<LAYOUT, true> taps;
                    float gm[3];
                    taps.template issue<true>(a.vol[m], a.grid, s);
                    taps.template eval<STRICT>(s, sv[m], gm);
#pragma unroll
                    for (int q = 0; q < 3; ++q) g[q] = Mm::mad(gm[q], a.weight[m], g[q]);
                }
                v = Mm::mad(sv[m], a.weight[m], v);
            }
        }
        if constexpr (SHADE) {
            reinterpret_cast<float4*>(e.mix)[row] = make_float4(v, g[0], g[1], g[2]);
            if (a.showSeg != 0) e.seg[row] = sample_label(a.labels, a.lab, s.q, a.hiLab);
        } else {                     // unshaded: (weighted intensity, seg label) as ONE 8-byte record in the mix array
            const uint32_t l = a.showSeg != 0 ? sample_label(a.labels, a.lab, s.q, a.hiLab) : 0u;
            reinterpret_cast<uint2*>(e.mix)[row] = make_uint2(__float_as_uint(v), l);
        }
    }
}

// The sequential part of a pass: every ray composites its <= chunk samples front to back from the per-row
// records (class from the MLP; intensity, gradient and seg label from the emission) — no volume access, and the
// next step's records are in flight while this step composites.
template <bool STRICT, bool SHADE>
__global__ __launch_bounds__(256) void c5_composite_kernel(const K1Args a, C5Ray* __restrict__ rays, const float4* __restrict__ geom,
                                                           const int16_t* __restrict__ classes,
                                                           const float* __restrict__ mix, const uint32_t* __restrict__ seg,
                                                           uint2* __restrict__ rowOwner, uint32_t* __restrict__ nextCounter,
                                                           uint32_t chunk) {
    __shared__ float4 lutShared[16];
    const float4* lutS = stage_lut(a, lutShared);
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    RayState r = { a.bg[0], a.bg[1], a.bg[2], 1.0f, 0u, 0u };
    const int64_t pix = kind == 1 ? (int64_t)py * a.map.width + px : 0;
    C5Ray st = { 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0u, 0u, 0u };
    float rd[3] = { 0.0f, 0.0f, 1.0f }, t1 = 0.0f;
    bool hit = false;
    if (kind == 1) {
        st = rays[pix];
        r.C0 = st.C0; r.C1 = st.C1; r.C2 = st.C2; r.T = st.T;
        if (nextCounter != nullptr || (SHADE && st.cnt != 0)) {
            const float4 g0 = geom[2 * pix];
            rd[0] = g0.x; rd[1] = g0.y; rd[2] = g0.z; t1 = g0.w;
            hit = geom[2 * pix + 1].w != 0.0f;
        }
    }
    struct Rec { float v, g[3]; Labels lb; };
    auto fetch = [&](uint32_t row, bool takes, Rec& c) {
        c.v = 0.0f; c.g[0] = c.g[1] = c.g[2] = 0.0f; c.lb.seg = 0u; c.lb.pred = 0u;
        if (takes) {
            if constexpr (SHADE) {
                const float4 m = reinterpret_cast<const float4*>(mix)[row];
                c.v = m.x; c.g[0] = m.y; c.g[1] = m.z; c.g[2] = m.w;
                if (a.showSeg != 0) c.lb.seg = seg[row];
            } else {
                const uint2 m = reinterpret_cast<const uint2*>(mix)[row];
                c.v = __uint_as_float(m.x);
                c.lb.seg = m.y;                  // (0 when the overlay is off: the emission wrote it so)
            }
            c.lb.pred = (uint32_t)(uint16_t)classes[row];
        }
    };
    float t = st.t;
    bool alive = true;
    C5Rows rows(st.off);
    Rec cur, nxt;
    bool more = rows.step(st.cnt > 0u);
    fetch(rows.row, st.cnt > 0u, cur);
    for (uint32_t k = 0; more; ++k) {
        more = rows.step(st.cnt > k + 1u);
        fetch(rows.row, more && st.cnt > k + 1u, nxt);
        // brats_rt.slang:117: `while (t < t1 && T > 0.01)` — t < t1 holds for these cnt steps by construction
        alive = alive && st.cnt > k && r.T > a.ert;
        if (__ballot(alive) == 0) break;                 // every ray of the wave is done with this pass
        if (alive) {
            composite<STRICT, SHADE>(a, rd, cur.lb, cur.v, cur.g, r, lutS);
            t += a.stepSize;
        }
        cur = nxt;
    }
    st.t = t; st.T = r.T; st.C0 = r.C0; st.C1 = r.C1; st.C2 = r.C2;
    // the next pass's plan for these rays (nullptr after the last pass: nothing is parked)
    if (nextCounter != nullptr) c5_plan_rows(a, kind == 1, pix, st, hit && r.T > a.ert, t1, rays, rowOwner, nextCounter, chunk);
    finish(a, kind, oidx, r);      // the frame so far (complete after the last pass); live-sample counters
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_brats_sample_counts(const MrirtBratsParams* p, const MrirtRenderExt* ext, uint32_t* counts, void* stream) {
    if (!counts) return MRIRT_ERR_NULL;
    if (ext && ext->tileSize != 0) return MRIRT_ERR_ARG;
    K1Args a;
    Prepared cfg;
    int rc = prepare(p, ext, nullptr, nullptr, nullptr, false, p ? p->imageSize[0] : 0, a, cfg);
    if (rc != MRIRT_OK) return rc;
    hipLaunchKernelGGL(sample_count_kernel, dim3(a.map.chunk * kXcds), dim3(a.map.blockPx == 8 ? 64 : 256), 0,
                       static_cast<hipStream_t>(stream), a, counts);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

template <bool STRICT>
static int launch_emit(const K1Args& a, const EmitArgs& e, uint32_t layout, hipStream_t s) {
    if (layout > MRIRT_LAYOUT_QUAD && layout != MRIRT_LAYOUT_MOD4) return MRIRT_ERR_LAYOUT;      // the C5 passes read LINEAR / BRICK / VG / QUAD / MOD4 grids
    const dim3 grid(a.map.chunk * kXcds), block(a.map.blockPx == 8 ? 64 : 256);
    switch (layout) {
        case MRIRT_LAYOUT_LINEAR: hipLaunchKernelGGL((emit_samples_kernel<STRICT, 0>), grid, block, 0, s, a, e); break;
        case MRIRT_LAYOUT_BRICK:  hipLaunchKernelGGL((emit_samples_kernel<STRICT, 1>), grid, block, 0, s, a, e); break;
        case MRIRT_LAYOUT_VG:     hipLaunchKernelGGL((emit_samples_kernel<STRICT, 2>), grid, block, 0, s, a, e); break;
        case MRIRT_LAYOUT_MOD4:   hipLaunchKernelGGL((emit_samples_kernel<STRICT, MRIRT_LAYOUT_MOD4>), grid, block, 0, s, a, e); break;
        default:                  hipLaunchKernelGGL((emit_samples_kernel<STRICT, 3>), grid, block, 0, s, a, e); break;
    }
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_brats_emit_samples(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                        const float zmu[4], const float zsigma[4], const int64_t* offsets,
                                        float* coords, float* feats, void* stream) {
    if (!vol || !zmu || !zsigma || !offsets || !coords || !feats) return MRIRT_ERR_NULL;
    for (int m = 0; m < 4; ++m) if (!vol[m]) return MRIRT_ERR_NULL;          // the MLP reads all four modalities
    if (ext && ext->tileSize != 0) return MRIRT_ERR_ARG;
    K1Args a;
    Prepared cfg;
    int rc = prepare(p, ext, vol, nullptr, nullptr, false, p ? p->imageSize[0] : 0, a, cfg);
    if (rc != MRIRT_OK) return rc;
    EmitArgs e;
    for (int m = 0; m < 4; ++m) { e.zmu[m] = zmu[m]; e.zsigma[m] = make_udiv(zsigma[m]); }
    for (int k = 0; k < 3; ++k) { e.dimM1[k] = (double)(p->dims[k] - 1); e.rdimM1[k] = 1.0 / e.dimM1[k]; }
    e.offsets = offsets; e.coords = coords; e.feats = reinterpret_cast<float4*>(feats); e.mix = nullptr; e.seg = nullptr; e.geom = nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return cfg.math == MRIRT_MATH_STRICT ? launch_emit<true>(a, e, cfg.layout, s) : launch_emit<false>(a, e, cfg.layout, s);
}

// ---------------------------------------------------------------------------------------
// C5 as one call: the chunked, ERT-aware per-sample INR render (see c5_plan_kernel).  Everything is enqueued on
// `stream`; batch sizes travel through device memory, so there is no host synchronisation inside the frame.
// ---------------------------------------------------------------------------------------
namespace mrirt {

__global__ void c5_sum_kernel(const uint32_t* __restrict__ counters, uint32_t n, uint64_t* __restrict__ queries) {
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 64) s += counters[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(queries), (unsigned long long)s);
}

static int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

static int c5_carve(const MrirtBratsParams* p, uint32_t chunk, void* base, C5Scratch& sc) {
    if (!p || chunk == 0 || chunk > 4096) return MRIRT_ERR_ARG;
    const int64_t px = (int64_t)p->imageSize[0] * p->imageSize[1];
    if (px <= 0) return MRIRT_ERR_DIMS;
    sc.cap = px * chunk;
    if (sc.cap >= ((int64_t)1 << 32) - ((int64_t)1 << 21)) return MRIRT_ERR_ARG;   // 32-bit row numbers per pass (+ one grid stride of headroom)
    char* b = static_cast<char*>(base);
    int64_t o = 0;
    sc.counters = reinterpret_cast<uint32_t*>(b + o); o += align256((int64_t)kC5MaxPasses * 8);     // batch sizes, then the refinement's segment tickets
    sc.rays = reinterpret_cast<C5Ray*>(b + o);        o += align256(px * (int64_t)sizeof(C5Ray));
    sc.geom = reinterpret_cast<float4*>(b + o);       o += align256(px * 32);
    sc.rowOwner = reinterpret_cast<uint2*>(b + o);    o += align256(sc.cap * 8);
    sc.coords = reinterpret_cast<float*>(b + o);      o += align256(sc.cap * 12);
    sc.feats = reinterpret_cast<float*>(b + o);       o += align256(sc.cap * 16);
    sc.mix = reinterpret_cast<float*>(b + o);         o += align256(sc.cap * 16);
    sc.seg = reinterpret_cast<uint32_t*>(b + o);      o += align256(sc.cap * 4);
    sc.classes = reinterpret_cast<int16_t*>(b + o);   o += align256(sc.cap * 2);
    sc.bytes = o;
    return MRIRT_OK;
}

// the C5 passes read LINEAR / BRICK / VG / QUAD / MOD4 grids; QUAD and MOD4 carry no gradients
static bool c5_layout_ok(uint32_t layout, bool shade) {
    const bool flat = layout == MRIRT_LAYOUT_QUAD || layout == MRIRT_LAYOUT_MOD4;
    return (layout <= MRIRT_LAYOUT_QUAD || layout == MRIRT_LAYOUT_MOD4) && !(flat && shade);
}

template <bool STRICT>
static int c5_launch_plan(const K1Args& a, const EmitArgs& e, uint32_t layout, bool shade, const C5Scratch& sc, uint32_t pass,
                          uint32_t chunk, hipStream_t s) {
    if (!c5_layout_ok(layout, shade)) return MRIRT_ERR_LAYOUT;
    uint32_t* counter = sc.counters + pass;
    if (pass == 0) {                                                  // later passes are planned by the composite kernel
        hipLaunchKernelGGL(c5_plan_kernel, dim3(a.map.chunk * kXcds), dim3(a.map.blockPx == 8 ? 64 : 256), 0, s,
                           a, sc.rays, sc.geom, sc.rowOwner, counter, chunk);
        MRIRT_HIP(hipGetLastError());
    }
    const int64_t blocksWanted = (sc.cap + 255) / 256;
    const dim3 grid((uint32_t)(blocksWanted < 4096 ? blocksWanted : 4096)), block(256);
#define MRIRT_C5E(L, SH) hipLaunchKernelGGL((c5_emit_kernel<STRICT, L, SH>), grid, block, 0, s, a, e, sc.rowOwner, counter)
    switch (layout) {
        case MRIRT_LAYOUT_LINEAR: if (shade) MRIRT_C5E(0, true); else MRIRT_C5E(0, false); break;
        case MRIRT_LAYOUT_BRICK:  if (shade) MRIRT_C5E(1, true); else MRIRT_C5E(1, false); break;
        case MRIRT_LAYOUT_VG:     if (shade) MRIRT_C5E(2, true); else MRIRT_C5E(2, false); break;
        case MRIRT_LAYOUT_MOD4:   MRIRT_C5E(MRIRT_LAYOUT_MOD4, false); break;
        default:                  MRIRT_C5E(3, false); break;
    }
#undef MRIRT_C5E
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

template <bool STRICT>
static int c5_launch_composite(const K1Args& a, bool shade, const C5Scratch& sc, uint32_t* nextCounter, uint32_t chunk, hipStream_t s) {
    const dim3 grid(a.map.chunk * kXcds), block(a.map.blockPx == 8 ? 64 : 256);     // the plan kernel's pixel -> lane map
    if (shade) hipLaunchKernelGGL((c5_composite_kernel<STRICT, true>), grid, block, 0, s, a, sc.rays, sc.geom, sc.classes, sc.mix, sc.seg, sc.rowOwner, nextCounter, chunk);
    else       hipLaunchKernelGGL((c5_composite_kernel<STRICT, false>), grid, block, 0, s, a, sc.rays, sc.geom, sc.classes, sc.mix, sc.seg, sc.rowOwner, nextCounter, chunk);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

}  // namespace mrirt

extern "C" int64_t mrirt_brats_inr_scratch_bytes(const MrirtBratsParams* p, uint32_t chunk_steps) {
    C5Scratch sc;
    return c5_carve(p, chunk_steps, nullptr, sc) == MRIRT_OK ? sc.bytes : 0;
}

namespace mrirt {

// what both chunked entry points refuse of their common arguments before they look at their network
int c5_check_common(const MrirtRenderExt* ext, const void* const vol[4], const float* zmu, const float* zsigma, const void* scratch,
                    const void* out_rgba) {
    if (!out_rgba || !scratch || !vol || !zmu || !zsigma) return MRIRT_ERR_NULL;
    const bool mod4 = ext && ext->layout == MRIRT_LAYOUT_MOD4;
    for (int m = 0; m < (mod4 ? 1 : 4); ++m) if (!vol[m]) return MRIRT_ERR_NULL;     // the MLP reads all four modalities
    if (ext && ext->tileSize != 0) return MRIRT_ERR_ARG;                      // whole-frame only
    return MRIRT_OK;
}

// The frame loop of the chunked C5 render (declared in brats_host.h)
int c5_frame(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4], const void* labels, const float zmu[4],
             const float zsigma[4], uint32_t chunk_steps, void* scratch, int64_t scratch_bytes, void* out_rgba, int64_t pitch_px,
             uint64_t* stats_dev, void* stream, int64_t maxCap, C5Classify classify, const void* ctx) {
    K1Args a;
    Prepared cfg;
    int rc = prepare(p, ext, vol, labels, nullptr, true, pitch_px, a, cfg);
    if (rc != MRIRT_OK) return rc;
    if (a.labCell != nullptr) return MRIRT_ERR_LAYOUT;           // the C5 passes read the ground-truth grid themselves (LINEAR / BRICK)
    if (!c5_layout_ok(cfg.layout, cfg.shade)) return MRIRT_ERR_LAYOUT;       // refused before anything touches the scratch
    if (p->showPred == 0) return MRIRT_ERR_ARG;
    C5Scratch sc;
    rc = c5_carve(p, chunk_steps, scratch, sc);
    if (rc != MRIRT_OK) return rc;
    if (scratch_bytes < sc.bytes) return MRIRT_ERR_ARG;
    if (sc.cap > maxCap) return MRIRT_ERR_ARG;
    // passes: a ray's chord is at most the box diagonal; the march counts it with the running fp32 sum t += stepSize, whose
    // increments are each off by up to half an ulp of t — a relative drift of up to ulp(tFar) / (2 stepSize) over the chord
    // when stepSize is only a few tens of ulps of t.  The bound carries twice that drift (tFar = the farthest any
    // sample can be, as in prepare()), so that no ray is still marching when the last pass has been composited.
    double diag2 = 0.0, dist2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double e = (double)p->voxelSize[k] * (double)p->dims[k];
        const double c = (double)p->volMin[k] + 0.5 * e - (double)p->eye[k];
        diag2 += e * e; dist2 += c * c;
    }
    double tFar = sqrt(dist2) + sqrt(diag2);
    if (ext && ext->cameraMode == 1u) tFar += fabs((double)ext->orthoHalfHeight) * (1.0 + (double)p->imageSize[0] / fmax(1.0, (double)p->imageSize[1]));
    const double ulpFar = (double)(nextafterf((float)tFar, INFINITY) - (float)tFar);
    const double drift = 1.0 + ulpFar / (double)p->stepSize;
    const uint64_t maxSteps = (uint64_t)(sqrt(diag2) / (double)p->stepSize * drift) + 3;
    const uint64_t passes = (maxSteps + chunk_steps - 1) / chunk_steps;
    if (passes > kC5MaxPasses) return MRIRT_ERR_ARG;
    EmitArgs e;
    for (int m = 0; m < 4; ++m) { e.zmu[m] = zmu[m]; e.zsigma[m] = make_udiv(zsigma[m]); }
    for (int k = 0; k < 3; ++k) { e.dimM1[k] = (double)(p->dims[k] - 1); e.rdimM1[k] = 1.0 / e.dimM1[k]; }
    e.offsets = nullptr; e.coords = sc.coords; e.feats = reinterpret_cast<float4*>(sc.feats); e.mix = sc.mix; e.seg = sc.seg; e.geom = sc.geom;
    a.out = out_rgba;
    a.stats = stats_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    MRIRT_HIP(hipMemsetAsync(sc.counters, 0, (size_t)kC5MaxPasses * 8, s));
    const bool strict = cfg.math == MRIRT_MATH_STRICT;
    for (uint32_t c = 0; c < (uint32_t)passes; ++c) {
        rc = strict ? c5_launch_plan<true>(a, e, cfg.layout, cfg.shade, sc, c, chunk_steps, s)
                    : c5_launch_plan<false>(a, e, cfg.layout, cfg.shade, sc, c, chunk_steps, s);
        if (rc != MRIRT_OK) return rc;
        rc = classify(sc, c, s, ctx);
        if (rc != MRIRT_OK) return rc;
        uint32_t* next = c + 1 < (uint32_t)passes ? sc.counters + c + 1 : nullptr;
        rc = strict ? c5_launch_composite<true>(a, cfg.shade, sc, next, chunk_steps, s)
                    : c5_launch_composite<false>(a, cfg.shade, sc, next, chunk_steps, s);
        if (rc != MRIRT_OK) return rc;
    }
    if (stats_dev != nullptr) {                                               // stats_dev[2] += MLP queries of the frame
        hipLaunchKernelGGL(c5_sum_kernel, dim3(1), dim3(64), 0, s, sc.counters, (uint32_t)passes, stats_dev + 2);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}

}  // namespace mrirt

static int c5_classify_mlp(const C5Scratch& sc, uint32_t c, hipStream_t s, const void* ctx) {
    return inr_forward_dev_n(static_cast<const MrirtInrDesc*>(ctx), sc.coords, sc.feats, sc.cap, sc.counters + c, sc.classes,
                             sc.counters + kC5MaxPasses + c, s);
}

extern "C" int mrirt_render_brats_inr(const MrirtBratsParams* p, const MrirtRenderExt* ext, const void* const vol[4],
                                      const void* labels, const MrirtInrDesc* net, const float zmu[4], const float zsigma[4],
                                      uint32_t chunk_steps, void* scratch, int64_t scratch_bytes,
                                      void* out_rgba, int64_t pitch_px, uint64_t* stats_dev, void* stream) {
    if (!net) return MRIRT_ERR_NULL;
    int rc = c5_check_common(ext, vol, zmu, zsigma, scratch, out_rgba);
    if (rc != MRIRT_OK) return rc;
    if ((net->kind != MRIRT_INR_FOURIER_RELU && net->kind != MRIRT_INR_SIREN) || net->numMods != 4) return MRIRT_ERR_ARG;
    // what inr_forward_dev_n would refuse in the first pass, after the plan and the emission had written the scratch
    if (mrirt_inr_pack_bytes(net) <= 0) return MRIRT_ERR_ARG;
    if (!net->weights || !net->biases) return MRIRT_ERR_NULL;
    return c5_frame(p, ext, vol, labels, zmu, zsigma, chunk_steps, scratch, scratch_bytes, out_rgba, pitch_px, stats_dev, stream, INT64_MAX,
                    c5_classify_mlp, net);
}
