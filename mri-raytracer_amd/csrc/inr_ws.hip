// INR forward, the weight-stationary kernel for the 4 x 256 SIREN (formulation and precision: inr_mlp.hip).
#include "inr_fwd.h"

namespace mrirt {

// =====================================================================================================
// Weight-stationary kernel for BASELINE config 5's network: the 4 x 256 SIREN on (coords, 4 modalities),
// 7 -> 256 -> 256 -> 256 -> 256 -> (<= 4 classes)   (notebooks/neumors_inr.ipynb:853-899,1165-1178).
//
// Why a second dataflow.  Measured on the streaming kernel (inr_stream.hip; knock-out builds since removed, their results
// are profiles/r02_inr_knockouts.txt and r02_inr_knockouts_streaming_kernel.txt): with the
// weight LDS-DMA compiled out it runs 24.7 -> 18.8 ms, with the input staging compiled out 24.7 -> 20.1 ms.  A SIMD
// has 32 issue cycles per MFMA; the stream spends ~12 of them per MFMA on DMA pieces (416 KiB of weights pass
// through LDS for every 256 points, and the point count per CU is capped by the register file that holds the
// activations).  Here the roles are swapped: the WEIGHTS live in the register file for the whole launch — a
// CU's four SIMDs hold 4 x 128 KiB of registers, the network is 416 KiB — and the ACTIVATIONS travel through
// LDS.  One wave per SIMD (512 registers); wave w owns out tiles 2w and 2w+1 of the three hidden layers (384 registers
// of A fragments: layers 1 and 2 in the AGPR half through "a"-constrained MFMAs, layer 3 in VGPRs, its last four
// fragments and the small layer-0 / head fragments in LDS); a round is G = 3 groups of 32 points; per layer a wave reads
// a group's sixteen 1-KiB B fragments from LDS (what all four waves wrote in the previous phase), runs its
// 2 x 16 MFMAs, and writes its two out tiles back as the next layer's B fragments 4w .. 4w+3 (the accumulator
// layout IS the B layout, as above: two ds_write_b128 per tile).  The head is one out tile: wave g (g < G) runs it
// for group g, one round late, interleaved with the next round's layer 0 (which is VALU-bound: two MFMAs and sixteen
// sines per tile pass, while the head is sixteen MFMAs and no activation).  No weight traffic at all after the
// prologue, one workgroup barrier per phase (four per round).
// Tried and measured no faster (round 2, s_memtime stamps + wall): a second schedule that chains the passes across phase
// and round boundaries with two write-only barriers per phase (post-op always under the next pass, ring running on
// into the next layer) — 20.0 k cycles per round against 18.1 k here; a micro-benchmark of the pass (tools/micro/
// mfma_pace.hip) shows why neither wins: 16 MFMAs + 16 LDS reads take 549 cycles, and the 16 v_sin + 8 converts of the
// previous tile's activation add ~160 on top instead of hiding (709) — with one wave per SIMD the VALU work of the gaps
// that carry two sines overflows the 24 issue cycles an MFMA leaves.
// Same packed image, same arithmetic per point (accumulator starts at the bias, k steps in ascending order):
// bit-identical logits to the streaming kernel (tools/ws_check.py; the tests hold both kernels to the same fp32 /
// fp64 references, and each is batch-position invariant by construction).
// =====================================================================================================
constexpr int kWsGroups = 3;
// Diagnostic build (-DMRIRT_WS_STAMPS): s_memtime at the phase boundaries of one steady-state round of every
// workgroup goes to the logits buffer (which then holds no logits): [block][wave][24] uint64.  Never in the product.
#ifdef MRIRT_WS_STAMPS
#define WS_STAMP(k) do { if (stampRound && lane == 0) stamps[((size_t)blockIdx.x * 4 + w) * 24 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define WS_STAMP(k) do { } while (0)
#endif

// MFMA with the operand register class spelled out.  hipcc's allocator fills the 256 arch VGPRs with weights first
// and then shuttles everything VALU touches through v_accvgpr moves (measured: 220 VGPRs of weights, 520
// v_accvgpr_read per round, 21 fragments spilled to scratch and reloaded every round).  An "a" constraint pins a
// fragment into the accumulation half of the unified file — which VALU cannot use anyway — and leaves the arch
// half to the accumulators, the B ring and the activation.  The compiler does not know these are matrix
// instructions, so the MFMA -> VALU read hazard is kept by construction (see the call sites) or by mfma_drain(acc).
__device__ __forceinline__ void mfma_a(f32x16& acc, const bf16x8& wa, const bf16x8& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(wa), "v"(b));
}
__device__ __forceinline__ void mfma_v(f32x16& acc, const bf16x8& wv, const bf16x8& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(wv), "v"(b));
}
// after the last MFMA of a chain whose result VALU reads next: 8 passes + 3 wait states, taken generously
// (the accumulator is an in/out operand so that no read of it can be scheduled above the wait)
__device__ __forceinline__ void mfma_drain(f32x16& acc) { asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc)); }

template <bool SIREN>
__global__ __launch_bounds__(256, 1) void inr_ws_kernel(const InrArgs a) {
    constexpr int G = kWsGroups, NH = 3, KS = 16, RD = 4;                // RD: B fragments in flight ahead of their MFMA
    constexpr int kActQ = G * 2 * KS * 64;               // uint4: [group][parity][k step][lane]    96 KiB
    constexpr int kInQ = G * 2 * 64;                     // layer-0 B fragments (k steps 0, 1)       6 KiB
    constexpr int kBiasQ = (4 * 256 + 32) / 4;           // padded biases                          4.1 KiB
    constexpr int kW0Q = 16 * 64, kWoQ = 16 * 64;        // layer-0 and head A fragments (all waves')   16 + 16 KiB
    constexpr int kW3Q = 4 * 4 * 64;                     // four layer-3 A fragments per wave that do not fit the registers  16 KiB
    constexpr int kW0Off = kActQ + kInQ + kBiasQ, kWoOff = kW0Off + kW0Q, kW3Off = kWoOff + kWoQ;
    __shared__ uint4 ldsAll[kActQ + kInQ + kBiasQ + kW0Q + kWoQ + kW3Q];

    const int64_t nPts = inr_point_count(a);
    if (nPts <= 0) return;
    const float tieThr = a.tie != nullptr ? a.tie[0] * a.tieScale : 0.0f;

    const uint32_t lane = threadIdx.x & 63u, r = lane & 31u, h = lane >> 5;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    inr_stage_biases(a, ldsAll + kActQ + kInQ);
    // ---- the network, resident in this wave's registers --------------------------------------------------
    const uint4* __restrict__ wp = a.wpack;
    bf16x8 Wh[NH][2][KS];                                 // 384 registers: the three hidden matrices' out tiles 2w, 2w+1
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 fr = wp[(size_t)(a.L.fragOff[l + 1] + (2 * w + j) * KS + ks) * 64 + lane];
                // 96 fragments = 384 registers is what fits beside the accumulators: the last four of layer 3 go through LDS
                if (l == NH - 1 && j == 1 && ks >= KS - 4) ldsAll[kW3Off + (w * 4 + (ks - (KS - 4))) * 64 + lane] = fr;
                else Wh[l][j][ks] = __builtin_bit_cast(bf16x8, fr);
            }
    // layer 0 (2 k steps per out tile) and the head (k-quarter per wave) are 4 + 4 fragments per wave: they stay in
    // LDS (lane-linear, read just before use) — 400 + of the 512 registers as weights left the allocator no room
    for (uint32_t f = w; f < 16; f += 4) {
        ldsAll[kW0Off + f * 64 + lane] = wp[(size_t)(a.L.fragOff[0] + f) * 64 + lane];          // [tile o][s] = fragment 2o + s
        ldsAll[kWoOff + f * 64 + lane] = wp[(size_t)(a.L.fragOff[NH + 1] + f) * 64 + lane];     // head k step f
    }
    // LDS addressing: a handful of per-lane base pointers (re-laundered every round so that the compiler cannot
    // expand them into one hoisted VGPR per fragment address and spill) + compile-time immediates (<= 64 KiB each).
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));       // plain vector types: HIP's uint4 / float4 classes
    typedef float f32x4 __attribute__((ext_vector_type(4)));          // cannot be assigned through an LDS-qualified pointer
    typedef __attribute__((address_space(3))) u32x4 lds_q;
    typedef __attribute__((address_space(3))) f32x4 lds_f4;
    lds_q* bR = (lds_q*)ldsAll + lane;                               // B-fragment reads: fragment f at bR[64 f]
    lds_q* bW = (lds_q*)ldsAll + 4 * w * 64 + lane;                  // this wave's output fragments 4w .. 4w+3
    lds_q* bIn = (lds_q*)ldsAll + kActQ + lane;                      // layer-0 B fragments
    lds_f4* bBias = (lds_f4*)((lds_q*)ldsAll + kActQ + kInQ) + 16 * w + h;               // tile 2w, rows 4h..
    lds_q* bWt = (lds_q*)ldsAll + kW0Off + 4 * w * 64 + lane;        // this wave's layer-0 fragments 4w..4w+3; head: + kW0Q;
                                                                     // its four LDS-held layer-3 fragments: + kW0Q + kWoQ
    auto launder = [&]() {
        uint32_t v0 = (uint32_t)(uintptr_t)bR, v1 = (uint32_t)(uintptr_t)bW, v2 = (uint32_t)(uintptr_t)bIn,
                 v4 = (uint32_t)(uintptr_t)bBias, v5 = (uint32_t)(uintptr_t)bWt;
        asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v4), "+v"(v5));
        bWt = (lds_q*)(uintptr_t)v5;
        bR = (lds_q*)(uintptr_t)v0; bW = (lds_q*)(uintptr_t)v1; bIn = (lds_q*)(uintptr_t)v2;
        bBias = (lds_f4*)(uintptr_t)v4;
    };
    // biases of this specialised network sit at layer l -> 256 l (head: 1024): compile-time immediates
    auto bias_tile = [&](int l, int j) {                                 // tile 2w + j: rows 8g + 4h .. +3 (g = 0..3)
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 b = bBias[(256 * l + 32 * j + 8 * g) >> 2];
            acc[4 * g + 0] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
        }
        return acc;
    };
    auto rd_frag = [&](int g, int par, int ks) { return __builtin_bit_cast(bf16x8, bR[((g * 2 + par) * KS + ks) * 64]); };
    auto wr_frag = [&](int g, int par, int j, int s2, const bf16x8& v) { bW[((g * 2 + par) * KS + 2 * j + s2) * 64] = __builtin_bit_cast(u32x4, v); };

    // raw inputs of point `pidx` -> the two layer-0 B fragments of the augmented split (see make_layout):
    //   k step 0 = [x_hi(0..6), x_lo(0..6), 0, 0],  k step 1 = [x_hi(0..6), 0 ...]; element j of lane half h is slot 8(j>>2) + 4h + (j&3)
    float rawc[3];
    float4 rawf;
    auto load_raw = [&](int64_t pidx) {
        const int64_t p = pidx < nPts ? pidx : nPts - 1;
        rawc[0] = a.coords[p * 3 + 0]; rawc[1] = a.coords[p * 3 + 1]; rawc[2] = a.coords[p * 3 + 2];
        rawf = reinterpret_cast<const float4*>(a.feats)[p];
    };
    auto stage_raw = [&](int g) {
        const float x[7] = { rawc[0], rawc[1], rawc[2], rawf.x, rawf.y, rawf.z, rawf.w };
        __bf16 hi[8], lo[8];
#pragma unroll
        for (int k = 0; k < 7; ++k) { hi[k] = (__bf16)x[k]; lo[k] = (__bf16)(x[k] - (float)hi[k]); }
        hi[7] = (__bf16)0.0f; lo[7] = (__bf16)0.0f;
        const __bf16 z = (__bf16)0.0f;
        bf16x8 f0, f1;
        // lane half 0: slots 0..3, 8..11        lane half 1: slots 4..7, 12..15
        const bf16x8 f0a = { hi[0], hi[1], hi[2], hi[3], lo[1], lo[2], lo[3], lo[4] };
        const bf16x8 f0b = { hi[4], hi[5], hi[6], lo[0], lo[5], lo[6], z, z };
        const bf16x8 f1a = { hi[0], hi[1], hi[2], hi[3], z, z, z, z };
        const bf16x8 f1b = { hi[4], hi[5], hi[6], z, z, z, z, z };
        f0 = h ? f0b : f0a;
        f1 = h ? f1b : f1a;
        lds_q* dst = (lds_q*)ldsAll + kActQ + g * 2 * 64 + lane;      // g = this wave's id: runtime, once per round
        dst[0] = __builtin_bit_cast(u32x4, f0);
        dst[64] = __builtin_bit_cast(u32x4, f1);
    };

    // one value of a finished accumulator per call: activation, and every second value the packed bf16 convert
    auto act_one = [&](f32x16& ap, bf16x8 (&Ho)[2], int i) {
        if constexpr (SIREN) ap[i] = __builtin_amdgcn_sinf(ap[i]);
        if (i & 1) {
            f32x2 x = { ap[i - 1], ap[i] };
            if constexpr (!SIREN) x = __builtin_elementwise_max(x, (f32x2){ 0.0f, 0.0f });
            Ho[i >> 3][(i & 7) - 1] = (__bf16)x.x;
            Ho[i >> 3][i & 7] = (__bf16)x.y;
        }
    };

    // The same in two sweeps, for the places where no MFMA stream separates a sine from the convert that reads it (layer 0's passes,
    // the last hidden layer's tail): sixteen independent transcendentals first, then the eight packed converts — a convert right
    // behind its sines waits out the transcendental's latency, and with one wave per SIMD nothing else can issue meanwhile
    // (s_memtime stamps: ~70 cycles per pass).
    auto sin_one = [&](f32x16& ap, int i) {
        if constexpr (SIREN) ap[i] = __builtin_amdgcn_sinf(ap[i]);
    };
    auto cvt_all = [&](f32x16& ap, bf16x8 (&Ho)[2]) {
#pragma unroll
        for (int i = 1; i < 16; i += 2) {
            f32x2 x = { ap[i - 1], ap[i] };
            if constexpr (!SIREN) x = __builtin_elementwise_max(x, (f32x2){ 0.0f, 0.0f });
            Ho[i >> 3][(i & 7) - 1] = (__bf16)x.x;
            Ho[i >> 3][i & 7] = (__bf16)x.y;
        }
    };

    // The head's epilogue: the drained accumulator of round rnd's group w -> logits, argmax and near-tie mark
    auto head_store = [&](const f32x16& acc, int64_t rnd) {
        const int64_t pidx = (rnd * G + w) * 32 + r;
        if (h == 0 && pidx < nPts) {                                      // classes 0..3 are rows 0..3: lane half 0, registers 0..3
            const float v[4] = { acc[0], acc[1], acc[2], acc[3] };
#ifndef MRIRT_WS_STAMPS
            if (a.logits != nullptr)
                for (uint32_t c = 0; c < a.L.outDim; ++c) a.logits[pidx * a.L.outDim + c] = v[c];
#endif
            if (a.argmax != nullptr) {
                float best = -INFINITY, second = -INFINITY;
                uint32_t bestc = 0;
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) top2_push(c < a.L.outDim ? v[c] : -INFINITY, c, best, second, bestc);   // strict: the first maximum
                const bool tie = a.tie != nullptr && !(best - second >= tieThr);     // near-tie mark (kFlagBit)
                a.argmax[pidx] = (int16_t)(bestc | (tie ? (uint32_t)kFlagBit : 0u));
            }
        }
    };

    // Head (linear, <= 4 classes): one out tile, so one wave per group — wave g reads group g's last hidden outputs
    // (parity NH & 1 ^ 1 ... written by all four waves before the barrier that precedes this) and the sixteen head
    // fragments from LDS, and stores logits / argmax.  np.argmax = first maximum.
    auto head = [&](int64_t rnd) {
        constexpr int par = (NH & 1) ^ 1;
        f32x16 acc;
        {
            const f32x4 hb = *((lds_f4*)((lds_q*)ldsAll + kActQ + kInQ) + (1024 >> 2) + h);   // rows 4h..4h+3 of the head's bias
            acc = (f32x16)(0.0f);
            acc[0] = hb.x; acc[1] = hb.y; acc[2] = hb.z; acc[3] = hb.w;
        }
        lds_q* bH = (lds_q*)ldsAll + (w * 2 + par) * KS * 64 + lane;
        lds_q* bWo = (lds_q*)ldsAll + kWoOff + lane;
        asm volatile("s_nop 3" : "+v"(acc));                             // VALU wrote acc (v_mov): two wait states before an MFMA reads it as C
        bf16x8 ra[4], rb[4];                                              // four k steps of operands in flight
#pragma unroll
        for (int d = 0; d < 4; ++d) { ra[d] = __builtin_bit_cast(bf16x8, bWo[d * 64]); rb[d] = __builtin_bit_cast(bf16x8, bH[d * 64]); }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            mfma_v(acc, ra[ks % 4], rb[ks % 4]);
            if (ks + 4 < KS) { ra[ks % 4] = __builtin_bit_cast(bf16x8, bWo[(ks + 4) * 64]); rb[ks % 4] = __builtin_bit_cast(bf16x8, bH[(ks + 4) * 64]); }
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_drain(acc);
        head_store(acc, rnd);
    };

    const int64_t nRounds = (nPts + G * 32 - 1) / (G * 32);
    int64_t round = blockIdx.x;
    if (w < G) {                                           // wave w stages (and later reduces) group w
        load_raw((round * G + w) * 32 + r);
        stage_raw((int)w);
    }
    __syncthreads();                                       // biases + first inputs are in LDS
    int64_t prevRound = -1;

    for (; round < nRounds; round += gridDim.x) {
        const int64_t nextRound = round + gridDim.x;
        launder();
#ifdef MRIRT_WS_STAMPS
        uint64_t* stamps = reinterpret_cast<uint64_t*>(a.logits);
        const bool stampRound = stamps != nullptr && round == (int64_t)blockIdx.x + 3 * (int64_t)gridDim.x;
#endif
        WS_STAMP(0);
        // ---- layer 0 of this round + head of the previous one, interleaved ------------------------------------
        // Layer 0 is VALU-bound (2 MFMAs but 16 sines per tile pass), the head is MFMA-bound (16 MFMAs, no activation),
        // and run one after the other they cost a sixth of a round (profiles/r02_inr_ws_knockouts.txt).  Here pass
        // i's activation is sliced under pass i+1's MFMAs and two or three head MFMAs (waves 0..G-1: wave g takes
        // group g of the PREVIOUS round, sixteen k steps over the last hidden layer's outputs) per pass.
        f32x16 carry;                                      // a phase's last accumulator, activated under the next phase's pass 0
        // The head's epilogue (the previous round's logits -> stores, argmax, near-tie mark): ~70 VALU instructions, ~560 cycles on
        // waves 0 .. G-1 at the end of the layer-0 phase (s_memtime stamps).  Moving it behind the barrier, under hidden layer 1's
        // first LDS reads, moves the same 560 cycles there (measured: cycles per round level, wall time +0.3 %): it stays here.
        f32x16 headAcc;
        const bool headPending = prevRound >= 0 && w < G;
        auto head_epilogue = [&]() {
            if (!headPending) return;
            mfma_drain(headAcc);
            head_store(headAcc, prevRound);
        };
        auto l0_head = [&](auto headC) {
            constexpr bool HEAD = decltype(headC)::value;
            constexpr int hpar = (NH & 1) ^ 1;                // parity the last hidden layer wrote
            lds_q* bH = (lds_q*)ldsAll + (w * 2 + hpar) * KS * 64 + lane;
            lds_q* bWo = (lds_q*)ldsAll + kWoOff + lane;
            f32x16 hacc;
            bf16x8 ra[2], rb[2];                               // head operands, two k steps ahead
            if constexpr (HEAD) {
                const f32x4 hb = *((lds_f4*)((lds_q*)ldsAll + kActQ + kInQ) + (1024 >> 2) + h);   // rows 4h..4h+3 of the head's bias
                hacc = (f32x16)(0.0f);
                hacc[0] = hb.x; hacc[1] = hb.y; hacc[2] = hb.z; hacc[3] = hb.w;
#pragma unroll
                for (int d = 0; d < 2; ++d) { ra[d] = __builtin_bit_cast(bf16x8, bWo[d * 64]); rb[d] = __builtin_bit_cast(bf16x8, bH[d * 64]); }
                asm volatile("s_nop 3" : "+v"(hacc));          // VALU wrote hacc (v_mov): wait states before an MFMA reads it as C
            }
            int hk = 0;                                        // head k step (a compile-time value in the unrolled code)
            auto head_step = [&]() {
                if constexpr (HEAD) {
                    if (hk < KS) {
                        mfma_v(hacc, ra[hk % 2], rb[hk % 2]);
                        if (hk + 2 < KS) { ra[hk % 2] = __builtin_bit_cast(bf16x8, bWo[(hk + 2) * 64]); rb[hk % 2] = __builtin_bit_cast(bf16x8, bH[(hk + 2) * 64]); }
                        ++hk;
                    }
                }
            };
            constexpr int NP = 2 * G;
            f32x16 acc = bias_tile(0, 0), accPrev, accNext;
            bf16x8 Ho[2];
            // the four layer-0 A fragments of this wave's two tiles are read ONCE per phase, the input fragments one group ahead:
            // read pass by pass right in front of their MFMAs, every pass exposed an LDS round trip (round 2's stamps: 3.6 k
            // cycles for a phase whose MFMA + VALU work is ~2 k).
            bf16x8 wa[4], Bin[2], BinNext[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) wa[q] = __builtin_bit_cast(bf16x8, bWt[q * 64]);
            Bin[0] = __builtin_bit_cast(bf16x8, bIn[0]); Bin[1] = __builtin_bit_cast(bf16x8, bIn[64]);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int g = i >> 1, j = i & 1;
                WS_STAMP(15 + i);
                if (j == 0 && g + 1 < G) { BinNext[0] = __builtin_bit_cast(bf16x8, bIn[((g + 1) * 2 + 0) * 64]); BinNext[1] = __builtin_bit_cast(bf16x8, bIn[((g + 1) * 2 + 1) * 64]); }
                mfma_v(acc, wa[2 * j + 0], Bin[0]);
                mfma_v(acc, wa[2 * j + 1], Bin[1]);
                if (j == 1) { Bin[0] = BinNext[0]; Bin[1] = BinNext[1]; }
                __builtin_amdgcn_sched_barrier(0);
                if (i + 1 < NP) accNext = bias_tile(0, (i + 1) & 1);
                if (i > 0) {
                    const int pg = (i - 1) >> 1, pj = (i - 1) & 1;
                    asm volatile("s_nop 15" : "+v"(accPrev));   // two MFMA issues + 16 states since accPrev's producer
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        sin_one(accPrev, v);
                        if (v == 3 || v == 9 || (v == 14 && i < 5)) { head_step(); __builtin_amdgcn_sched_barrier(0); }
                    }
                    cvt_all(accPrev, Ho);
                    wr_frag(pg, 1, pj, 0, Ho[0]);
                    wr_frag(pg, 1, pj, 1, Ho[1]);
                } else {
                    head_step(); head_step(); head_step();
                }
                __builtin_amdgcn_sched_barrier(0);
                accPrev = acc;
                if (i + 1 < NP) acc = accNext;
            }
            // the last pass's activation is carried into hidden layer 1's pass 0 (see `carry` below); what is left of the head:
            WS_STAMP(21);
            head_step();
            carry = accPrev;
            if constexpr (HEAD) {
                while (hk < KS) head_step();                   // (none left with G = 3: 3 + 3*4 ... counted at compile time)
                headAcc = hacc;
                head_epilogue();
            }
        };
        if (prevRound >= 0 && w < G) l0_head(IC<1>{}); else l0_head(IC<0>{});
        WS_STAMP(1);
        __syncthreads();
        WS_STAMP(2);
        // ---- hidden layers: layer l reads parity (l & 1), writes the other; the last one feeds the head ---------
        // The last pass of a layer has no MFMAs of its own layer left to hide its activation under: as a tail after the loop it
        // cost 476 cycles per layer (s_memtime stamps, profiles/r04_inr_ws/).  Layers 0, 1 and 2 therefore hand their last
        // accumulator to the NEXT layer (`carry`), whose pass 0 — which had nothing to cover — activates it and writes it into the
        // buffer that layer reads (group G - 1, tile 1).  Group G - 1 is first read by the B-fragment ring's look-ahead, RD steps before
        // pass 2 (G - 1), i.e. late in pass 2 (G - 1) - 1: one more barrier at the START of that pass orders the carried writes
        // (made three passes earlier); groups 0 .. G - 2 were complete at the layer-boundary barrier as before.
        auto hidden = [&](auto lC) {
            constexpr int l = decltype(lC)::value;            // 1 .. NH
            constexpr int par = l & 1;
            constexpr int NP = 2 * G;                          // tile passes: (group g, tile j) = (i >> 1, i & 1)
            constexpr bool CARRY_IN = true, CARRY_OUT = l < NH;      // layer 1 takes layer 0's last pass
            bf16x8 ring[RD];
#pragma unroll
            for (int d = 0; d < RD; ++d) ring[d] = rd_frag(0, par, d);
            f32x16 accPrev;
            if constexpr (CARRY_IN) accPrev = carry;
            bf16x8 Ho[2];                                      // packed outputs of the previous pass
            bf16x8 w3[4];                                      // layer 3: the LDS-held A fragments of tile 1, k steps 12..15
            f32x16 acc = bias_tile(l, 0);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int j = i & 1;
                f32x16 accNext;
                if constexpr (l == 1) WS_STAMP(8 + i);
                static_assert(RD <= KS, "the ring's look-ahead reaches group G - 1 no earlier than pass 2 (G - 1) - 1");
                if (CARRY_IN && i == 2 * (G - 1) - 1) __syncthreads();   // the previous layer's carried unit is in LDS on every wave
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int q = i * KS + ks;                 // position in the phase's B-fragment stream
                    if constexpr (l <= 2) mfma_a(acc, Wh[l - 1][j][ks], ring[q % RD]);             // layers 1, 2: the 256 AGPRs
                    else if (j == 1 && ks >= KS - 4) mfma_v(acc, w3[ks - (KS - 4)], ring[q % RD]);  // layer 3's four LDS-held fragments
                    else mfma_v(acc, Wh[l - 1][j][ks], ring[q % RD]);                               // layer 3: arch VGPRs
                    if (q + RD < NP * KS) ring[q % RD] = rd_frag((q + RD) / KS >> 1, par, (q + RD) % KS);
                    if constexpr (l == NH) { if (j == 1 && ks >= KS - 7 && ks < KS - 3) w3[ks - (KS - 7)] = __builtin_bit_cast(bf16x8, bWt[kW0Q + kWoQ + (ks - (KS - 7)) * 64]); }
                    if (i > 0 || CARRY_IN) {
                        // the previous pass's accumulator (pass 0: the previous LAYER's last one), ONE value per step (two in steps 2
                        // and 3): a v_sin next to an MFMA costs ~16 issue cycles, two of them overflow the 24 an MFMA leaves
                        // (tools/micro/mfma_pace.hip).  The compiler does not know the asm statements are MFMAs, so the XDL-write ->
                        // VALU-read wait is kept by hand: two MFMA issues, two LDS issues and 4 idle states.
                        // Where it goes: this layer's output buffer (par ^ 1) — the carried unit into the buffer this layer READS (par).
                        const int pg = i > 0 ? (i - 1) >> 1 : G - 1, pj = i > 0 ? (i - 1) & 1 : 1, wpar = i > 0 ? (par ^ 1) : par;
                        if (ks == 1) asm volatile("s_nop 3" : "+v"(accPrev));
                        if (ks == 2) { act_one(accPrev, Ho, 0); act_one(accPrev, Ho, 1); }
                        if (ks == 3) { act_one(accPrev, Ho, 2); act_one(accPrev, Ho, 3); }
                        if (ks >= 4) act_one(accPrev, Ho, ks);
                        if (ks == 8) wr_frag(pg, wpar, pj, 0, Ho[0]);
                        if (ks == 15) wr_frag(pg, wpar, pj, 1, Ho[1]);
                    }
                    if (ks == 11 && i + 1 < NP) accNext = bias_tile(l, (i + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                accPrev = acc;
                if (i + 1 < NP) acc = accNext;
            }
            if constexpr (l == 1) WS_STAMP(8 + NP);
            if constexpr (CARRY_OUT) {
                carry = accPrev;                               // activated under the next layer's pass 0
            } else {
                // the last hidden layer's last pass: the head reads it in the next phase
                mfma_drain(accPrev);
#pragma unroll
                for (int v = 0; v < 16; ++v) sin_one(accPrev, v);
                cvt_all(accPrev, Ho);
                wr_frag(G - 1, par ^ 1, 1, 0, Ho[0]);
                wr_frag(G - 1, par ^ 1, 1, 1, Ho[1]);
            }
        };
        hidden(IC<1>{});
        WS_STAMP(3);
        __syncthreads();
        hidden(IC<2>{});
        WS_STAMP(4);
        __syncthreads();
        WS_STAMP(5);
        if (nextRound < nRounds && w < G) load_raw((nextRound * G + w) * 32 + r);      // in flight under the last hidden phase
        hidden(IC<3>{});
        WS_STAMP(6);
        if (nextRound < nRounds && w < G) stage_raw((int)w);                          // ldsIn was last read before two barriers
        __syncthreads();
        WS_STAMP(7);
        prevRound = round;
    }
    // the last round's head
    if (prevRound >= 0 && w < G) head(prevRound);
}

// nets the weight-stationary kernel takes: the 7-input SIREN with four 256-wide layers and <= 4 classes, points mode
bool ws_eligible(const InrArgs& a) {
    return a.kind == MRIRT_INR_SIREN && a.L.aug0 && a.L.hidden == 256 && a.L.numLayers == 5 && a.L.outDim <= 4 &&
           a.M == 4 && !a.volume && (reinterpret_cast<uintptr_t>(a.feats) & 15u) == 0;
}

int launch_inr_ws(const InrArgs& a, hipStream_t s) {
    int dev = 0, cus = 0;
    MRIRT_HIP(hipGetDevice(&dev));
    MRIRT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int64_t rounds = (a.n + kWsGroups * 32 - 1) / (kWsGroups * 32);
    const int64_t nres = cus > 0 ? cus : 256;                  // one workgroup per CU (149 KiB of LDS, 512 registers)
    const dim3 grid((uint32_t)(rounds < nres ? rounds : nres)), block(256);
#ifdef MRIRT_WS_STAMPS
    // the stamps go where the logits would: [block][wave][24] uint64 must fit the n * outDim floats
    if (a.logits != nullptr && (uint64_t)a.n * a.L.outDim * sizeof(float) < (uint64_t)grid.x * 4 * 24 * 8) return MRIRT_ERR_ARG;
#endif
    hipLaunchKernelGGL(inr_ws_kernel<true>, grid, block, 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

}  // namespace mrirt
