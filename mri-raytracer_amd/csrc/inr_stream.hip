// INR forward, the streaming kernel: every network the packed layout accepts (formulation and precision: inr_mlp.hip).
//
// Work split: a workgroup is 8 waves (2 per SIMD: one wave's DMA / LDS waits are covered by the other's
// MFMAs); each wave owns 32 points of a 256-point batch, and the workgroup is PERSISTENT: it walks batches
// round-robin and the weight stream is cyclic (the head chunk stages the next batch's first chunk), so
// launch, bias staging and DMA latency are paid once.  The weights of up to four out tiles (<= 64 KiB) are a
// "chunk": chunks are consecutive in the packed image and are staged one chunk ahead by LDS-DMA
// (global_load_lds, one 1-KiB fragment per wave-instruction into a lane-linear image; double buffer,
// one barrier per chunk; the pieces are dealt through the MFMA stream, right after each tile's bias read),
// then read by all 8 waves with conflict-free ds_read_b128 through a four-deep register ring.  The
// accumulator starts at the bias and the layer scale is folded into the packed weights, so an activation is
// v_sin_f32 (or half a v_pk_max_f32) plus the packed bf16 convert, sliced under the next tile's MFMAs.
// Layer-0 inputs: a per-workgroup LDS table of feature descriptors applied to the wave's staged raw inputs.
#include <atomic>

#include "inr_fwd.h"

namespace mrirt {

constexpr int kResidentFrags = 56;    // RES: the whole packed image (<= 56 KiB) lives in LDS; two workgroups still fit a CU

// RES (small nets: the 4 x 64 network of inr/interactive.ipynb is 36 fragments): the weights are loaded into LDS
// once per workgroup and stay; the batch loop then has no DMA and no barrier at all — with chunks this small the
// per-chunk barrier and the DMA latency behind it were most of a batch's time.
template <int HID, int KT0, bool SIREN, bool AUG = false, bool RES = false>
__global__ __launch_bounds__(512) void inr_forward_kernel(const InrArgs a) {
    constexpr int KT = HID / 32;                         // k tiles of a hidden-wide input == out tiles of a hidden-wide output
    constexpr int OTC = KT < 4 ? KT : 4;                 // out tiles per chunk (one barrier per chunk)
    // The first layer of a SIREN multiplies its inputs by w0 = 30 before a sine, so it runs in split bf16 (hi + lo
    // operands, three products: ~16 mantissa bits).  A ReLU net's first layer sees coordinates, sin / cos
    // features and z-scored intensities and is as tolerant of bf16 as its hidden layers: one product.
    // AUG: the split folded into the k axis (<= 8 inputs; see the packed-image note above).
    constexpr bool SPLIT = SIREN && !AUG;
    constexpr int F0 = KT0 * (SPLIT ? 4 : 2), FH = KT * 2;   // fragments per out tile: layer 0 / other layers
    constexpr int CH0 = OTC * F0, CHH = OTC * FH;        // fragments per chunk
    constexpr int CHMAX = CH0 > CHH ? CH0 : CHH;
    constexpr int PERW = (CHMAX + kInrWaves - 1) / kInrWaves;
    constexpr int RD = 4;                                // A-fragment prefetch distance (ring of registers)
    // DMA pieces of the NEXT chunk are dealt over the first three quarters of this chunk's k steps
    constexpr int SP0 = (OTC * KT0 * 2 * 3 / 4) / PERW > 0 ? (OTC * KT0 * 2 * 3 / 4) / PERW : 1;
    constexpr int SPH = (CHH * 3 / 4) / PERW > 0 ? (CHH * 3 / 4) / PERW : 1;
    constexpr int PPT = (PERW + OTC - 1) / OTC;          // hidden layers: pieces per out tile
    static_assert((PERW - 1) * SP0 < OTC * KT0 * 2 && (PERW - 1) * SPH < CHH, "every DMA piece must get a slot");
    constexpr int kBiasQ = kMaxLayers * 256 / 4;         // every layer's padded biases, as float4
    constexpr int kTabQ = 128;                           // one descriptor per layer-0 input feature
    constexpr int kRawQ = kInrWaves * 32 * kRawStride / 4;   // each wave's 32 points x (3 coords, <= 8 mods, a zero)
    // 2 weight buffers (<= 64 KiB each) + biases + feature table + raw inputs: ONE LDS object (G17)
    constexpr int kWQ = (RES ? kResidentFrags : 2 * CHMAX) * 64;     // weight region, in uint4
    __shared__ uint4 ldsAll[kWQ + kBiasQ + kTabQ + kRawQ];
    uint4 (*lds)[CHMAX * 64] = reinterpret_cast<uint4 (*)[CHMAX * 64]>(ldsAll);
    const float4* ldsBias = reinterpret_cast<const float4*>(ldsAll + kWQ);
    float4* ldsTab = reinterpret_cast<float4*>(ldsAll + kWQ + kBiasQ);
    float* ldsRaw = reinterpret_cast<float*>(ldsAll + kWQ + kBiasQ + kTabQ);
    const int64_t nPts = inr_point_count(a);
    if (nPts <= 0) return;                               // uniform: nothing was staged, no barrier is pending
    const float tieThr = a.tie != nullptr ? a.tie[0] * a.tieScale : 0.0f;
    if (a.kind < 2 && threadIdx.x < 128) ldsTab[threadIdx.x] = inr_feature_entry<AUG>(a, threadIdx.x);
    inr_stage_biases(a, ldsAll + kWQ);

    // lane / r / h are re-derived (opaquely) at the top of every batch: addresses computed from a
    // loop-invariant lane id would be hoisted out of the batch loop and spilled around it
    uint32_t lane = threadIdx.x & 63u, r = lane & 31u, h = lane >> 5;
    const uint32_t wave = threadIdx.x >> 6;
    const uint4* __restrict__ wp = a.wpack;
    const uint32_t waveS = __builtin_amdgcn_readfirstlane(wave);
    constexpr bool siren = SIREN;                        // sin activations (kinds 1, 3) vs ReLU (kinds 0, 2)

    // ---- chunk streaming: LDS-DMA, one 1-KiB fragment per wave-instruction (lane-linear image) -----------
    // piece i of this wave = fragment wave + 8 i of the chunk.  A DMA instruction costs its wave tens of
    // issue cycles, so inside the MFMA streams the pieces are dealt out one every few k steps (the other
    // wave of the SIMD keeps the matrix core busy meanwhile) instead of eight in a row at the chunk's start.
    // The fragment count is a compile-time constant (a chunk that is followed by the short head chunk
    // fetches a full hidden chunk: the packed image carries that much slack, mrirt_inr_pack_bytes), so
    // with 8 | N the piece is unconditional and the MFMA stream stays one basic block.
    auto stage_piece = [&](uint32_t fragStart, auto nfragC, int dstBuf, int i) {
        if constexpr (RES) return;
        constexpr int N = decltype(nfragC)::value;
        const int f = (int)waveS + i * kInrWaves;                    // scalar: the source is s[base] + lane * 16
        if ((N % kInrWaves == 0) ? (i < N / kInrWaves) : (f < N))
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(wp) + ((size_t)(fragStart + f) << 10) + (lane << 4)),
                (__attribute__((address_space(3))) void*)(&lds[dstBuf][f * 64]), 16, 0, 0);
    };
    auto stage_issue = [&](uint32_t fragStart, auto nfragC, int dstBuf) {
#pragma unroll
        for (int i = 0; i < PERW; ++i) stage_piece(fragStart, nfragC, dstBuf, i);
    };
    uint32_t curFrag = a.L.fragOff[0];                   // RES: first fragment of the chunk being read
    auto frag_at = [&](int buf, int f) {
        if constexpr (RES) return __builtin_bit_cast(bf16x8, ldsAll[(curFrag + f) * 64 + lane]);
        else return __builtin_bit_cast(bf16x8, lds[buf][f * 64 + lane]);
    };

    uint32_t nextFrag = a.L.fragOff[0];
    int buf = 0;
    if constexpr (RES) {
        for (uint32_t f = waveS; f < a.L.totalFrags; f += kInrWaves)     // the whole image, once
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(wp) + ((size_t)f << 10) + (lane << 4)),
                (__attribute__((address_space(3))) void*)(&ldsAll[f * 64]), 16, 0, 0);
    } else {
        stage_issue(nextFrag, IC<CH0>{}, 0);
    }
    nextFrag += CH0;

    // layer-0 B operands: this lane's point, features 16s + 8(j>>2) + 4h + (j&3) of k tile t
    bf16x8 xin_hi[KT0][2], xin_lo[KT0][2];
    // Every load below is unconditional and straight-line (clamped index, value masked afterwards): a load
    // inside a per-feature branch makes hipcc wait vmcnt(0) per feature — one memory round trip each.
    auto load_inputs = [&](int64_t pidx) {
        const int64_t p = pidx < nPts ? pidx : nPts - 1; // clamp: compute something, store nothing
        if (a.kind < 2) {
            // lane half 0 stages its point's raw inputs (3 coords + <= 8 modalities + a zero) in LDS ...
            float* raw = ldsRaw + waveS * 32 * kRawStride + r;       // [input][point]: lanes of a half hit 32 banks
            if (h == 0) {                                // (inr_refine_kernel's run_batch has the same block: see there)
                float c[3], m[kMaxMods];
                const uint32_t M = a.M;
                if (a.volume) {                          // model.py:124-128, fp64 then one rounding to fp32
                    const uint32_t k = (uint32_t)(p % a.D), j = (uint32_t)((p / a.D) % a.W), i = (uint32_t)(p / ((int64_t)a.D * a.W));
                    c[0] = (float)(((double)i / (double)(a.H - 1)) * 2.0 - 1.0);
                    c[1] = (float)(((double)j / (double)(a.W - 1)) * 2.0 - 1.0);
                    c[2] = (float)(((double)k / (double)(a.D - 1)) * 2.0 - 1.0);
                    const size_t hwd = (size_t)a.H * a.W * a.D;
#pragma unroll
                    for (uint32_t g = 0; g < kMaxMods; ++g) m[g] = M ? a.feats[(size_t)(g < M ? g : M - 1) * hwd + p] : 0.0f;
                } else {
                    c[0] = a.coords[p * 3 + 0]; c[1] = a.coords[p * 3 + 1]; c[2] = a.coords[p * 3 + 2];
#pragma unroll
                    for (uint32_t g = 0; g < kMaxMods; ++g) m[g] = M ? a.feats[p * (int64_t)M + (g < M ? g : M - 1)] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) raw[32 * k] = c[k];
#pragma unroll
                for (int k = 0; k < kMaxMods; ++k) raw[32 * (3 + k)] = m[k];
                raw[32 * (kRawStride - 1)] = 0.0f;
            }
            // ... and both halves build their features from the table (same wave: LDS ops are in order)
            // (eight descriptors, then eight raw values, then the arithmetic: two LDS latencies per k step
            // instead of two per feature)
#pragma unroll
            for (int t = 0; t < KT0; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float4 d[8];
                    float x[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) d[j] = ldsTab[32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[j] = raw[32 * __builtin_bit_cast(uint32_t, d[j].z)];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t mode = __builtin_bit_cast(uint32_t, d[j].w);
                        const float v = mode == 1u ? __builtin_amdgcn_sinf(__builtin_fmaf(x[j], d[j].x, d[j].y)) : x[j];
                        const __bf16 hi = (__bf16)v;
                        const __bf16 lo = (__bf16)(v - (float)hi);
                        xin_hi[t][s][j] = (AUG && mode == 2u) ? lo : hi;
                        xin_lo[t][s][j] = lo;
                    }
                }
        } else {
            // raw-x kinds (tests, other front ends): feats IS the [n][inDim] input matrix
#pragma unroll
            for (int t = 0; t < KT0; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t f = 32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
                        v[j] = a.feats[p * (int64_t)a.L.inDim + (f < a.L.inDim ? f : 0u)];
                        v[j] = f < a.L.inDim ? v[j] : 0.0f;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const __bf16 hi = (__bf16)v[j];
                        xin_hi[t][s][j] = hi;
                        xin_lo[t][s][j] = (__bf16)(v[j] - (float)hi);
                    }
                }
        }
    };

    bf16x8 Hc[KT][2];            // current layer's input, as B operands
    bf16x8 Hn[KT][2];            // next layer's input, built out tile by out tile

    // bias of out tile o for this lane half: rows 8g + 4h .. +3 (g = 0..3) = four aligned float4
    // The accumulator STARTS at the bias (accumulator register i holds row (i&3) + 8(i>>2) + 4h, i.e. the
    // four aligned float4 at rows 8g + 4h of the LDS copy), so no add is left for the activation.
    auto bias_tile = [&](uint32_t layerOff, int o) {                     // ds_read_b128 x 4
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b = ldsBias[(layerOff + 32 * o + 8 * g + 4 * h) >> 2];
            acc[4 * g + 0] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
        }
        return acc;
    };
    // one instruction per value (v_sin_f32 on revolutions: the 1/2pi and w0 are folded into the weights;
    // neumors_inr.ipynb:1165-1178) or half of one (v_pk_max_f32; model.py:46-48), plus the packed bf16 convert
    auto activate = [&](const f32x16& acc, int o) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int i = 8 * s + j;
                f32x2 x = { acc[i], acc[i + 1] };
                if (siren) { x.x = __builtin_amdgcn_sinf(x.x); x.y = __builtin_amdgcn_sinf(x.y); }
                else x = __builtin_elementwise_max(x, (f32x2){ 0.0f, 0.0f });
                Hn[o][s][j] = (__bf16)x.x;
                Hn[o][s][j + 1] = (__bf16)x.y;
            }
    };
    // The same activation, one slice per k step of the NEXT out tile.  The two waves of a SIMD leave the
    // chunk barrier in phase; with whole-tile activation they would both be in their VALU phase at once
    // and the matrix core would idle (measured: MFMA-busy + VALU cycles == kernel cycles).  Sliced under
    // the next tile's MFMAs, a v_sin_f32 (16 cycles) fits inside each MFMA's 32.
    auto act_slice = [&](f32x16& ap, int o, int step, auto nstepsC) {
        constexpr int NS = decltype(nstepsC)::value, PER = 16 / NS;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = step * PER + q;
            if (siren) ap[i] = __builtin_amdgcn_sinf(ap[i]);
            if (i & 1) {
                f32x2 x = { ap[i - 1], ap[i] };
                if (!siren) x = __builtin_elementwise_max(x, (f32x2){ 0.0f, 0.0f });
                Hn[o][i >> 3][(i & 7) - 1] = (__bf16)x.x;
                Hn[o][i >> 3][i & 7] = (__bf16)x.y;
            }
        }
    };
    // the chunk prefetched during this chunk's compute becomes current (hipcc drains the LDS-DMA
    // with vmcnt(0) at the barrier)
    auto next_chunk = [&]() {
        if constexpr (RES) curFrag = nextFrag;           // nothing is staged, nothing to wait for
        else { __syncthreads(); buf ^= 1; }
    };

    __syncthreads();                                     // biases and layer-0 chunk 0 are in LDS

    // Persistent workgroup: batches of 256 points, round-robin.  The weight stream is cyclic — the head
    // chunk stages layer 0's first chunk of the NEXT batch — so after the first batch no DMA latency,
    // workgroup launch or bias staging is exposed.
    const int64_t nBatches = (nPts + kInrWaves * 32 - 1) / (kInrWaves * 32);
    int64_t pendIdx = -1;
    int16_t pendVal = 0;
    for (int64_t batch = blockIdx.x; batch < nBatches; batch += gridDim.x) {
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    r = lane & 31u; h = lane >> 5;
    if (pendIdx >= 0) a.argmax[pendIdx] = pendVal;       // the previous batch's classes
    const int64_t pidx = (batch * kInrWaves + waveS) * 32 + r;
    load_inputs(pidx);

    // ---- layer 0: SIREN: hi/lo split, three products per k step; ReLU nets: one ------------------------------
    {
        const uint32_t b0 = a.L.biasOff[0];
#pragma unroll
        for (int og = 0; og < KT / OTC; ++og) {
            const int nfragNext = (og + 1 < KT / OTC) ? CH0 : (a.L.numLayers > 2 ? CHH : FH);   // layer 0 / layer 1 / head
            bf16x8 ring[RD];                             // fragment stream (SPLIT: even = hi, odd = lo of k step f/2)
#pragma unroll
            for (int d = 0; d < RD; ++d) if (d < CH0) ring[d] = frag_at(buf, d);
#pragma unroll
            for (int oo = 0; oo < OTC; ++oo) {
                const int o = og * OTC + oo;
                f32x16 acc = bias_tile(b0, o);
#pragma unroll
                for (int p = 0; p < KT0 * 2; ++p) {
                    const int t = p >> 1, s = p & 1, f = oo * F0 + (SPLIT ? 2 : 1) * p, step = oo * KT0 * 2 + p;
                    if (step % SP0 == 0 && step / SP0 < PERW) {
                        if (og + 1 < KT / OTC) stage_piece(nextFrag, IC<CH0>{}, buf ^ 1, step / SP0);    // folds: og is unrolled
                        else                   stage_piece(nextFrag, IC<CHH>{}, buf ^ 1, step / SP0);
                    }
                    if constexpr (SPLIT) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[(f + 1) % RD], xin_hi[t][s], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[f % RD], xin_lo[t][s], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[f % RD], xin_hi[t][s], acc, 0, 0, 0);
                        if (f + RD < CH0) ring[f % RD] = frag_at(buf, f + RD);
                        if (f + 1 + RD < CH0) ring[(f + 1) % RD] = frag_at(buf, f + 1 + RD);
                    } else {
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[f % RD], xin_hi[t][s], acc, 0, 0, 0);
                        if (f + RD < CH0) ring[f % RD] = frag_at(buf, f + RD);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                activate(acc, o);
            }
            next_chunk();
            nextFrag += nfragNext;
        }
    }

    // ---- hidden layers 1 .. L-2 ----------------------------------------------------------------------------
    for (uint32_t l = 1; l + 1 < a.L.numLayers; ++l) {
#pragma unroll
        for (int t = 0; t < KT; ++t) { Hc[t][0] = Hn[t][0]; Hc[t][1] = Hn[t][1]; }
        const uint32_t bl = a.L.biasOff[l];
        const bool lastHidden = l + 2 == a.L.numLayers;
        f32x16 accPrev;                                  // finished tile o - 1, activated under tile o's MFMAs
#pragma unroll
        for (int og = 0; og < KT / OTC; ++og) {
            const int nfragNext = (og + 1 < KT / OTC || !lastHidden) ? CHH : FH;    // more hidden tiles, or the head
            // A fragments run RD ahead of the MFMA that consumes them (the chunk is one fragment stream,
            // so the prefetch carries across out tiles): an LDS read is ~4 MFMA issue slots of latency
            bf16x8 ring[RD];
#pragma unroll
            for (int d = 0; d < RD; ++d) if (d < CHH) ring[d] = frag_at(buf, d);
#pragma unroll
            for (int oo = 0; oo < OTC; ++oo) {
                const int o = og * OTC + oo;
                f32x16 acc = bias_tile(bl, o);
#pragma unroll
                for (int ts = 0; ts < FH; ++ts) {
                    const int f = oo * FH + ts;
                    // right after the tile's bias read: hipcc makes any LDS read it cannot tell apart from the
                    // DMA target wait vmcnt(0), so a piece still in flight at the next tile's bias read stalls it
                    if constexpr (FH > PPT) {
                        if (ts >= 1 && ts <= PPT && oo * PPT + ts - 1 < PERW) stage_piece(nextFrag, IC<CHH>{}, buf ^ 1, oo * PPT + ts - 1);
                    } else {
                        if (f % SPH == 0 && f / SPH < PERW) stage_piece(nextFrag, IC<CHH>{}, buf ^ 1, f / SPH);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[f % RD], Hc[ts >> 1][ts & 1], acc, 0, 0, 0);
                    if (f + RD < CHH) ring[f % RD] = frag_at(buf, f + RD);
                    if (o > 0) act_slice(accPrev, o - 1, ts, IC<FH>{});
                    __builtin_amdgcn_sched_barrier(0);   // keep the refill RD steps ahead (the scheduler would sink it)
                }
                accPrev = acc;
            }
            next_chunk();
            nextFrag += nfragNext;
        }
#pragma unroll
        for (int ts = 0; ts < FH; ++ts) act_slice(accPrev, KT - 1, ts, IC<FH>{});     // the layer's last tile
    }

    // ---- head: one out tile (outDim <= 16 rows used), linear ---------------------------------------------------
    {
        f32x16 acc = bias_tile(a.L.biasOff[a.L.numLayers - 1], 0);      // rows >= outDim: zero padding
        stage_issue(a.L.fragOff[0], IC<CH0>{}, buf ^ 1);                 // the next batch's first chunk
        bf16x8 ring[RD];
#pragma unroll
        for (int d = 0; d < RD; ++d) if (d < FH) ring[d] = frag_at(buf, d);
#pragma unroll
        for (int f = 0; f < FH; ++f) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[f % RD], Hn[f >> 1][f & 1], acc, 0, 0, 0);
            if (f + RD < FH) ring[f % RD] = frag_at(buf, f + RD);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (a.logits != nullptr && pidx < nPts) {         // uniform pointer test; not the throughput path
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t cls = (i & 3) + 8 * (i >> 2) + 4 * h;
                if (cls < a.L.outDim) a.logits[pidx * a.L.outDim + cls] = acc[i];
            }
        }
        // np.argmax = first maximum.  Within a lane cls grows with i, so a strict > keeps the first; the
        // two lane halves hold interleaved classes, so the merge breaks ties towards the smaller class.
        float best = -INFINITY, second = -INFINITY;
        uint32_t bestc = 4 * h;                          // this half's first class (all -inf: class 0, as numpy)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t cls = (i & 3) + 8 * (i >> 2) + 4 * h;
            const float v = cls < a.L.outDim ? acc[i] : -INFINITY;
            top2_push(v, cls, best, second, bestc);
        }
        const float ob = __shfl_xor(best, 32), os = __shfl_xor(second, 32);
        const uint32_t oc = __shfl_xor(bestc, 32);
        if (ob > best || (ob == best && oc < bestc)) { second = fmaxf(best, os); best = ob; bestc = oc; }
        else second = fmaxf(second, ob);
        // near-tie mark (see kFlagBit): the refinement kernel re-evaluates this point; NaN gaps are marked too
        const bool tie = a.tie != nullptr && !(best - second >= tieThr);
        // stored at the top of the next batch: issued here, the store would still be in flight at the
        // chunk barrier below, whose vmcnt(0) (for the DMA) would then wait out its whole HBM round trip
        pendIdx = (a.argmax && h == 0 && pidx < nPts) ? pidx : -1;
        pendVal = (int16_t)(bestc | (tie ? (uint32_t)kFlagBit : 0u));
    }
    next_chunk();
    nextFrag = a.L.fragOff[0] + CH0;
    if constexpr (RES) curFrag = a.L.fragOff[0];
    }   // batch
    if (pendIdx >= 0) a.argmax[pendIdx] = pendVal;
}

template <int HID, bool RES>
static InrKernel stream_kernel(const InrArgs& a) {
    return inr_select_kernel(a, [](auto kt0, auto siren, auto aug) -> InrKernel {
        return inr_forward_kernel<HID, decltype(kt0)::value, decltype(siren)::value != 0, decltype(aug)::value != 0, RES>;
    });
}

template <int HID>
static int launch_inr_kt0(const InrArgs& a, hipStream_t s) {
    const int64_t groups = (a.n + kInrWaves * 32 - 1) / (kInrWaves * 32);
    const bool siren = a.kind == MRIRT_INR_SIREN || a.kind == 3u;
    InrKernel kern = stream_kernel<HID, false>(a);
    bool res = false;
    if constexpr (HID <= 64) {
        if (a.L.totalFrags <= (uint32_t)kResidentFrags) {
            res = true;
            kern = stream_kernel<HID, true>(a);
        }
    }
    // persistent workgroups: as many as are resident at once (the 4 x 256 nets: one per CU, 150 KB of LDS)
    // cached per device and kernel family; a relaxed atomic: two threads racing here compute the same number
    constexpr int kMaxDev = 16;
    static std::atomic<int> resident[kMaxDev][2][2][3];
    int dev = 0;
    MRIRT_HIP(hipGetDevice(&dev));
    std::atomic<int>& slot = resident[dev >= 0 && dev < kMaxDev ? dev : 0][res ? 1 : 0][a.L.kt0 == 1 ? 0 : 1][siren ? (a.L.aug0 ? 2 : 1) : 0];
    int nres = (dev >= 0 && dev < kMaxDev) ? slot.load(std::memory_order_relaxed) : 0;
    if (nres == 0) {
        int cus = 0, perCu = 0;
        MRIRT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        MRIRT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kern, kInrWaves * 64, 0));
        nres = (cus > 0 ? cus : 256) * (perCu > 0 ? perCu : 1);
        if (dev >= 0 && dev < kMaxDev) slot.store(nres, std::memory_order_relaxed);
    }
    const dim3 grid((uint32_t)(groups < nres ? groups : nres)), block(kInrWaves * 64);
    hipLaunchKernelGGL(kern, grid, block, 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

int launch_inr_stream(const InrArgs& a, hipStream_t s) {
    if ((a.n + kInrWaves * 32 - 1) / (kInrWaves * 32) >= (1ll << 31)) return MRIRT_ERR_ARG;
    switch (a.L.hidden) {
        case 32: return launch_inr_kt0<32>(a, s);
        case 64: return launch_inr_kt0<64>(a, s);
        case 128: return launch_inr_kt0<128>(a, s);
        default: return launch_inr_kt0<256>(a, s);
    }
}

}  // namespace mrirt
