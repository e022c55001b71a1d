// INR forward, the near-tie refinement kernel (why points are marked and how: inr_mlp.hip).
#include "inr_fwd.h"

namespace mrirt {

// =====================================================================================================
// Near-tie refinement: the marked points (kFlagBit in the stored class) once more, with split-bf16 operands in
// every layer — W = W_hi + W_lo, H = H_hi + H_lo (bf16 each), three MFMAs per k step (lo.hi + hi.lo + hi.hi,
// fp32 accumulate): ~16 mantissa bits per operand instead of 8, so the class agrees with the fp32 reference except
// on ties three orders of magnitude closer (measured: logits within 2e-5 of the range, profiles/r03_inr_refine.txt).
// 2-3 % of the points of a random 4-class head take this path (none of a confident one), at three times the MFMA
// work each.
//
// Dataflow: the streaming kernel's (transposed layers, the accumulator tile is the next layer's B operand; both
// halves of the split stay in registers), simplified where 3 % of the work allows: 4 waves x 32 points per batch,
// ONE wave per SIMD (the hi + lo activations of two layers are 256 registers).  Weights come from the refine image
// one out tile (<= 32 KiB; layer 0: as many tiles as fit) at a time by LDS-DMA into a ring of four LDS buffers,
// THREE tiles ahead of the MFMAs: a tile's MFMAs take 0.6 us and an L2 round trip more than that, so one tile in
// flight left the kernel latency-bound (measured: 2.8 us per tile).  The DMAs span the workgroup barriers: counted
// s_waitcnt vmcnt(2 tiles' pieces) + a raw s_barrier per tile (guide: "Pipelining across barriers"); every tile is
// exactly PERW DMA instructions per wave (a full ring slot: a short tile drags the fragments behind it into slots nobody
// reads) so that the count is one immediate, and in the hidden layers they are issued one at a time between the k steps
// (issue_part); the stream is cyclic (after the head comes layer 0 again), so a batch starts with its first three tiles
// already in LDS.
// Work list: a workgroup scans interleaved 2048-point segments of the class array for marks (16-byte loads), collects the point
// ids in LDS and runs a batch whenever 128 are waiting (the remainder at the end): no global compaction pass, nothing for
// the host to size; the only global atomic is the optional segment ticket (InrArgs::segTicket: the C5 passes).
// =====================================================================================================
constexpr int kRefWaves = 4;
// Diagnostic build (-DMRIRT_REF_STAMPS): s_memtime at the phase boundaries of every workgroup's second batch goes to the logits
// buffer (which then holds no logits): [block][wave][64] uint64, decoded by tools/refine_stamps.py.  Never in the product.
#ifdef MRIRT_REF_STAMPS
#define REF_STAMP(k) do { if (a.logits != nullptr && batchNo == 1u && lane == 0) reinterpret_cast<unsigned long long*>(a.logits)[((size_t)blockIdx.x * 4 + waveS) * 64 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define REF_STAMP(k) do { } while (0)
#endif

template <int HID, int KT0, bool SIREN, bool AUG>
__global__ __launch_bounds__(256, 1) void inr_refine_kernel(const InrArgs a) {
    constexpr int KT = HID / 32;
    constexpr bool L0SPLIT = !AUG;                       // AUG: layer 0's split is folded into its k axis already
    constexpr int NK0 = KT0 * 2, NKH = KT * 2;           // k steps of an out tile: layer 0 / the wider layers
    constexpr int F0 = NK0 * (L0SPLIT ? 2 : 1), FH = NKH * 2;   // fragments of an out tile
    constexpr int FMAX = F0 > FH ? F0 : FH;
    constexpr int C0 = (FMAX / F0) < KT ? (FMAX / F0 > 0 ? FMAX / F0 : 1) : KT;   // layer-0 out tiles per DMA tile
    static_assert(KT % C0 == 0 && C0 * F0 <= FMAX && FMAX % kRefWaves == 0, "layer-0 chunking");
    constexpr int PERW = FMAX / kRefWaves;               // DMA instructions per wave per tile (always this many)
    constexpr int NBUF = 4, AHEAD = NBUF - 1;            // LDS ring; tiles in flight ahead of the one being read
    constexpr int RD = 4;                                // k steps of A fragments in registers ahead of their MFMAs
    constexpr int kScanV = 8, kSeg = 256 * kScanV;       // a scan step reads 2048 classes: eight consecutive ones (16 bytes) per thread
    constexpr int kBatch = kRefWaves * 32;
    constexpr int kListCap = kBatch + kSeg;
    constexpr int kBiasQ = kMaxLayers * 256 / 4, kTabQ = 128, kRawQ = kRefWaves * 32 * kRawStride / 4;
    constexpr int kWQ = NBUF * FMAX * 64;
    __shared__ uint4 ldsAll[kWQ + kBiasQ + kTabQ + kRawQ + kListCap / 4 + 1];       // ONE LDS object (guide: a second one de-pipelines the DMA); the last uint4: listCount[0..1]
    const float4* ldsBias = reinterpret_cast<const float4*>(ldsAll + kWQ);
    float4* ldsTab = reinterpret_cast<float4*>(ldsAll + kWQ + kBiasQ);
    float* ldsRaw = reinterpret_cast<float*>(ldsAll + kWQ + kBiasQ + kTabQ);
    uint32_t* list = reinterpret_cast<uint32_t*>(ldsAll + kWQ + kBiasQ + kTabQ + kRawQ);
    uint32_t* listCount = list + kListCap;

    const int64_t nPts = inr_point_count(a);
    if (nPts <= 0 || (int64_t)blockIdx.x * kSeg >= nPts) return;       // uniform

    if (a.kind < 2 && threadIdx.x < 128) ldsTab[threadIdx.x] = inr_feature_entry<AUG>(a, threadIdx.x);
    inr_stage_biases(a, ldsAll + kWQ);
    if (threadIdx.x == 0) *listCount = 0u;

    const uint32_t lane = threadIdx.x & 63u, r = lane & 31u, h = lane >> 5;
    const uint32_t waveS = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint4* __restrict__ wr = a.wpack + (size_t)ref_base_frag(a.L) * 64;      // the refine image

    // ---- the cyclic tile stream: layer 0 in chunks of C0 out tiles, then one out tile at a time, the head, and again ----
    const uint32_t ldsBase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)ldsAll;
    uint32_t isLayer = 0, isTile = 0, isFrag = a.L.refFragOff[0];     // the next tile to ISSUE (scalars)
    uint32_t ringIssue = 0, ringRead = 0;                              // ring slots: next to fill / being read
    bool primed = false;
    uint32_t batchNo = 0;
    // One tile's DMAs in PERW parts, so that the hidden layers can place them in the shadows of their MFMAs: a lone wave issues
    // an instruction every ~8 cycles, and the all-at-once form with its per-DMA address arithmetic (64 instructions) held the
    // MFMAs up for 520 cycles per tile (s_memtime stamps, round 4).  Wave w moves fragments w * PERW .. w * PERW + PERW - 1 of the
    // tile into the slots of the same numbers: ONE address register pair and one M0 value per four parts plus the instruction's
    // immediate offset, which the hardware adds to the global AND the LDS address.  Every tile moves a full ring slot (FMAX
    // fragments): a short tile (layer 0's) drags the fragments that follow it into slots nobody reads, and the image ends in
    // kRefSlackFrags of slack for the last one.
    static_assert(FMAX <= kRefSlackFrags, "the slack after the refine image covers one ring slot");
    const char* curSrc = nullptr;                                     // this wave's first fragment of the tile being issued (+ lane * 16)
    uint32_t curDst = 0;                                              // its ring slot (LDS byte address)
    auto issue_begin = [&]() {
        curSrc = reinterpret_cast<const char*>(wr) + ((size_t)(isFrag + waveS * PERW) << 10) + (lane << 4);
        curDst = __builtin_amdgcn_readfirstlane(ldsBase + ((ringIssue * FMAX + waveS * PERW) << 10));
    };
    auto issue_part = [&](int i) {                                    // (a constant once the caller's loop is unrolled)
        // Issued as inline asm ON PURPOSE: told about an LDS-DMA, hipcc makes the next ds_read whose address it cannot
        // tell apart from the DMA's target (a ring slot chosen at run time) wait vmcnt(0) — the whole look-ahead drained
        // once per tile (seen in the ISA of the builtin form).  The waits for these loads are the counted ones in
        // tile_done(); hipcc's own counted waits (for the batch's input loads) can only over-wait, never under-wait.
        const char* src = curSrc + (i >> 2) * 4096;
        const uint32_t dst = curDst + (uint32_t)((i >> 2) * 4096);
        switch (i & 3) {
            case 0:  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(src), "s"(dst) : "memory", "m0"); break;
            case 1:  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off offset:1024" :: "v"(src), "s"(dst) : "memory", "m0"); break;
            case 2:  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off offset:2048" :: "v"(src), "s"(dst) : "memory", "m0"); break;
            default: asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off offset:3072" :: "v"(src), "s"(dst) : "memory", "m0"); break;
        }
    };
    auto issue_end = [&]() {
        const uint32_t last = a.L.numLayers - 1;
        isFrag += isLayer == 0 ? (uint32_t)(C0 * F0) : (uint32_t)FH;
        const uint32_t tilesHere = isLayer == 0 ? (uint32_t)(KT / C0) : (isLayer == last ? 1u : (uint32_t)KT);
        if (++isTile == tilesHere) { isTile = 0; if (++isLayer > last) { isLayer = 0; isFrag = a.L.refFragOff[0]; } }
        ringIssue = ringIssue + 1 == NBUF ? 0u : ringIssue + 1;
    };
    auto issue_tile = [&]() {
        issue_begin();
#pragma unroll
        for (int i = 0; i < PERW; ++i) issue_part(i);
        issue_end();
    };
    // end of a tile: this wave's pieces of the NEXT tile have landed (the two after it may still be in flight), its own
    // LDS reads of this tile have retired; after the barrier that holds for every wave
    auto tile_done = [&]() {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PERW * (AHEAD - 1)) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        ringRead = ringRead + 1 == NBUF ? 0u : ringRead + 1;
    };
    auto frag_at = [&](int f) { return __builtin_bit_cast(bf16x8, ldsAll[(ringRead * FMAX + f) * 64 + lane]); };

    // ---- one batch: list[off .. off + m) ---------------------------------------------------------------------
    auto run_batch = [&](uint32_t off, uint32_t m) {
        const uint32_t slot = waveS * 32 + r;
        const bool valid = slot < m;
        const int64_t p = (int64_t)list[off + (valid ? slot : 0u)];

        // layer-0 B operands (the streaming kernel's load_inputs, for an arbitrary point id)
        bf16x8 xin_hi[KT0][2], xin_lo[KT0][2];
        if (a.kind < 2) {
            float* raw = ldsRaw + waveS * 32 * kRawStride + r;
            // The h == 0 block of inr_forward_kernel's load_inputs, kept as a second copy: as one shared __forceinline__ function it
            // changed the register figures of both kernels (profiles/r16_inr_split/README.txt)
            if (h == 0) {
                float c[3], mm[kMaxMods];
                const uint32_t M = a.M;
                if (a.volume) {
                    const uint32_t k = (uint32_t)(p % a.D), j = (uint32_t)((p / a.D) % a.W), i = (uint32_t)(p / ((int64_t)a.D * a.W));
                    c[0] = (float)(((double)i / (double)(a.H - 1)) * 2.0 - 1.0);
                    c[1] = (float)(((double)j / (double)(a.W - 1)) * 2.0 - 1.0);
                    c[2] = (float)(((double)k / (double)(a.D - 1)) * 2.0 - 1.0);
                    const size_t hwd = (size_t)a.H * a.W * a.D;
#pragma unroll
                    for (uint32_t g = 0; g < kMaxMods; ++g) mm[g] = M ? a.feats[(size_t)(g < M ? g : M - 1) * hwd + p] : 0.0f;
                } else {
                    c[0] = a.coords[p * 3 + 0]; c[1] = a.coords[p * 3 + 1]; c[2] = a.coords[p * 3 + 2];
#pragma unroll
                    for (uint32_t g = 0; g < kMaxMods; ++g) mm[g] = M ? a.feats[p * (int64_t)M + (g < M ? g : M - 1)] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) raw[32 * k] = c[k];
#pragma unroll
                for (int k = 0; k < kMaxMods; ++k) raw[32 * (3 + k)] = mm[k];
                raw[32 * (kRawStride - 1)] = 0.0f;
            }
#pragma unroll
            for (int t = 0; t < KT0; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float4 d = ldsTab[32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)];
                        const float x = raw[32 * __builtin_bit_cast(uint32_t, d.z)];
                        const uint32_t mode = __builtin_bit_cast(uint32_t, d.w);
                        const float v = mode == 1u ? __builtin_amdgcn_sinf(__builtin_fmaf(x, d.x, d.y)) : x;
                        const __bf16 hi = (__bf16)v;
                        const __bf16 lo = (__bf16)(v - (float)hi);
                        xin_hi[t][s][j] = (AUG && mode == 2u) ? lo : hi;
                        xin_lo[t][s][j] = lo;
                    }
                }
        } else {
#pragma unroll
            for (int t = 0; t < KT0; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t f = 32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
                        float v = a.feats[p * (int64_t)a.L.inDim + (f < a.L.inDim ? f : 0u)];
                        v = f < a.L.inDim ? v : 0.0f;
                        const __bf16 hi = (__bf16)v;
                        xin_hi[t][s][j] = hi;
                        xin_lo[t][s][j] = (__bf16)(v - (float)hi);
                    }
        }
        // the inputs are in registers (the compiler has waited for every ordinary load above, and with it for any DMA
        // still in flight); from here to the end of the batch the only vector-memory operations in flight are DMAs
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (!primed) {                                   // first batch of this workgroup: start the stream
#pragma unroll
            for (int d = 0; d < AHEAD; ++d) issue_tile();
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PERW * (AHEAD - 1)) : "memory");
            primed = true;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                    // first tile in LDS for every wave (and table + biases + list on the first batch)

        // the activations of two layers, hi and lo halves of the split, as PACKED 32-bit words (two bf16 each; word j of
        // [tile][0..7] = elements 2j, 2j + 1 of the tile's 16 per lane).  Written a word at a time by act_pair: element-wise
        // inserts into bf16x8 made hipcc keep every value as an fp32 register until its partner arrived and convert again
        // at the layer's end (round 4: 417 + 161 registers, 128 v_cvt_pk and as many v_accvgpr moves per layer).
        uint32_t Hc_hi[KT][8], Hc_lo[KT][8], Hn_hi[KT][8], Hn_lo[KT][8];
        auto b_frag = [&](const uint32_t (&hw)[8], int s2) {
            return __builtin_bit_cast(bf16x8, make_uint4(hw[4 * s2], hw[4 * s2 + 1], hw[4 * s2 + 2], hw[4 * s2 + 3]));
        };
        auto bias_tile = [&](uint32_t layerOff, int o) {
            f32x16 acc;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b = ldsBias[(layerOff + 32 * o + 8 * g + 4 * h) >> 2];
                acc[4 * g + 0] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
            }
            return acc;
        };
        // activation of elements i, i + 1 (i even), then the split of the results: hi = bf16(x), lo = bf16(x - hi)
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        auto act_pair = [&](const f32x16& acc, int o, int i) {
            float x0 = acc[i], x1 = acc[i + 1];
            if constexpr (SIREN) { x0 = __builtin_amdgcn_sinf(x0); x1 = __builtin_amdgcn_sinf(x1); }
            else { x0 = fmaxf(x0, 0.0f); x1 = fmaxf(x1, 0.0f); }
            const bf16x2 hi = { (__bf16)x0, (__bf16)x1 };
            const uint32_t hp = __builtin_bit_cast(uint32_t, hi);
            const bf16x2 lo = { (__bf16)(x0 - __builtin_bit_cast(float, hp << 16)), (__bf16)(x1 - __builtin_bit_cast(float, hp & 0xffff0000u)) };
            Hn_hi[o][i >> 1] = hp;
            Hn_lo[o][i >> 1] = __builtin_bit_cast(uint32_t, lo);
        };
        auto activate = [&](const f32x16& acc, int o) {
#pragma unroll
            for (int i = 0; i < 16; i += 2) act_pair(acc, o, i);
        };
        // the three products of one k step (small terms first)
        auto mfma3 = [&](f32x16& acc, const bf16x8& whi, const bf16x8& wlo, const bf16x8& bhi, const bf16x8& blo) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, bhi, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, blo, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, bhi, acc, 0, 0, 0);
        };

        // ---- layer 0 -----------------------------------------------------------------------------------------
        REF_STAMP(0);
#ifdef MRIRT_REF_STAMPS
        if (a.logits != nullptr && batchNo == 2u && lane == 0) reinterpret_cast<unsigned long long*>(a.logits)[((size_t)blockIdx.x * 4 + waveS) * 64 + 6] = __builtin_amdgcn_s_memtime();
#endif
        {
            const uint32_t b0 = a.L.biasOff[0];
#pragma unroll
            for (int c = 0; c < KT / C0; ++c) {
                issue_tile();
#pragma unroll
                for (int oo = 0; oo < C0; ++oo) {
                    const int o = c * C0 + oo;
                    f32x16 acc = bias_tile(b0, o);
#pragma unroll
                    for (int q = 0; q < NK0; ++q) {
                        const int t = q >> 1, s2 = q & 1;
                        if constexpr (L0SPLIT) mfma3(acc, frag_at(oo * F0 + 2 * q), frag_at(oo * F0 + 2 * q + 1), xin_hi[t][s2], xin_lo[t][s2]);
                        else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(oo * F0 + q), xin_hi[t][s2], acc, 0, 0, 0);
                    }
                    activate(acc, o);
                }
                tile_done();
            }
        }
        // ---- hidden layers -----------------------------------------------------------------------------------
        REF_STAMP(1);
        for (uint32_t l = 1; l + 1 < a.L.numLayers; ++l) {
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) { Hc_hi[t][j] = Hn_hi[t][j]; Hc_lo[t][j] = Hn_lo[t][j]; }
            const uint32_t bl = a.L.biasOff[l];
            f32x16 accPrev;                              // finished tile o - 1: activated and split under tile o's MFMAs
            f32x16 biasNext;                             // tile o + 1's biases (its initial accumulator), read under tile o's MFMAs
#pragma unroll
            for (int o = 0; o < KT; ++o) {
                if (l == 2) REF_STAMP(8 + 3 * o);
                issue_begin();
                if (l == 2 && o == 2) REF_STAMP(40);
                f32x16 acc = o == 0 ? bias_tile(bl, 0) : biasNext;
                bf16x8 rhi[RD], rlo[RD];
#pragma unroll
                for (int d = 0; d < RD; ++d) if (d < NKH) { rhi[d] = frag_at(2 * d); rlo[d] = frag_at(2 * d + 1); }
#pragma unroll
                for (int q = 0; q < NKH; ++q) {
                    mfma3(acc, rhi[q % RD], rlo[q % RD], b_frag(Hc_hi[q >> 1], q & 1), b_frag(Hc_lo[q >> 1], q & 1));
                    if (l == 2 && o == 2) REF_STAMP(41 + q);
                    if (q + RD < NKH) { rhi[q % RD] = frag_at(2 * (q + RD)); rlo[q % RD] = frag_at(2 * (q + RD) + 1); }
#pragma unroll
                    for (int i = q * PERW / NKH; i < (q + 1) * PERW / NKH; ++i) issue_part(i);      // the tile three ahead
                    if (q == NKH / 2 && o + 1 < KT) biasNext = bias_tile(bl, o + 1);
                    if (o > 0) {                     // the pairs complete by the end of this k step
#pragma unroll
                        for (int pr = (q * 16 / NKH) / 2; pr < ((q + 1) * 16 / NKH) / 2; ++pr) act_pair(accPrev, o - 1, 2 * pr);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // keep the slices where they are written: one per k step
                }
                issue_end();
                accPrev = acc;
                if (l == 2) REF_STAMP(9 + 3 * o);
                tile_done();
                if (l == 2) REF_STAMP(10 + 3 * o);
            }
            activate(accPrev, KT - 1);                   // the layer's last tile
            REF_STAMP(1 + l);
        }
        // ---- head ----------------------------------------------------------------------------------------------
        {
            REF_STAMP(32);
            issue_tile();
            REF_STAMP(33);
            f32x16 acc = bias_tile(a.L.biasOff[a.L.numLayers - 1], 0);
            bf16x8 rhi[RD], rlo[RD];
#pragma unroll
            for (int d = 0; d < RD; ++d) if (d < NKH) { rhi[d] = frag_at(2 * d); rlo[d] = frag_at(2 * d + 1); }
#pragma unroll
            for (int q = 0; q < NKH; ++q) {
                mfma3(acc, rhi[q % RD], rlo[q % RD], b_frag(Hn_hi[q >> 1], q & 1), b_frag(Hn_lo[q >> 1], q & 1));
                if (q + RD < NKH) { rhi[q % RD] = frag_at(2 * (q + RD)); rlo[q % RD] = frag_at(2 * (q + RD) + 1); }
            }
            REF_STAMP(34);
            float best = -INFINITY, second = -INFINITY;
            uint32_t bestc = 4 * h;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t cls = (i & 3) + 8 * (i >> 2) + 4 * h;
                top2_push(cls < a.L.outDim ? acc[i] : -INFINITY, cls, best, second, bestc);
            }
            const float ob = __shfl_xor(best, 32);
            const uint32_t oc = __shfl_xor(bestc, 32);
            if (ob > best || (ob == best && oc < bestc)) { best = ob; bestc = oc; }
            REF_STAMP(35);
            tile_done();                                 // (before the stores: they would count against the DMA budget)
            REF_STAMP(5);
            ++batchNo;
#ifdef MRIRT_REF_STAMPS
            if (false) {
#else
            if (a.logits != nullptr && valid) {
#endif
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t cls = (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (cls < a.L.outDim) a.logits[p * a.L.outDim + cls] = acc[i];
                }
            }
            if (a.argmax != nullptr && valid && h == 0) a.argmax[p] = (int16_t)bestc;       // the clean class
        }
    };

    // ---- scan for marks, batch as they accumulate ------------------------------------------------------------
    uint32_t cnt = 0;                                    // replicated in every thread: entries waiting in `list`
    __syncthreads();
    const bool vecOK = (reinterpret_cast<uintptr_t>(a.argmax) & 15u) == 0;       // (a sliced tensor: element loads)
    for (int64_t seg = blockIdx.x; seg * kSeg < nPts; ) {
        const int64_t i0 = seg * kSeg + (int64_t)threadIdx.x * kScanV;
        // Eight classes per thread in ONE 16-byte load (round 4: four strided 2-byte loads per thread made the scan of 67 M classes
        // 1.2 ms — half of what the whole second pass cost; now 0.1 ms)
        uint32_t w[4] = { 0u, 0u, 0u, 0u };
        if (!a.refineAll && i0 < nPts) {
            if (vecOK && i0 + kScanV <= nPts) {
                const uint4 q = *reinterpret_cast<const uint4*>(a.argmax + i0);
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < kScanV; ++j)
                    if (i0 + j < nPts) w[j >> 1] |= (uint32_t)(uint16_t)a.argmax[i0 + j] << (16 * (j & 1));
            }
        }
        // the segment after this one: the next of the round-robin deal, or the next nobody has taken yet
        if (a.segTicket != nullptr && threadIdx.x == 0) listCount[1] = atomicAdd(a.segTicket, 1u);
        uint64_t mk[kScanV];
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < kScanV; ++j) {
            const bool marked = i0 + j < nPts && (a.refineAll != 0u || ((w[j >> 1] >> (16 * (j & 1))) & (uint32_t)kFlagBit) != 0u);
            mk[j] = __ballot(marked);
            total += (uint32_t)__popcll(mk[j]);
        }
        if (total != 0) {                                // wave-uniform: one LDS atomic per wave and step
            uint32_t wbase = 0;
            if (lane == 0) wbase = atomicAdd(listCount, total);
            wbase = __shfl(wbase, 0);
#pragma unroll
            for (int j = 0; j < kScanV; ++j) {
                if ((mk[j] >> lane) & 1ull)
                    list[wbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk[j], 0u))] = (uint32_t)(i0 + j);
                wbase += (uint32_t)__popcll(mk[j]);
            }
        }
        __syncthreads();
        cnt = *listCount;
        const int64_t nextSeg = a.segTicket != nullptr ? (int64_t)gridDim.x + (int64_t)listCount[1] : seg + (int64_t)gridDim.x;
        const bool lastSeg = nextSeg * kSeg >= nPts;                 // after the last segment the remainder goes as a short batch
        while (cnt >= (uint32_t)kBatch || (lastSeg && cnt > 0)) {    // (ONE call site: the batch body is inlined once)
            const uint32_t m = cnt < (uint32_t)kBatch ? cnt : (uint32_t)kBatch;
            run_batch(cnt - m, m);
            cnt -= m;
        }
        __syncthreads();                                 // every wave has read its list entries (and the next segment's number)
        if (threadIdx.x == 0) *listCount = cnt;
        __syncthreads();
        seg = nextSeg;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the stream's look-ahead DMAs: nothing may be in flight at exit
}

template <int HID>
static int launch_refine_hid(const InrArgs& a, hipStream_t s) {
    const InrKernel kern = inr_select_kernel(a, [](auto kt0, auto siren, auto aug) -> InrKernel {
        return inr_refine_kernel<HID, decltype(kt0)::value, decltype(siren)::value != 0, decltype(aug)::value != 0>;
    });
    int dev = 0, cus = 0;
    MRIRT_HIP(hipGetDevice(&dev));
    MRIRT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int64_t segs = (a.n + 2047) / 2048, nres = cus > 0 ? cus : 256;       // one workgroup per CU (512 registers per wave); 2048-class scan steps
    const dim3 grid((uint32_t)(segs < nres ? segs : nres));
#ifdef MRIRT_REF_STAMPS
    // the stamps go where the logits would: [block][wave][64] uint64 must fit the n * outDim floats
    if (a.logits != nullptr && (uint64_t)a.n * a.L.outDim * sizeof(float) < (uint64_t)grid.x * 4 * 64 * 8) return MRIRT_ERR_ARG;
#endif
    hipLaunchKernelGGL(kern, grid, dim3(kRefWaves * 64), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

// the split-bf16 pass over the marked points of a.argmax (or over every point: a.refineAll)
int launch_refine(const InrArgs& a, hipStream_t s) {
    if (a.n >= (1ll << 32)) return MRIRT_ERR_ARG;        // point ids travel as 32-bit words
    switch (a.L.hidden) {
        case 32: return launch_refine_hid<32>(a, s);
        case 64: return launch_refine_hid<64>(a, s);
        case 128: return launch_refine_hid<128>(a, s);
        default: return launch_refine_hid<256>(a, s);
    }
}

}  // namespace mrirt
