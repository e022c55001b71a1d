// INR training loop (csrc/inr_optim.hip): the counter-based voxel sampler, the global-norm reduction and the AdamW update.
// Their index arithmetic is written once here, for the device kernels and for the host (tests/native/inr_loop_harness.hip
// walks it under AddressSanitizer + UBSan over buffers of exactly the real sizes).  DESIGN.md section 15.
#pragma once
#include <stdint.h>

#include "inr_train.h"

namespace mrirt {

constexpr uint32_t kOptThreads = 256;
constexpr uint32_t kOptMaxBlocks = 256;       // blocks of the norm pass: one fp64 partial sum each
constexpr uint32_t kCacheMaxMods = 8;
constexpr uint32_t kCacheMaxCases = 65535;

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -------------------------
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

MRIRT_HD uint32_t mulhi32(uint32_t r, uint32_t m) { return (uint32_t)(((uint64_t)r * m) >> 32); }

// c (counter) <- ten rounds under key (k0, k1); the key is bumped by the Weyl constants between rounds
MRIRT_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c[0], p1 = (uint64_t)kPhiloxM1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
}

// ---- sampler -----------------------------------------------------------------------------------------------------------------
struct SamplePoint { uint32_t cs, x, y, z; };

// point i of micro-batch b under `seed`: key (seed lo, seed hi), counter (i, b lo, b hi, 0); no rejection step
MRIRT_HD SamplePoint sample_point(uint64_t seed, uint64_t batch, uint32_t i, uint32_t ncases, uint32_t H, uint32_t W, uint32_t D) {
    uint32_t c[4] = { i, (uint32_t)batch, (uint32_t)(batch >> 32), 0u };
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    SamplePoint p;
    p.cs = mulhi32(c[0], ncases); p.x = mulhi32(c[1], H); p.y = mulhi32(c[2], W); p.z = mulhi32(c[3], D);
    return p;
}
// element offset of voxel (x, y, z) in seg[H][W][D], and of modality m's copy of it in mods[M][H][W][D]
MRIRT_HD int64_t voxel_offset(uint32_t x, uint32_t y, uint32_t z, uint32_t W, uint32_t D) {
    return ((int64_t)x * W + y) * (int64_t)D + z;
}
MRIRT_HD int64_t mod_offset(uint32_t m, int64_t voxel, int64_t hwd) { return (int64_t)m * hwd + voxel; }
// the arithmetic of sample_batch and predict_volume: (index / (extent - 1)) * 2 - 1, every operation rounded to fp32
MRIRT_HD float sample_coord(uint32_t i, uint32_t extent) { return ((float)i / (float)(extent - 1u)) * 2.0f - 1.0f; }

// ---- global norm -------------------------------------------------------------------------------------------------------------
MRIRT_HD uint32_t opt_blocks(int64_t n) {
    const uint64_t b = ((uint64_t)n + kOptThreads - 1) / kOptThreads;
    return (uint32_t)(b < kOptMaxBlocks ? b : kOptMaxBlocks);
}
// thread t of block b sums elements opt_first(b, t), + opt_stride(blocks), ... below n of the virtual array [gw | gb]
MRIRT_HD int64_t opt_first(uint32_t block, uint32_t thread) { return (int64_t)block * kOptThreads + thread; }
MRIRT_HD int64_t opt_stride(uint32_t blocks) { return (int64_t)blocks * kOptThreads; }
// doubles: [opt_blocks(n)] partial sums
MRIRT_HD uint64_t opt_scratch_bytes(int64_t n) { return tr_align((uint64_t)opt_blocks(n) * sizeof(double)); }

// ---- update ------------------------------------------------------------------------------------------------------------------
// The update walks "units": for each of the two segments (weights, biases) first its float4 units (all of them when the
// segment's four arrays are 16-byte aligned, else none), then its scalar tail.  One thread per unit.
struct OptUnits { int64_t wVec, wTail, bVec, bTail; };
MRIRT_HD OptUnits opt_units(int64_t nw, int64_t nb, bool wAligned, bool bAligned) {
    OptUnits u;
    u.wVec = wAligned ? nw / 4 : 0; u.wTail = nw - 4 * u.wVec;
    u.bVec = bAligned ? nb / 4 : 0; u.bTail = nb - 4 * u.bVec;
    return u;
}
MRIRT_HD int64_t opt_unit_count(const OptUnits& u) { return u.wVec + u.wTail + u.bVec + u.bTail; }
// unit i -> segment (0 weights, 1 biases), first element inside the segment, width (4 or 1)
MRIRT_HD void opt_unit(const OptUnits& u, int64_t i, uint32_t& seg, int64_t& first, uint32_t& width) {
    if (i < u.wVec) { seg = 0; first = 4 * i; width = 4; return; }
    i -= u.wVec;
    if (i < u.wTail) { seg = 0; first = 4 * u.wVec + i; width = 1; return; }
    i -= u.wTail;
    if (i < u.bVec) { seg = 1; first = 4 * i; width = 4; return; }
    i -= u.bVec;
    seg = 1; first = 4 * u.bVec + i; width = 1;
}

// ---- scratch of mrirt_inr_train_run -------------------------------------------------------------------------------------------
// [one step's scratch (train_layout)][coords n x 3][feats n x M][labels n][logits n x C][dlogits n x C][gw][gb][gnorm: 2 doubles]
// [norm partial sums]; every region 256-B aligned
struct RunLayout {
    uint64_t nw, nb;
    uint64_t stepBytes, offCoords, offFeats, offLabels, offLogits, offDlogits, offGw, offGb, offGnorm, offOpt, optBytes, bytes;
};
MRIRT_HD RunLayout run_layout(const TrainLayout& L, int64_t n, uint32_t numMods) {
    RunLayout R;
    const uint32_t last = L.numLayers - 1;
    R.nw = (uint64_t)L.wOff[last] + (uint64_t)L.in[last] * L.out[last];
    R.nb = (uint64_t)L.bOff[last] + L.out[last];
    R.stepBytes = L.bytes;
    R.offCoords = tr_align(L.bytes);
    R.offFeats = R.offCoords + tr_align((uint64_t)n * 3 * sizeof(float));
    R.offLabels = R.offFeats + tr_align((uint64_t)n * numMods * sizeof(float));
    R.offLogits = R.offLabels + tr_align((uint64_t)n * sizeof(int32_t));
    R.offDlogits = R.offLogits + tr_align((uint64_t)n * L.outDim * sizeof(float));
    R.offGw = R.offDlogits + tr_align((uint64_t)n * L.outDim * sizeof(float));
    R.offGb = R.offGw + tr_align(R.nw * sizeof(float));
    R.offGnorm = R.offGb + tr_align(R.nb * sizeof(float));
    R.offOpt = R.offGnorm + tr_align(2 * sizeof(double));
    R.optBytes = opt_scratch_bytes((int64_t)(R.nw + R.nb));
    R.bytes = R.offOpt + R.optBytes;
    return R;
}

}  // namespace mrirt
