// Fused forward of the coordinate-injection INR (csrc/inr_inject_fused.hip): the LDS layout, the index
// arithmetic of the weight staging, of a wave's A-buffers and of the MFMA fragments, and the per-element feature code,
// written once for the kernel and for the host (tests/native/inject_fused_harness.hip walks it under AddressSanitizer + UBSan
// over heap buffers of exactly the sizes the layout states).
//
// A workgroup of kFusedWaves waves holds the whole network in LDS: every W_l k-major ([k][pitch], k padded to 4 with zero
// rows, out padded to 16 with zero columns), every bias padded to 16, and B.  A wave owns 16 rows of a 64-row tile and two
// buffers of its own, [k][16 rows] each: layer l reads its A operand [h | coords | mods | 0 ..] from buffer l & 1 and writes
// its activation into the other one, where the wave then appends the next layer's injected columns and its zero padding.
#pragma once
#include <stdint.h>

#include "inr_inject.h"
#include "siren_sincos.h"

namespace mrirt {

constexpr uint32_t kFusedWaves = 4, kFusedThreads = 64 * kFusedWaves;
constexpr uint32_t kFusedWaveRows = 16, kFusedTileRows = kFusedWaveRows * kFusedWaves;
constexpr uint32_t kFusedGroup = 4;                      // column tiles whose accumulators are in flight together
constexpr uint32_t kFusedExt = (3 + kInjMaxMods + 3) / 4;   // injected values a lane keeps: element (lane >> 4) + 4 i of [coords | mods]
constexpr uint64_t kFusedLdsBudget = 160u * 1024u;       // all of a CU's LDS: one workgroup per CU

// One feature pair of a point, exactly as the chain computes it (inj_features_kernel calls this): the unfused fp32
// expression for c01, p and the angle, then the STRICT sine / cosine.
MRIRT_HD void inj_feature(float cx, float cy, float cz, float b0, float b1, float b2, float& sn, float& cs) {
    const float ux = (cx + 1.0f) * 0.5f, uy = (cy + 1.0f) * 0.5f, uz = (cz + 1.0f) * 0.5f;
    const float p = ((ux * b0) + (uy * b1)) + (uz * b2);
    const float ang = 6.2831855f * p;
    siren_sincos(ang, sn, cs);
}

// Offsets in floats from the start of the dynamic LDS; every region starts on a multiple of 4 floats (16 bytes).
struct InjFusedLayout {
    uint32_t kPad[kInjMaxLayers], outPad[kInjMaxLayers], pitch[kInjMaxLayers];
    uint32_t wOff[kInjMaxLayers], bOff[kInjMaxLayers];
    uint32_t offB;
    uint32_t offWave, waveFloats, bufFloats[2];          // wave v: buffer 0 at offWave + v waveFloats, buffer 1 behind it
    uint64_t bytes;                                      // all of it; the fused path takes the shape iff bytes <= kFusedLdsBudget
};

MRIRT_HD uint32_t fused_round(uint32_t x, uint32_t to) { return (x + to - 1) / to * to; }

// The pitch of a staged W_l: a B fragment reads rows k, k + 1 (lanes 0 .. 31) and k + 2, k + 3 of 16 neighbouring columns
// with ds_read_b32, whose bank is (address / 4) mod 32 within a 32-lane half: a pitch of 16 mod 32 puts the half's two rows
// on disjoint banks.
MRIRT_HD uint32_t fused_pitch(uint32_t outPad) { return outPad % 32u == 16u ? outPad : outPad + 16u; }

MRIRT_HD InjFusedLayout inj_fused_layout(const InjNet& N) {
    InjFusedLayout Y = {};
    uint32_t at = 0;
    for (uint32_t l = 0; l < N.numLayers; ++l) {
        Y.kPad[l] = fused_round(N.in[l], 4);
        Y.outPad[l] = fused_round(N.out[l], 16);
        Y.pitch[l] = fused_pitch(Y.outPad[l]);
        Y.wOff[l] = at;
        at += Y.kPad[l] * Y.pitch[l];
    }
    for (uint32_t l = 0; l < N.numLayers; ++l) {
        Y.bOff[l] = at;
        at += Y.outPad[l];
    }
    Y.offB = at;
    at += fused_round((N.F / 2) * 3, 4);
    // buffer l & 1 holds layer l's A operand, kPad[l] x 16; the head's logits ([16][16]) go where layer L's operand would
    for (uint32_t l = 0; l <= N.numLayers; ++l) {
        const uint32_t need = (l < N.numLayers ? Y.kPad[l] : 16u) * kFusedWaveRows;
        if (need > Y.bufFloats[l & 1u]) Y.bufFloats[l & 1u] = need;
    }
    Y.offWave = at;
    Y.waveFloats = Y.bufFloats[0] + Y.bufFloats[1];
    Y.bytes = ((uint64_t)Y.offWave + (uint64_t)kFusedWaves * Y.waveFloats) * sizeof(float);
    return Y;
}

MRIRT_HD bool inj_fused_fits(const InjFusedLayout& Y) { return Y.bytes <= kFusedLdsBudget; }

// ---- staging ------------------------------------------------------------------------------------------------------------------
// Element e < kPad[l] pitch[l] of the staged W_l is row k = e / pitch, column c = e % pitch: W_l[k][c] (w[wOff[l] + k out + c])
// inside the matrix, 0 in the padding.  Returns the offset into w, or -1 for a zero.
MRIRT_HD int64_t fused_stage_src(const InjNet& N, const InjFusedLayout& Y, uint32_t l, uint32_t e) {
    const uint32_t k = e / Y.pitch[l], c = e - k * Y.pitch[l];
    return (k < N.in[l] && c < N.out[l]) ? (int64_t)N.wOff[l] + (int64_t)k * N.out[l] + c : -1;
}

// ---- a wave's buffers ---------------------------------------------------------------------------------------------------------
// element (k, row) of a buffer
MRIRT_HD uint32_t fused_a_index(uint32_t k, uint32_t row) { return k * kFusedWaveRows + row; }
// Lane `lane` keeps element e = (lane >> 4) + 4 i of its row's [coords | mods]; where layer l's buffer takes it: the k of
// that element, or -1 when layer l does not inject it (or the element does not exist).
MRIRT_HD int fused_ext_k(const InjNet& N, uint32_t l, uint32_t e) {
    if (e < 3u) return N.splitM[l] != N.split[l] ? (int)(N.split[l] + e) : -1;
    const uint32_t m = e - 3u;
    return (m < N.M && N.in[l] != N.splitM[l]) ? (int)(N.splitM[l] + m) : -1;
}
// MFMA step s (k = 4 s .. 4 s + 3): the A element a lane reads from its wave's buffer and the B element it reads from the
// staged W_l for column tile j
MRIRT_HD uint32_t fused_frag_a(uint32_t s, uint32_t lane) { return fused_a_index(4u * s + (lane >> 4), lane & 15u); }
MRIRT_HD uint32_t fused_frag_b(const InjFusedLayout& Y, uint32_t l, uint32_t s, uint32_t j, uint32_t lane) {
    return Y.wOff[l] + (4u * s + (lane >> 4)) * Y.pitch[l] + 16u * j + (lane & 15u);
}
// the epilogue: a lane's four accumulator registers of column tile j are rows 4 (lane >> 4) .. + 3 of column 16 j + (lane & 15),
// one 16-byte store at this element of the output buffer (only for columns < out)
MRIRT_HD uint32_t fused_epi_index(uint32_t j, uint32_t lane) { return fused_a_index(16u * j + (lane & 15u), 4u * (lane >> 4)); }

// argmax as inj_argmax, over z[0], z[stride], ..: the first index of the maximum, a NaN counting as the maximum
MRIRT_HD uint32_t inj_argmax_strided(const float* z, uint32_t C, uint32_t stride) {
    uint32_t best = 0;
    for (uint32_t k = 1; k < C; ++k)
        if (!(z[best * stride] != z[best * stride]) && (z[k * stride] > z[best * stride] || z[k * stride] != z[k * stride])) best = k;
    return best;
}

// rows this call processes: count_dev's word clamped to n_max, or n_max without one
MRIRT_HD uint32_t fused_rows(uint32_t nMax, bool haveCount, uint32_t count) { return haveCount ? (count < nMax ? count : nMax) : nMax; }

}  // namespace mrirt
