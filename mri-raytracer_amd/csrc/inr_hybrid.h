// The hybrid, uncertainty-guided sampler of the reference's notebooks/improved.ipynb (cell 9) and its coordinate noise (cell 12)
// (csrc/inr_hybrid.hip): the chunking of the per-class voxel index, the order-preserving key and the
// per-thread steps of the exact selection, the unit normals and the row a micro-batch point reads, written once for the device
// kernels and for the host (tests/native/hybrid_harness.hip walks them under AddressSanitizer + UBSan over buffers of exactly
// the real sizes).
#pragma once
#include <math.h>
#include <stdint.h>

#include "inr_lossx.h"

namespace mrirt {

// ---- class index: mrirt_inr_tumour_index's compaction with C bins ------------------------------------------------------------------
// The chunks, the threads and a thread's voxels are the tumour index's (tum_chunks, tum_first, kTumThreads, kTumPerThread).
// uint32: [ncases][tum_chunks][C] voxels per (case, chunk, class), scanned in place over the chunks of a (case, class) to the
// exclusive prefix inside that list
MRIRT_HD uint64_t cls_scratch_bytes(uint32_t ncases, uint64_t hwd, uint32_t C) {
    return tr_align((uint64_t)ncases * tum_chunks(hwd) * C * sizeof(uint32_t));
}
MRIRT_HD uint64_t cls_chunk_slot(uint32_t cs, uint32_t chunk, uint32_t k, uint32_t chunksPerCase, uint32_t C) {
    return ((uint64_t)cs * chunksPerCase + chunk) * C + k;
}
// a label is in a list when it lies in 0..C-1
MRIRT_HD bool cls_in(int16_t label, uint32_t C) { return label >= 0 && (uint32_t)label < C; }
// the list of (class k, case cs) is index[offsets[cls_list(k, cs, ncases)] .. offsets[cls_list(k, cs, ncases) + 1])
MRIRT_HD uint32_t cls_list(uint32_t k, uint32_t cs, uint32_t ncases) { return k * ncases + cs; }
// the case whose list of class k holds `slot`: the last cs with offsets[cls_list(k, cs)] <= slot (empty lists share their
// start with the next one and are passed over).  first_k <= slot < first_k + total_k.
MRIRT_HD uint32_t cls_case_of(const int64_t* offsets, uint32_t k, uint32_t ncases, int64_t slot) {
    uint32_t lo = 0, hi = ncases;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offsets[cls_list(k, mid, ncases)] <= slot) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- exact selection of the k largest ------------------------------------------------------------------------------------------------
constexpr uint32_t kSelThreads = 1024;
constexpr uint32_t kSelMaxN = 65536;
constexpr uint32_t kSelBins = 256;            // one key byte per pass, most significant first
constexpr uint32_t kSelPasses = 4;

// order-preserving key: negative values ~bits, others bits | sign, so that -0 < +0; every NaN is the one key above +inf
MRIRT_HD uint32_t sel_key_bits(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
MRIRT_HD uint32_t sel_key(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    return sel_key_bits(c.u);
}
MRIRT_HD uint32_t sel_shift(uint32_t pass) { return 8u * (kSelPasses - 1u - pass); }
// the key bytes above pass `pass`'s byte
MRIRT_HD uint32_t sel_mask(uint32_t pass) { return pass == 0 ? 0u : ~(0xFFFFFFFFu >> (8u * pass)); }
// thread t owns the consecutive elements sel_first(t, n) .. sel_first(t + 1, n) - 1 (none past n): ascending (thread, element)
// is ascending index order
MRIRT_HD uint32_t sel_per_thread(uint32_t n) { return (n + kSelThreads - 1) / kSelThreads; }
MRIRT_HD uint32_t sel_first(uint32_t t, uint32_t n) {
    const uint64_t f = (uint64_t)t * sel_per_thread(n);
    return f < n ? (uint32_t)f : n;
}
// thread d < kSelBins after pass `pass`'s histogram: `above` = the keys of the still-open set with a larger byte.  Bin d holds
// the need-th largest when above < need <= above + hist[d]; exactly one d does.
MRIRT_HD uint32_t sel_above(const uint32_t* hist, uint32_t d) {
    uint32_t above = 0;
    for (uint32_t b = d + 1; b < kSelBins; ++b) above += hist[b];
    return above;
}
MRIRT_HD bool sel_is_digit(uint32_t above, uint32_t mine, uint32_t need) { return above < need && need <= above + mine; }
// Of the keys equal to the threshold, the `need` with the highest indices are taken: the one with `rank` equal keys before it
// (in index order) is taken when rank >= equal - need.
MRIRT_HD bool sel_takes(uint32_t key, uint32_t threshold, uint32_t rank, uint32_t equal, uint32_t need) {
    return key > threshold || (key == threshold && rank >= equal - need);
}

// ---- unit normals ------------------------------------------------------------------------------------------------------------------
constexpr double kTwoPi = 6.283185307179586;
constexpr double kTwoM32 = 2.3283064365386963e-10;       // 2^-32
// Box-Muller in fp64 from two words: R = sqrt(-2 log((ra + 1) 2^-32)), angle 2 pi rb 2^-32
MRIRT_HD double nrm_radius(uint32_t ra) { return sqrt(-2.0 * log(((double)ra + 1.0) * kTwoM32)); }
MRIRT_HD double nrm_angle(uint32_t rb) { return kTwoPi * ((double)rb * kTwoM32); }
struct Normal3 { float x, y, z; };
MRIRT_HD Normal3 nrm_of_words(const uint32_t r[4]) {
    const double R = nrm_radius(r[0]), a = nrm_angle(r[1]);
    Normal3 z;
    z.x = (float)(R * cos(a));
    z.y = (float)(R * sin(a));
    z.z = (float)(nrm_radius(r[2]) * cos(nrm_angle(r[3])));
    return z;
}
// the Philox words of point i at counter word 3 = `stream`: 0 the batch's own draw (mix_words), 1 the candidates, 2 the normals
MRIRT_HD MixDraw hyb_words(uint64_t seed, uint64_t batch, uint32_t i, uint32_t stream) {
    MixDraw d;
    d.r[0] = i; d.r[1] = (uint32_t)batch; d.r[2] = (uint32_t)(batch >> 32); d.r[3] = stream;
    philox4x32_10(d.r, (uint32_t)seed, (uint32_t)(seed >> 32));
    return d;
}
MRIRT_HD Normal3 nrm_point(uint64_t seed, uint64_t batch, uint32_t i) {
    const MixDraw d = hyb_words(seed, batch, i, 2u);
    return nrm_of_words(d.r);
}

// ---- hybrid micro-batch ------------------------------------------------------------------------------------------------------------
// floor(a b / 2^64)
MRIRT_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
    const uint64_t al = a & 0xFFFFFFFFull, ah = a >> 32, bl = b & 0xFFFFFFFFull, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (lh & 0xFFFFFFFFull) + (hl & 0xFFFFFFFFull);
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}
// slot of a balanced draw: first_k + floor(((r0 << 32) | r1) total_k / 2^64), total_k > 0
MRIRT_HD int64_t hyb_slot(uint32_t r0, uint32_t r1, int64_t first, int64_t total) {
    return first + (int64_t)mulhi64(((uint64_t)r0 << 32) | r1, (uint64_t)total);
}
// Row i of micro-batch `batch`: candidate picks[i] below U, a voxel of class (i - U) / P below U + C P, else sample_point's.
// index / offsets may be NULL when P == 0, picks when U == 0.
MRIRT_HD SamplePoint hyb_row(uint64_t seed, uint64_t batch, uint32_t i, int64_t U, int64_t P, uint32_t C, const uint32_t* picks,
                             const uint32_t* index, const int64_t* offsets, uint32_t ncases, uint32_t H, uint32_t W, uint32_t D, int64_t hwd) {
    if ((int64_t)i < U) return mix_uniform(hyb_words(seed, batch, picks[i], 1u), ncases, H, W, D);
    const MixDraw dr = mix_words(seed, batch, i);
    SamplePoint p = mix_uniform(dr, ncases, H, W, D);
    if ((int64_t)i < U + (int64_t)C * P) {
        const uint32_t k = (uint32_t)(((int64_t)i - U) / P);
        const int64_t first = offsets[cls_list(k, 0, ncases)], total = offsets[cls_list(k + 1, 0, ncases)] - first;
        if (total > 0) {
            const int64_t slot = hyb_slot(dr.r[0], dr.r[1], first, total);
            const uint32_t v = index[slot];
            if ((int64_t)v < hwd) {                                  // a foreign index cannot point outside the volume
                p.cs = cls_case_of(offsets, k, ncases, slot);
                tum_decode(v, W, D, p.x, p.y, p.z);
            }
        }
    }
    return p;
}
// coordinate noise: c + sigma z, the product and the sum each rounded to fp32
MRIRT_HD float hyb_noise(float c, float sigma, float z) {
    const float s = sigma * z;
    return c + s;
}

}  // namespace mrirt
