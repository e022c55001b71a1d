// Index arithmetic of the case preparation kernels (csrc/prep.hip), as plain C++ shared with the host harness
// (tests/native/prep_harness.hip): the order-preserving key of an fp32 value and its inverse, the fp32 rank of a
// percentile, the choice of a histogram bin for a rank, the reflected index of the Gaussian filter, the tile decomposition
// of its line passes and the scratch layout of the percentile window.
#pragma once
#include <string.h>

#include "mrirt_device.h"

namespace mrirt {

// --- the percentile window --------------------------------------------------------------------------------------------
constexpr uint32_t kPrepThreads = 256;
constexpr uint32_t kPrepHistThreads = 1024;                     // the histogram workgroup: 16 waves share one LDS histogram
constexpr uint32_t kPrepItems = 4;                              // elements per thread before a block takes a second stride
constexpr uint32_t kPrepBlockElems = kPrepHistThreads * kPrepItems; // 4096
constexpr uint32_t kPrepMaxBlocks = 512;                        // per-block partial histograms kept in the scratch
constexpr uint32_t kPrepRanks = 4;                              // k1, k1 + 1, k2, k2 + 1
constexpr uint32_t kPrepBins = 256, kPrepDigitBits = 8, kPrepPasses = 4;
constexpr uint32_t kPrepNanKey = 0xFFFFFFFFu;
constexpr int64_t kPrepMaxN = 0x7FFFFFFF;

MRIRT_HD uint32_t prep_f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
MRIRT_HD float prep_u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// uint32 key whose unsigned order is the order NumPy sorts fp32 in: negatives below positives, -0.0 and +0.0 one key,
// every NaN the largest key
MRIRT_HD uint32_t prep_key(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return kPrepNanKey;
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
// the fp32 bits of a key (+0.0 for the zero key, the quiet NaN 0x7FC00000 for the NaN key)
MRIRT_HD uint32_t prep_key_inverse(uint32_t key) {
    if (key == kPrepNanKey) return 0x7FC00000u;
    return (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
}

// np.percentile's (linear) index for n elements, evaluated in fp32 as NumPy does for fp32 data: k = floor(v) and
// g = v - k of v = f32(n - 1) * (f32(q) / 100).  k is clamped to n - 1 (f32(n - 1) may round up past it beyond 2^24).
MRIRT_HD void prep_rank(int64_t n, float q, uint32_t* k, float* g) {
    const float qq = q / 100.0f;
    const float v = (float)(n - 1) * qq;
    int64_t kk = (int64_t)v;                                   // v >= 0: truncation is floor
    float gg = v - (float)kk;
    if (kk > n - 1) { kk = n - 1; gg = 0.0f; }
    *k = (uint32_t)kk;
    *g = gg;
}

MRIRT_HD uint32_t prep_hist_blocks(int64_t n) {
    const int64_t b = (n + kPrepBlockElems - 1) / kPrepBlockElems;
    return (uint32_t)(b < 1 ? 1 : (b > kPrepMaxBlocks ? kPrepMaxBlocks : b));
}

// the bin of `hist` (kPrepBins counts) holding the element of 0-based rank `rank` among the counted ones, and the rank
// that remains inside that bin.  A rank past the total (cannot happen for a consistent histogram) lands in the last bin.
MRIRT_HD uint32_t prep_select_bin(const uint32_t* hist, uint32_t rank, uint32_t* remaining) {
    uint32_t before = 0;
    for (uint32_t b = 0; b < kPrepBins; ++b) {
        const uint32_t c = hist[b];
        if (rank - before < c || b == kPrepBins - 1) { *remaining = rank - before; return b; }
        before += c;
    }
    *remaining = 0;
    return kPrepBins - 1;
}

// the radix-select state kept in the scratch between launches
struct PrepSelectState {
    uint32_t prefix[kPrepRanks];        // the digits chosen so far (the whole key after the last pass)
    uint32_t rem[kPrepRanks];           // rank among the elements that share the prefix
    uint32_t slot[kPrepRanks];          // histogram a rank reads: ranks with one prefix share a slot
    uint32_t nslots;
    uint32_t minKey, maxKey;
    uint32_t pad;
};

// slot[r] = the first rank with the same prefix, renumbered densely; returns the number of distinct prefixes
MRIRT_HD uint32_t prep_assign_slots(const uint32_t* prefix, uint32_t* slot) {
    uint32_t n = 0;
    for (uint32_t r = 0; r < kPrepRanks; ++r) {
        uint32_t s = n;
        for (uint32_t q = 0; q < r; ++q)
            if (prefix[q] == prefix[r]) { s = slot[q]; break; }
        slot[r] = s;
        if (s == n) ++n;
    }
    return n;
}

// scratch of mrirt_prep_window: [ state | per-block {min, max} keys | totals | per-block histograms ], each part 256-B aligned
struct PrepWindowPlan { uint32_t blocks; int64_t state, minmax, totals, partial, total; };
MRIRT_HD int64_t prep_align256(int64_t x) { return (x + 255) / 256 * 256; }
MRIRT_HD bool prep_window_plan(int64_t n, PrepWindowPlan* p) {
    if (n < 1 || n > kPrepMaxN) return false;
    p->blocks = prep_hist_blocks(n);
    p->state = 0;
    p->minmax = prep_align256((int64_t)sizeof(PrepSelectState));
    p->totals = p->minmax + prep_align256(8ll * p->blocks);
    p->partial = p->totals + prep_align256(4ll * kPrepRanks * kPrepBins);
    p->total = p->partial + prep_align256(4ll * kPrepRanks * kPrepBins * p->blocks);
    return true;
}

// --- the z-score ------------------------------------------------------------------------------------------------------
constexpr uint32_t kPrepZItems = 8, kPrepZMaxBlocks = 256;
MRIRT_HD uint32_t prep_zscore_blocks(int64_t n) {
    const int64_t per = (int64_t)kPrepThreads * kPrepZItems;
    const int64_t b = (n + per - 1) / per;
    return (uint32_t)(b < 1 ? 1 : (b > kPrepZMaxBlocks ? kPrepZMaxBlocks : b));
}
// scratch of mrirt_prep_zscore_stats: per modality 4 doubles of state, then blocks x { fp64 sum, uint64 count }
MRIRT_HD int64_t prep_zscore_scratch(int64_t n, uint32_t M) {
    if (n < 1 || n > kPrepMaxN || M < 1 || M > 64) return 0;
    return prep_align256(32ll * M) + prep_align256(16ll * M * prep_zscore_blocks(n));
}

// --- the Gaussian filter ----------------------------------------------------------------------------------------------
constexpr int kPrepMaxRadius = 16;

// scipy.ndimage's `reflect` (d c b a | a b c d | d c b a): valid for any i, repeats when the axis is shorter than the radius
MRIRT_HD int64_t prep_reflect(int64_t i, int64_t n) {
    const int64_t p = 2 * n;
    int64_t m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// A line pass sees the volume as [outer][len][inner] (inner = the product of the extents behind the axis) and cuts it into
// tiles of TO x TL x TI outputs; a tile stages TO x (TL + 2 r) x TI inputs.
struct PrepLineGeom { int64_t outer, len, inner, tilesO, tilesL, tilesI, tiles; };
MRIRT_HD PrepLineGeom prep_line_geom(const uint32_t dims[3], int axis, uint32_t TO, uint32_t TL, uint32_t TI) {
    PrepLineGeom g;
    g.outer = 1; g.inner = 1;
    for (int k = 0; k < axis; ++k) g.outer *= dims[k];
    for (int k = axis + 1; k < 3; ++k) g.inner *= dims[k];
    g.len = dims[axis];
    g.tilesO = (g.outer + TO - 1) / TO;
    g.tilesL = (g.len + TL - 1) / TL;
    g.tilesI = (g.inner + TI - 1) / TI;
    g.tiles = g.tilesO * g.tilesL * g.tilesI;
    return g;
}
// origin (o0, l0, i0) of tile t, the inner tiles fastest
MRIRT_HD void prep_tile_origin(const PrepLineGeom& g, int64_t t, uint32_t TO, uint32_t TL, uint32_t TI, int64_t* o0, int64_t* l0, int64_t* i0) {
    *i0 = (t % g.tilesI) * TI;
    t /= g.tilesI;
    *l0 = (t % g.tilesL) * TL;
    *o0 = (t / g.tilesL) * TO;
}
// element e of a tile's staged block, the inner index fastest, then the line position (halo included), then the outer one
MRIRT_HD void prep_stage_coords(uint32_t e, uint32_t rows, uint32_t TI, uint32_t* o, uint32_t* l, uint32_t* i) {
    *i = e % TI;
    e /= TI;
    *l = e % rows;
    *o = e / rows;
}

}  // namespace mrirt
