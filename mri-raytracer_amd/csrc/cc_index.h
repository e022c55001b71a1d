// Connected components of a label volume, the per-thread text: the inside rule, the forward neighbours of a connectivity, the
// union-find whose links only ever decrease, what a thread of each stage of mrirt_cc_label / mrirt_cc_sizes / mrirt_cc_filter /
// mrirt_slice_counts does, and the scratch layout — written once for the device kernels (csrc/components.hip) and for the host
// (tests/native/cc_harness.hip runs it under AddressSanitizer + UBSan with every buffer exactly its size long).
//
// Definition ("Connected components of label volumes"): voxel v of an (n0, n1, n2) volume, linear index
// (i0 n1 + i1) n2 + i2, is inside iff 0 <= labels[v] < 32 and bit labels[v] of classMask is set; two inside voxels are adjacent
// iff they differ by at most 1 on every axis and on at most `connectivity` axes; a component's root is its smallest linear
// index and components are numbered 1 .. N by increasing root.
//
// The parent array is the output volume: -1 on an outside voxel, otherwise the linear index of an inside voxel of the same
// component that is NOT LARGER than the voxel's own (a root holds itself).  Every write to it keeps that, so every walk
// along parents strictly descends.
#pragma once
#include "mrirt_device.h"

namespace mrirt {

constexpr uint32_t kCcThreads = 256;                   // threads of every workgroup of csrc/components.hip
constexpr uint32_t kCcItems = 4;                       // consecutive elements a thread of a count / number workgroup owns
constexpr uint32_t kCcChunk = kCcThreads * kCcItems;   // elements a workgroup counts, scans or rewrites
constexpr uint32_t kCcT0 = 8, kCcT1 = 8, kCcT2 = 32;   // the label tile, in voxels
constexpr uint32_t kCcTileVox = kCcT0 * kCcT1 * kCcT2; // 2048: 8 KiB of int32 parents in LDS
constexpr uint32_t kCcPerThread = kCcTileVox / kCcThreads;      // thread t owns the voxels (j, t / 32, t % 32), j < 8
constexpr uint32_t kCcMaxLevels = 3;                   // 1024^3 > 2^31 - 1: three levels of chunk sums always end in one chunk
constexpr uint64_t kCcMaxVoxels = 0x7FFFFFFFull;
constexpr uint32_t kCcMaxGrid = 1u << 20;              // workgroups of a tile launch (more tiles: a workgroup takes several in turn)
constexpr uint32_t kCcSliceZ = 32, kCcSliceRows = 256; // slice counts: a workgroup takes 32 indices of the last axis x 256 rows
constexpr uint32_t kCcSizeSlots = 256, kCcSizeChunks = 4;   // sizes: a workgroup's LDS table, the chunks it takes
constexpr uint32_t kCcFilterGrid = 1024;               // workgroups of the filter launch (each finds the largest component itself)

static_assert(kCcT1 * kCcT2 == kCcThreads && kCcPerThread == kCcT0, "thread t owns one column of the tile");
static_assert(kCcThreads % kCcSliceZ == 0 && kCcSliceRows % (kCcThreads / kCcSliceZ) == 0, "slice-count workgroup shape");

struct CcGeom {
    uint32_t n[3];        // voxels per axis
    uint32_t total;       // n0 n1 n2 <= 2^31 - 1
    uint32_t tiles[3];    // label tiles per axis
    uint32_t numTiles;
};

MRIRT_HD bool cc_inside(int32_t label, uint32_t classMask) { return label >= 0 && label < 32 && ((classMask >> label) & 1u) != 0u; }

MRIRT_HD uint32_t cc_linear(const CcGeom& g, uint32_t i0, uint32_t i1, uint32_t i2) { return (i0 * g.n[1] + i1) * g.n[2] + i2; }

MRIRT_HD void cc_tile_origin(const CcGeom& g, uint32_t tileId, uint32_t o[3]) {
    o[2] = (tileId % g.tiles[2]) * kCcT2;
    const uint32_t r = tileId / g.tiles[2];
    o[1] = (r % g.tiles[1]) * kCcT1;
    o[0] = (r / g.tiles[1]) * kCcT0;
}

// The forward neighbours: code k in 14 .. 26 is the offset d = (k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1), the 13 offsets of
// {-1, 0, 1}^3 that are lexicographically positive, i.e. whose neighbour has the LARGER linear index.  Under `connectivity`
// those with at most that many non-zero components count: 3, 9 or 13 of them.  Every adjacent pair is one voxel and one of
// its forward neighbours, exactly once.
constexpr uint32_t kCcFirstForward = 14, kCcEndForward = 27;
MRIRT_HD bool cc_forward_offset(uint32_t k, uint32_t connectivity, int32_t d[3]) {
    d[0] = (int32_t)(k / 9u) - 1;
    d[1] = (int32_t)(k / 3u % 3u) - 1;
    d[2] = (int32_t)(k % 3u) - 1;
    const uint32_t axes = (d[0] != 0 ? 1u : 0u) + (d[1] != 0 ? 1u : 0u) + (d[2] != 0 ? 1u : 0u);
    return axes <= connectivity;
}

// --- memory: on the device every read and update of a parent goes through an atomic of the scope the launch needs ---------
enum CcScope { kCcLds = 0, kCcAgent = 1, kCcPlain = 2 };

template <CcScope S>
MRIRT_HD int32_t cc_load(const int32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (S == kCcAgent) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (S == kCcLds) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
    return *p;
}

// *p = min(*p, v); returns what *p held
template <CcScope S>
MRIRT_HD int32_t cc_atomic_min(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (S == kCcLds) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    const int32_t old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

MRIRT_HD void cc_atomic_add(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p += v;
#endif
}

// --- union-find ----------------------------------------------------------------------------------------------------------
// The voxel x's walk along parents ends at.  A value read may be older than the newest (another XCD's L2, a write in flight):
// it is still an ancestor, so the walk ends at an ancestor; what is DECIDED from it is the caller's business.
template <CcScope S>
MRIRT_HD int32_t cc_find(const int32_t* parent, int32_t x) {
    // ends: x strictly decreases on every trip (the loop goes on only while 0 <= p < x) and is never negative
    for (;;) {
        const int32_t p = cc_load<S>(parent + x);
        if (p < 0 || p >= x) return x;
        x = p;
    }
}

// Unites the components of the inside voxels a and b.  A link is only ever made from a root to a smaller index, by an
// atomic min on the root's own entry, and counts as made only when the atomic RETURNED the root itself.  When it returns
// something else (old < a: a had been linked meanwhile) the entry now holds min(old, b): a's tie to the other of the two is
// gone from the array, and this thread carries it on as the pair (old, b).  "Already the same root" is decided from two
// walks that ended at the same voxel: both are ancestors, so a and b are — or, where a tie is still carried by another
// thread, will be — in one set.
template <CcScope S>
MRIRT_HD void cc_union(int32_t* parent, int32_t a, int32_t b) {
    // ends: max(a, b) strictly decreases on every trip — the larger is replaced by a value below it (old < a, then a walk
    // downwards), the smaller only walks downwards — and is never negative
    for (;;) {
        a = cc_find<S>(parent, a);
        b = cc_find<S>(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = cc_atomic_min<S>(parent + a, b);
        if (old == a) return;                            // a was a root and now points at b
        if (old < 0) return;                             // never on a parent array (an inside voxel's entry is >= 0)
        a = old;
    }
}

// --- label, local pass: one workgroup per tile, the tile's parents in LDS as LOCAL indices (l0 T1 + l1) T2 + l2 -----------
// (local and linear indices order a tile's voxels the same way, so a tile component's smallest local index is its smallest
// linear index)
MRIRT_HD void cc_local_coords(uint32_t l, uint32_t c[3]) {
    c[2] = l % kCcT2;
    c[1] = l / kCcT2 % kCcT1;
    c[0] = l / (kCcT1 * kCcT2);
}

// thread t: its voxels' entries, themselves when inside, -1 when outside the class set or the volume
MRIRT_HD void cc_tile_load(const CcGeom& g, const int16_t* labels, uint32_t classMask, const uint32_t o[3], int32_t* tile, uint32_t t) {
    for (uint32_t j = 0; j < kCcPerThread; ++j) {
        const uint32_t l = j * kCcThreads + t;
        uint32_t c[3];
        cc_local_coords(l, c);
        const uint32_t i0 = o[0] + c[0], i1 = o[1] + c[1], i2 = o[2] + c[2];
        bool in = false;
        if (i0 < g.n[0] && i1 < g.n[1] && i2 < g.n[2]) in = cc_inside((int32_t)labels[cc_linear(g, i0, i1, i2)], classMask);
        tile[l] = in ? (int32_t)l : -1;
    }
}

// thread t (after every thread's cc_tile_load): unites each of its inside voxels with its inside forward neighbours in the tile
MRIRT_HD void cc_tile_link(uint32_t connectivity, int32_t* tile, uint32_t t) {
    for (uint32_t j = 0; j < kCcPerThread; ++j) {
        const uint32_t l = j * kCcThreads + t;
        if (cc_load<kCcLds>(tile + l) < 0) continue;     // the sign of an entry never changes
        uint32_t c[3];
        cc_local_coords(l, c);
        for (uint32_t k = kCcFirstForward; k < kCcEndForward; ++k) {
            int32_t d[3];
            if (!cc_forward_offset(k, connectivity, d)) continue;
            const uint32_t m0 = c[0] + (uint32_t)d[0], m1 = c[1] + (uint32_t)d[1], m2 = c[2] + (uint32_t)d[2];   // -1 wraps to 2^32 - 1
            if (m0 >= kCcT0 || m1 >= kCcT1 || m2 >= kCcT2) continue;
            const uint32_t m = (m0 * kCcT1 + m1) * kCcT2 + m2;
            if (cc_load<kCcLds>(tile + m) >= 0) cc_union<kCcLds>(tile, (int32_t)l, (int32_t)m);
        }
    }
}

// thread t (after every thread's cc_tile_link): the local roots of its voxels (-1: outside)
MRIRT_HD void cc_tile_roots(const int32_t* tile, uint32_t t, int32_t root[kCcPerThread]) {
    for (uint32_t j = 0; j < kCcPerThread; ++j) {
        const uint32_t l = j * kCcThreads + t;
        root[j] = cc_load<kCcLds>(tile + l) < 0 ? -1 : cc_find<kCcLds>(tile, (int32_t)l);
    }
}

// thread t: the parent array's entries of its voxels, the local root as a linear index
MRIRT_HD void cc_tile_store(const CcGeom& g, const uint32_t o[3], const int32_t root[kCcPerThread], int32_t* parent, uint32_t t) {
    for (uint32_t j = 0; j < kCcPerThread; ++j) {
        uint32_t c[3];
        cc_local_coords(j * kCcThreads + t, c);
        const uint32_t i0 = o[0] + c[0], i1 = o[1] + c[1], i2 = o[2] + c[2];
        if (i0 >= g.n[0] || i1 >= g.n[1] || i2 >= g.n[2]) continue;
        int32_t p = -1;
        if (root[j] >= 0) {
            uint32_t r[3];
            cc_local_coords((uint32_t)root[j], r);
            p = (int32_t)cc_linear(g, o[0] + r[0], o[1] + r[1], o[2] + r[2]);
        }
        parent[cc_linear(g, i0, i1, i2)] = p;
    }
}

// --- label, global merge: thread t of tile o unites its inside voxels with their inside forward neighbours in OTHER tiles ---
MRIRT_HD void cc_merge_thread(const CcGeom& g, uint32_t connectivity, const uint32_t o[3], int32_t* parent, uint32_t t) {
    for (uint32_t j = 0; j < kCcPerThread; ++j) {
        uint32_t c[3];
        cc_local_coords(j * kCcThreads + t, c);
        // a forward neighbour leaves the tile upwards on any axis, downwards only on axes 1 and 2
        if (c[0] != kCcT0 - 1 && c[1] != 0 && c[1] != kCcT1 - 1 && c[2] != 0 && c[2] != kCcT2 - 1) continue;
        const uint32_t i0 = o[0] + c[0], i1 = o[1] + c[1], i2 = o[2] + c[2];
        if (i0 >= g.n[0] || i1 >= g.n[1] || i2 >= g.n[2]) continue;
        const uint32_t v = cc_linear(g, i0, i1, i2);
        if (cc_load<kCcAgent>(parent + v) < 0) continue;
        for (uint32_t k = kCcFirstForward; k < kCcEndForward; ++k) {
            int32_t d[3];
            if (!cc_forward_offset(k, connectivity, d)) continue;
            const uint32_t m0 = c[0] + (uint32_t)d[0], m1 = c[1] + (uint32_t)d[1], m2 = c[2] + (uint32_t)d[2];
            if (m0 < kCcT0 && m1 < kCcT1 && m2 < kCcT2) continue;                       // the local pass united these
            const uint32_t w0 = i0 + (uint32_t)d[0], w1 = i1 + (uint32_t)d[1], w2 = i2 + (uint32_t)d[2];
            if (w0 >= g.n[0] || w1 >= g.n[1] || w2 >= g.n[2]) continue;                 // (below 0 wraps to above n)
            const uint32_t w = cc_linear(g, w0, w1, w2);
            if (cc_load<kCcAgent>(parent + w) >= 0) cc_union<kCcAgent>(parent, (int32_t)v, (int32_t)w);
        }
    }
}

// --- label, flatten (its own launch, after the merge): element i points at its root ---------------------------------------
MRIRT_HD void cc_flatten_element(int32_t* parent, uint32_t i) {
    const int32_t p = parent[i];
    if (p >= 0) parent[i] = cc_find<kCcPlain>(parent, p);
}

// --- number: roots are parent[i] == i; root number k (1 ..) is kept as -(k) - 1 until the last launch (-1 stays outside) ---
MRIRT_HD uint32_t cc_is_root(const int32_t* parent, uint32_t i) { return parent[i] == (int32_t)i ? 1u : 0u; }
MRIRT_HD int32_t cc_encode_number(uint32_t k) { return -(int32_t)k - 1; }
// a non-root reads its root's encoded number (roots are not rewritten in this launch, non-roots are not read)
MRIRT_HD void cc_spread_element(int32_t* parent, uint32_t i) {
    const int32_t p = parent[i];
    if (p < 0) return;
    const int32_t r = parent[p];
    parent[i] = r <= -2 ? -r - 1 : 0;
}
MRIRT_HD void cc_flip_element(int32_t* parent, uint32_t i) {
    const int32_t p = parent[i];
    if (p < 0) parent[i] = -p - 1;                       // -1 -> 0, -(k) - 1 -> k
}

// --- sizes: a workgroup sums into an LDS table first — slot c % 256 belongs to the first number that claims it, a number
// that finds its slot taken adds to memory directly — and adds every slot to memory once at its end ---------------------
MRIRT_HD int32_t cc_lds_claim(int32_t* tag, int32_t c) {           // *tag == 0 ? *tag = c : nothing; returns what *tag held
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t expected = 0;
    __hip_atomic_compare_exchange_strong(tag, &expected, c, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return expected;
#else
    const int32_t old = *tag;
    if (old == 0) *tag = c;
    return old;
#endif
}
MRIRT_HD void cc_lds_add(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    *p += v;
#endif
}
MRIRT_HD void cc_sizes_add(int32_t* tags, int32_t* counts, int32_t* sizes, int32_t c, int32_t n) {
    const uint32_t slot = (uint32_t)c % kCcSizeSlots;
    const int32_t old = cc_lds_claim(tags + slot, c);
    if (old == 0 || old == c) cc_lds_add(counts + slot, n);
    else cc_atomic_add(sizes + (c - 1), n);
}
// a thread's kCcItems consecutive elements from `base` on, equal neighbours summed before they reach the table
MRIRT_HD void cc_sizes_thread(const int32_t* components, uint32_t total, int64_t nComponents, int32_t* tags, int32_t* counts,
                              int32_t* sizes, uint32_t base) {
    int32_t cur = 0, cnt = 0;
    for (uint32_t i = 0; i < kCcItems; ++i) {
        const int32_t c = base + i < total ? components[base + i] : 0;
        if (c == cur) { ++cnt; continue; }
        if (cur >= 1 && (int64_t)cur <= nComponents) cc_sizes_add(tags, counts, sizes, cur, cnt);
        cur = c;
        cnt = 1;
    }
    if (cur >= 1 && (int64_t)cur <= nComponents) cc_sizes_add(tags, counts, sizes, cur, cnt);
}
// thread t < kCcSizeSlots (after every thread's cc_sizes_thread): its slot's sum to memory
MRIRT_HD void cc_sizes_flush(const int32_t* tags, const int32_t* counts, int32_t* sizes, uint32_t t) {
    if (tags[t] != 0) cc_atomic_add(sizes + (tags[t] - 1), counts[t]);
}

// --- filter --------------------------------------------------------------------------------------------------------------
// larger size wins, then the lower number: the maximum of these keys is the largest component (0 = none)
MRIRT_HD unsigned long long cc_size_key(int32_t size, uint32_t index) {
    return ((unsigned long long)(uint32_t)(size < 0 ? 0 : size) << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}
MRIRT_HD int16_t cc_filter_value(int16_t label, int32_t c, const int32_t* sizes, int64_t nComponents, int64_t minVoxels,
                                 uint32_t keepLargest, unsigned long long bestKey, int16_t fill) {
    if (c < 1 || (int64_t)c > nComponents) return label;
    const int32_t size = sizes[c - 1];
    bool kept = (int64_t)size >= minVoxels;
    if (keepLargest != 0u) kept = kept && cc_size_key(size, (uint32_t)(c - 1)) == bestKey;
    return kept ? label : fill;
}

// --- slice counts: bit 0 = A (p > 0), bit 1 = I (p == prev and p > 0), bit 2 = U (p > 0 or prev > 0); z == 0 has no prev ---
MRIRT_HD uint32_t cc_slice_flags(int16_t p, int16_t prev, bool hasPrev) {
    uint32_t f = p > 0 ? 1u : 0u;
    if (hasPrev) f |= ((p == prev && p > 0) ? 2u : 0u) | ((p > 0 || prev > 0) ? 4u : 0u);
    return f;
}

// --- scratch: level[l] = one uint32 per chunk of level l - 1 (level -1 = the voxels), until one chunk holds a level ------
struct CcPlan {
    CcGeom g;
    uint32_t levels, count[kCcMaxLevels];
    int64_t level[kCcMaxLevels], total;
};

MRIRT_HD int64_t cc_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Argument check shared by the entry points (host; before any HIP call).  Returns a MrirtStatus value (0 = fine).
inline int cc_geom(const uint32_t hwd[3], CcGeom* g) {
    uint64_t total = 1;
    for (int k = 0; k < 3; ++k) {
        if (hwd[k] == 0) return -2;                                           // MRIRT_ERR_DIMS
        total *= (uint64_t)hwd[k];
        if (total > kCcMaxVoxels) return -5;                                  // MRIRT_ERR_ARG
    }
    for (int k = 0; k < 3; ++k) g->n[k] = hwd[k];
    g->total = (uint32_t)total;
    g->tiles[0] = (hwd[0] + kCcT0 - 1) / kCcT0;
    g->tiles[1] = (hwd[1] + kCcT1 - 1) / kCcT1;
    g->tiles[2] = (hwd[2] + kCcT2 - 1) / kCcT2;
    g->numTiles = g->tiles[0] * g->tiles[1] * g->tiles[2];                    // <= total: every tile holds a voxel
    return 0;
}

inline int cc_plan(const uint32_t hwd[3], CcPlan* p) {
    const int rc = cc_geom(hwd, &p->g);
    if (rc != 0) return rc;
    p->levels = 0;
    uint32_t n = p->g.total;
    int64_t at = 0;
    do {
        n = (n + kCcChunk - 1) / kCcChunk;
        p->count[p->levels] = n;
        p->level[p->levels++] = at;
        at += cc_align((int64_t)n * 4);
    } while (n > kCcChunk);
    p->total = at;
    return 0;
}

}  // namespace mrirt
