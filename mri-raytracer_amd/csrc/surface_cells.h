// Naive surface nets of a label volume, the per-thread text: the corner mask of a cell, the vertex of an active cell, the
// ownership test and the winding of a quad, the classify tile and the scratch layout of mrirt_surface_count /
// mrirt_surface_extract, written once for the device kernels (csrc/surface.hip) and for the host
// (tests/native/surface_harness.hip runs it under AddressSanitizer + UBSan with every buffer exactly its size long).
//
// Definition ("Class surfaces from label volumes"): a volume of (n0, n1, n2) voxels has (n0+1)(n1+1)(n2+1) cells;
// cell c = (c0, c1, c2), linear index (c0 (n1+1) + c1)(n2+1) + c2, has the voxels c - 1 + b, b in {0,1}^3, as corners, and a
// voxel outside the volume is outside.  Bit 4 b0 + 2 b1 + b2 of a cell's corner mask is set when corner b is inside; a cell
// is active when its mask is neither 0 nor 255.  Everything below is integer tests but for one float32 division, one
// addition, one multiplication and one more addition per vertex coordinate, each separate (-ffp-contract=off).
#pragma once
#include <math.h>

#include "mrirt_device.h"

namespace mrirt {

constexpr uint32_t kSurfThreads = 256;                 // threads of every workgroup of csrc/surface.hip
constexpr uint32_t kSurfItems = 4;                     // consecutive elements a thread of a scan / emit workgroup owns
constexpr uint32_t kSurfChunk = kSurfThreads * kSurfItems;      // elements a workgroup reduces or scans
constexpr uint32_t kSurfT0 = 4, kSurfT1 = 4, kSurfT2 = 64;      // classify tile, in cells: thread t owns the column (t / 64, t % 64)
constexpr uint32_t kSurfTileBytes = (kSurfT0 + 1) * (kSurfT1 + 1) * (kSurfT2 + 1);   // its voxels' inside flags, one byte each
constexpr uint32_t kSurfMaxLevels = 3;                 // 1024^3 > 2^31 - 1 cells: three levels of sums always end in one chunk
constexpr uint64_t kSurfMaxCells = 0x7FFFFFFFull;

struct SurfGeom {
    uint32_t n[3];        // voxels per axis
    uint32_t nc[3];       // cells per axis (n + 1)
    uint32_t s[3];        // cell strides: nc1 * nc2, nc2, 1
    uint32_t cells;
    uint32_t tiles[3];    // classify tiles per axis
};

// sums of (active cells, owned quads) over a run of cells: a quad total can pass 2^32 (three per cell)
struct SurfCount {
    unsigned long long v, q;
};
MRIRT_HD SurfCount operator+(const SurfCount& a, const SurfCount& b) { return SurfCount{ a.v + b.v, a.q + b.q }; }

MRIRT_HD bool surf_inside(int32_t label, uint32_t classMask) { return label >= 0 && label < 32 && ((classMask >> label) & 1u) != 0u; }

MRIRT_HD void surf_cell_coords(const SurfGeom& g, uint32_t cell, uint32_t c[3]) {
    c[2] = cell % g.nc[2];
    const uint32_t r = cell / g.nc[2];
    c[1] = r % g.nc[1];
    c[0] = r / g.nc[1];
}

// --- classify: one workgroup per tile of kSurfT0 x kSurfT1 x kSurfT2 cells -----------------------------------------------
MRIRT_HD void surf_tile_origin(const SurfGeom& g, uint32_t tileId, uint32_t o[3]) {
    o[2] = (tileId % g.tiles[2]) * kSurfT2;
    const uint32_t r = tileId / g.tiles[2];
    o[1] = (r % g.tiles[1]) * kSurfT1;
    o[0] = (r / g.tiles[1]) * kSurfT0;
}

// Thread t of nt stages its share of the tile's (T0+1)(T1+1)(T2+1) voxels — voxel o - 1 + (i, j, k) at
// tile[(i (T1+1) + j)(T2+1) + k] — as inside flags, so every label of the tile is read from memory once.
MRIRT_HD void surf_tile_load(const SurfGeom& g, const int16_t* labels, uint32_t classMask, const uint32_t o[3], uint8_t* tile,
                             uint32_t t, uint32_t nt) {
    for (uint32_t idx = t; idx < kSurfTileBytes; idx += nt) {
        const uint32_t k = idx % (kSurfT2 + 1), r = idx / (kSurfT2 + 1), j = r % (kSurfT1 + 1), i = r / (kSurfT1 + 1);
        const int64_t v0 = (int64_t)o[0] + i - 1, v1 = (int64_t)o[1] + j - 1, v2 = (int64_t)o[2] + k - 1;
        bool in = false;
        if (v0 >= 0 && v0 < (int64_t)g.n[0] && v1 >= 0 && v1 < (int64_t)g.n[1] && v2 >= 0 && v2 < (int64_t)g.n[2])
            in = surf_inside((int32_t)labels[(v0 * g.n[1] + v1) * g.n[2] + v2], classMask);
        tile[idx] = in ? 1u : 0u;
    }
}

// the four corners (b1, b2) of plane i of the staged tile, for the column (l1, l2): bits 2 b1 + b2
MRIRT_HD uint32_t surf_tile_plane(const uint8_t* tile, uint32_t i, uint32_t l1, uint32_t l2) {
    const uint8_t* r = tile + (i * (kSurfT1 + 1) + l1) * (kSurfT2 + 1) + l2;
    return (uint32_t)r[0] | ((uint32_t)r[1] << 1) | ((uint32_t)r[kSurfT2 + 1] << 2) | ((uint32_t)r[kSurfT2 + 2] << 3);
}

// Thread t (of kSurfThreads = T1 * T2) writes the corner masks of its column of the tile (after every thread's surf_tile_load).
MRIRT_HD void surf_tile_classify(const SurfGeom& g, const uint32_t o[3], const uint8_t* tile, uint8_t* code, uint32_t t) {
    const uint32_t l1 = t / kSurfT2, l2 = t % kSurfT2, c1 = o[1] + l1, c2 = o[2] + l2;
    if (c1 >= g.nc[1] || c2 >= g.nc[2]) return;
    uint32_t lower = surf_tile_plane(tile, 0, l1, l2);
    for (uint32_t l0 = 0; l0 < kSurfT0 && o[0] + l0 < g.nc[0]; ++l0) {
        const uint32_t upper = surf_tile_plane(tile, l0 + 1, l1, l2);
        code[(o[0] + l0) * g.s[0] + c1 * g.s[1] + c2] = (uint8_t)(lower | (upper << 4));
        lower = upper;
    }
}

// --- what a cell contributes ---------------------------------------------------------------------------------------------
MRIRT_HD bool surf_active(uint32_t mask) { return mask != 0u && mask != 255u; }

// Bit a is set when cell c owns the lattice edge from voxel c - 1 along axis a (c_b >= 1 and c_c >= 1 for the cyclic
// triple (a, b, c)) and that edge's two voxels differ: the edge emits a quad.
MRIRT_HD uint32_t surf_quad_axes(uint32_t mask, const uint32_t c[3]) {
    const uint32_t b000 = mask & 1u;
    uint32_t axes = 0;
    if (c[1] >= 1 && c[2] >= 1 && ((mask >> 4) & 1u) != b000) axes |= 1u;
    if (c[2] >= 1 && c[0] >= 1 && ((mask >> 2) & 1u) != b000) axes |= 2u;
    if (c[0] >= 1 && c[1] >= 1 && ((mask >> 1) & 1u) != b000) axes |= 4u;
    return axes;
}

// vertex flag in bits 0..15, owned-quad count (0..3) in bits 16..31: the sum over a chunk of kSurfChunk cells fits both halves
MRIRT_HD uint32_t surf_cell_counts(uint32_t mask, const uint32_t c[3]) {
    const uint32_t axes = surf_quad_axes(mask, c);
    return (surf_active(mask) ? 1u : 0u) | (((axes & 1u) + ((axes >> 1) & 1u) + (axes >> 2)) << 16);
}

// The vertex of an active cell: over the cell's edges whose two corners differ (from corner b along axis a, b_a = 0),
// S_k = sum of 2 b_k + (k == a) and m their number; q_k = float(S_k) / float(2 m), x_k = (float(c_k - 1) + q_k) * spacing_k + origin_k.
MRIRT_HD void surf_vertex(uint32_t mask, const uint32_t c[3], const float spacing[3], const float origin[3], float x[3]) {
    int32_t S[3] = { 0, 0, 0 }, m = 0;
    for (int a = 0; a < 3; ++a) {
        const uint32_t ea = 4u >> a;
        for (uint32_t b = 0; b < 8; ++b) {
            if ((b & ea) != 0u || (((mask >> b) ^ (mask >> (b | ea))) & 1u) == 0u) continue;
            ++m;
            for (int k = 0; k < 3; ++k) S[k] += 2 * (int32_t)((b >> (2 - k)) & 1u) + (k == a ? 1 : 0);
        }
    }
    const float den = (float)(2 * m);
    for (int k = 0; k < 3; ++k) {
        const float q = (float)S[k] / den;
        const float p = (float)((int32_t)c[k] - 1) + q;
        const float sx = p * spacing[k];
        x[k] = sx + origin[k];
    }
}

// The two triangles of the quad around the edge along axis a that cell `cell` owns: Q(ib, ic) is the vertex of cell
// c - (1 - ib) e_b - (1 - ic) e_c; the normal points along +a when voxel c - 1 (corner 0) is inside.
MRIRT_HD void surf_quad(const SurfGeom& g, int a, uint32_t mask, uint32_t cell, const uint32_t* vidx, int32_t tri[6]) {
    const uint32_t sb = g.s[(a + 1) % 3], sc = g.s[(a + 2) % 3];
    const int32_t q00 = (int32_t)vidx[cell - sb - sc], q10 = (int32_t)vidx[cell - sc], q01 = (int32_t)vidx[cell - sb],
                  q11 = (int32_t)vidx[cell];
    const bool in = (mask & 1u) != 0u;
    tri[0] = q00; tri[1] = in ? q10 : q11; tri[2] = in ? q11 : q10;
    tri[3] = q00; tri[4] = in ? q11 : q01; tri[5] = in ? q01 : q11;
}

// --- scratch ---------------------------------------------------------------------------------------------------------------
// code: one corner mask per cell (padded to whole chunks); vidx: the vertex number of every ACTIVE cell (others unwritten
// and unread); level[l]: SurfCount per chunk of level l - 1 (level -1 = the cells), reduced upwards until one chunk holds
// a level, then scanned downwards in place into exclusive prefixes.
struct SurfPlan {
    SurfGeom g;
    uint32_t levels, count[kSurfMaxLevels];
    int64_t code, vidx, level[kSurfMaxLevels], total;
};

MRIRT_HD int64_t surf_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Argument checks shared by the entry points (host; before any HIP call).  Returns a MrirtStatus value (0 = fine) and the plan.
inline int surf_plan(const uint32_t hwd[3], SurfPlan* p) {
    uint64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        if (hwd[k] == 0) return -2;                                           // MRIRT_ERR_DIMS
        cells *= (uint64_t)hwd[k] + 1;
        if (cells > kSurfMaxCells) return -5;                                 // MRIRT_ERR_ARG
    }
    SurfGeom& g = p->g;
    for (int k = 0; k < 3; ++k) { g.n[k] = hwd[k]; g.nc[k] = hwd[k] + 1; }
    g.s[0] = g.nc[1] * g.nc[2]; g.s[1] = g.nc[2]; g.s[2] = 1;
    g.cells = (uint32_t)cells;
    g.tiles[0] = (g.nc[0] + kSurfT0 - 1) / kSurfT0;
    g.tiles[1] = (g.nc[1] + kSurfT1 - 1) / kSurfT1;
    g.tiles[2] = (g.nc[2] + kSurfT2 - 1) / kSurfT2;
    if ((uint64_t)g.tiles[0] * g.tiles[1] * g.tiles[2] > kSurfMaxCells) return -5;
    p->levels = 0;
    uint32_t n = g.cells;
    do {
        n = (n + kSurfChunk - 1) / kSurfChunk;
        p->count[p->levels++] = n;
    } while (n > kSurfChunk);                                                 // the top level fits one chunk: one workgroup scans it
    const int64_t chunks = p->count[0];
    p->code = 0;
    p->vidx = surf_align(chunks * kSurfChunk);
    int64_t at = p->vidx + surf_align((int64_t)g.cells * 4);
    for (uint32_t l = 0; l < p->levels; ++l) {
        p->level[l] = at;
        at += surf_align((int64_t)p->count[l] * (int64_t)sizeof(SurfCount));
    }
    p->total = at;
    return 0;
}

inline int surf_check_frame(const float spacing[3], const float origin[3]) {
    for (int k = 0; k < 3; ++k)
        if (!isfinite(spacing[k]) || !(spacing[k] > 0.0f) || !isfinite(origin[k])) return -5;   // MRIRT_ERR_ARG
    return 0;
}

}  // namespace mrirt
