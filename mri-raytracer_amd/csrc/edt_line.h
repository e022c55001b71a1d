// Exact squared Euclidean distance transform, the per-thread text: pass geometry, tile load, the 1-D line pass and the
// scratch layout of mrirt_hausdorff, written once for the device kernels (csrc/edt.hip) and for the host
// (tests/native/edt_harness.hip runs it under AddressSanitizer + UBSan with every buffer exactly its size long).
//
// Definition ("Hausdorff distance and the exact distance transform"): the coordinate of index i on an axis with
// spacing s is c(i) = double(float(i) * s) — the reference's float32 coordinate grid, widened (inr/inr/model.py:168-172) —
// and one pass along an axis is g'[i] = min_j (g[j] + (c(i) - c(j))^2): a subtraction, a square, an addition and a minimum,
// four separate fp64 operations (compiled with -ffp-contract=off).  Three passes, axis 0 then 1 then 2, from g = 0 on the
// mask and +inf elsewhere give min_y ((d0^2 + d1^2) + d2^2) with those very roundings, because x -> fl(x + b) is monotone:
// min_j fl(x_j + b) = fl(min_j x_j + b).  The pass is the O(n^2) minimum itself, not a lower envelope: nothing to prove.
//
// Organisation of a pass: a tile is TL neighbouring lines, whole (n elements each), staged as tile[j * TL + l] next to the
// n coordinates; thread t owns line l = t % TL and computes kEdtBlock outputs i at a time, so one staged g[j] serves four
// (sub, mul, add, min) groups.  Along axes 0 and 1 neighbouring lines are neighbouring addresses (the D axis is contiguous):
// loads and stores of a tile are runs of TL doubles.  Along axis 2 the lines themselves are contiguous and the load
// transposes them into the same tile shape.  A tile is loaded completely before any of its outputs is stored and tiles are
// disjoint, so a pass runs in place.
#pragma once
#include <math.h>

#include "mrirt_device.h"

namespace mrirt {

constexpr uint32_t kEdtMaxLine = 4096;        // longest axis (documented in include/mrirt.h): tile + coordinates fit 64 KiB
constexpr uint32_t kEdtMaxClasses = 32;
constexpr uint32_t kEdtThreads = 256;         // threads of a tile's workgroup
constexpr int kEdtBlock = 4;                  // outputs a thread forms per sweep over the line
constexpr uint32_t kEdtMaxTileLines = 16;
constexpr uint32_t kEdtTileBytes = 65536;     // staging budget of a workgroup: (n * TL + n) doubles
constexpr int64_t kEdtSquaredScratch = 64;    // mrirt_edt_scratch_bytes(hwd, 0): mrirt_edt_squared runs in place in its output
constexpr uint32_t kEdtAccWords = 4;          // per class: bits of a_c, bits of b_c, class present in pred, in truth

MRIRT_HD double edt_coord(uint32_t i, float s) { return (double)((float)i * s); }

// lines per tile: the largest power of two <= 16 whose tile and coordinate table fit the staging budget (>= 1 for n <= 4096)
MRIRT_HD uint32_t edt_tile_lines(uint32_t n) {
    uint32_t tl = kEdtMaxTileLines;
    while (tl > 1 && ((uint64_t)n * tl + n) * sizeof(double) > kEdtTileBytes) tl >>= 1;
    return tl;
}

// One pass over an [H][W][D] volume: `outer` groups of `inner` lines of n elements; element j of line q of group o is at
// o * outerStride + q * lineStride + j * elemStride.
struct EdtPass {
    uint32_t n, outer, inner, tl, chunks;     // chunks = tiles per group = ceil(inner / tl)
    int64_t outerStride, lineStride, elemStride;
    float s;
};

MRIRT_HD EdtPass edt_pass(const uint32_t hwd[3], int axis, float s) {
    const int64_t H = hwd[0], W = hwd[1], D = hwd[2];
    EdtPass p;
    p.s = s;
    if (axis == 0)      { p.n = hwd[0]; p.outer = 1;      p.inner = (uint32_t)(W * D); p.outerStride = 0;     p.lineStride = 1; p.elemStride = W * D; }
    else if (axis == 1) { p.n = hwd[1]; p.outer = hwd[0]; p.inner = hwd[2];            p.outerStride = W * D; p.lineStride = 1; p.elemStride = D; }
    else                { p.n = hwd[2]; p.outer = 1;      p.inner = (uint32_t)(H * W); p.outerStride = 0;     p.lineStride = D; p.elemStride = 1; }
    p.tl = edt_tile_lines(p.n);
    p.chunks = (p.inner + p.tl - 1) / p.tl;
    return p;
}

MRIRT_HD uint32_t edt_tile_count(const EdtPass& p, uint32_t chunk) {
    const uint32_t first = chunk * p.tl;
    return p.inner - first < p.tl ? p.inner - first : p.tl;
}

MRIRT_HD int64_t edt_offset(const EdtPass& p, uint32_t o, uint32_t chunk, uint32_t l, uint32_t j) {
    return (int64_t)o * p.outerStride + (int64_t)(chunk * p.tl + l) * p.lineStride + (int64_t)j * p.elemStride;
}

// Thread t of nt stages its share of tile (o, chunk): from the field, or — the first pass — from the label volume as
// 0 where label == cls and +inf elsewhere.  tile holds n * tl doubles (lines past the tile's count stay unwritten and
// unread), ctab n.
MRIRT_HD void edt_tile_load(const EdtPass& p, uint32_t o, uint32_t chunk, const double* field, const int16_t* labels, int32_t cls,
                            double* tile, double* ctab, uint32_t t, uint32_t nt) {
    const uint32_t cnt = edt_tile_count(p, chunk), total = p.n * cnt;
    for (uint32_t idx = t; idx < total; idx += nt) {
        uint32_t l, j;
        if (p.lineStride == 1) { l = idx % cnt; j = idx / cnt; }      // neighbouring lines are neighbouring addresses
        else                   { j = idx % p.n; l = idx / p.n; }      // the line itself is contiguous
        const int64_t off = edt_offset(p, o, chunk, l, j);
        tile[j * p.tl + l] = labels != nullptr ? ((int32_t)labels[off] == cls ? 0.0 : (double)INFINITY) : field[off];
    }
    for (uint32_t j = t; j < p.n; j += nt) ctab[j] = edt_coord(j, p.s);
}

// The line pass: best[r] = min_j (g[j * gStride] + (c[i0 + r] - c[j])^2) for r < kEdtBlock (outputs past the line's end
// repeat the last one; the caller drops them).
MRIRT_HD void edt_line_block(const double* g, uint32_t gStride, const double* c, uint32_t n, uint32_t i0, double best[kEdtBlock]) {
    double ci[kEdtBlock];
    for (int r = 0; r < kEdtBlock; ++r) {
        ci[r] = c[i0 + r < n ? i0 + r : n - 1];
        best[r] = (double)INFINITY;
    }
    for (uint32_t j = 0; j < n; ++j) {
        const double gj = g[j * gStride], cj = c[j];
        for (int r = 0; r < kEdtBlock; ++r) {
            const double d = ci[r] - cj;
            const double d2 = d * d;
            const double v = gj + d2;
            best[r] = fmin(best[r], v);
        }
    }
}

// Thread t of nt forms and stores its outputs of the staged tile (after every thread's edt_tile_load).
MRIRT_HD void edt_tile_compute(const EdtPass& p, uint32_t o, uint32_t chunk, const double* tile, const double* ctab, double* field,
                               uint32_t t, uint32_t nt) {
    const uint32_t cnt = edt_tile_count(p, chunk), l = t % p.tl, groups = nt / p.tl;
    if (l >= cnt) return;
    for (uint32_t i0 = (t / p.tl) * kEdtBlock; i0 < p.n; i0 += groups * kEdtBlock) {
        double best[kEdtBlock];
        edt_line_block(tile + l, p.tl, ctab, p.n, i0, best);
        for (int r = 0; r < kEdtBlock; ++r)
            if (i0 + r < p.n) field[edt_offset(p, o, chunk, l, i0 + r)] = best[r];
    }
}

// Squared distances are >= 0 (or +inf): their bit patterns order as they do, so a maximum is an integer maximum.
MRIRT_HD uint64_t edt_bits(double x) { union { double d; uint64_t u; } v; v.d = x; return v.u; }
MRIRT_HD double edt_from_bits(uint64_t u) { union { double d; uint64_t u; } v; v.u = u; return v.d; }

// Scratch of mrirt_hausdorff: the two fields of the class in flight (F_T, F_P), then kEdtAccWords uint64 per class.
struct EdtScratch { int64_t field[2], acc, total; };
MRIRT_HD EdtScratch edt_scratch(int64_t voxels, uint32_t numClasses) {
    EdtScratch s;
    s.field[0] = 0;
    s.field[1] = voxels * (int64_t)sizeof(double);
    s.acc = 2 * voxels * (int64_t)sizeof(double);
    s.total = s.acc + (int64_t)numClasses * kEdtAccWords * (int64_t)sizeof(uint64_t);
    return s;
}

// Argument checks shared by the entry points (host; before any HIP call).  Returns a MrirtStatus value (0 = fine).
inline int edt_check_volume(const uint32_t hwd[3], const float spacing[3]) {
    uint64_t vox = 1;
    for (int k = 0; k < 3; ++k) {
        if (hwd[k] == 0 || hwd[k] > kEdtMaxLine) return -2;                   // MRIRT_ERR_DIMS
        vox *= hwd[k];
    }
    if (vox >= (1ull << 31)) return -2;
    if (spacing != nullptr)
        for (int k = 0; k < 3; ++k)                                           // the far end's coordinate must be finite too
            if (!isfinite(spacing[k]) || !isfinite((float)(hwd[k] - 1) * spacing[k])) return -5;   // MRIRT_ERR_ARG
    return 0;
}

}  // namespace mrirt
