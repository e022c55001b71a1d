// Exact empty-space skipping: the index arithmetic of the map, written once for the device (csrc/brats_skip.hip builds the
// map, the skipping march of csrc/brats_march.hip reads it through MapWindow), for the host wrappers (mrirt_skip_mask_words,
// csrc/grid_ops.hip) and for tests/native/index_harness.hip, which walks it under AddressSanitizer + UBSan.
//
// Scratch layout: MrirtSkip::mask points at mrirt_skip_mask_words(dims) 32-bit words.  First the 8^3 macro cells' bits as
// whole 64-lane ballots (skip_bit_words(cells) words: skip_mask_kernel's lane 0 stores two words per wave), then two byte maps
// of skip_map_stride(cells) bytes each: the empty-radius map the march reads (byte r of a cell: 0 = may contribute, r >= 1 =
// this cell and every macro cell within Chebyshev distance r - 1 contribute nothing), and the scratch of its separable passes.
#pragma once
#include "mrirt_device.h"

namespace mrirt {

constexpr uint32_t kSkipDistCap = 31;  // largest radius the map records: 239 voxels of room

MRIRT_HD uint32_t skip_bit_words(uint32_t cells) { return ((cells + 63u) / 64u) * 2u; }
MRIRT_HD uint32_t skip_map_stride(uint32_t cells) { return (cells + 3u) & ~3u; }
// where lane 0 of the wave whose first cell is `cell` stores its ballot (two words), or -1: no store
MRIRT_HD int64_t skip_ballot_word(uint32_t cell, uint32_t cells) { return cell < ((cells + 63u) & ~63u) ? (int64_t)(cell >> 5) : -1; }

// The distance map from the mask, one axis at a time (box emptiness is separable).  r(c) = largest r <= cap such that
// every in-grid cell within r - 1 of c along the axes done so far has the property; cells outside the grid never hold a
// sample, so they do not constrain.  Pass x reads the bits, passes y and z read the previous pass's bytes.
// `at(cell)` = the previous pass's value of a cell (pass x: cap or 0 from the bit).
template <int AXIS, class At>
MRIRT_HD uint32_t skip_dist_cell(uint32_t c, uint32_t mx, uint32_t my, uint32_t mz, At at) {
    const uint32_t xyz[3] = { c % mx, (c / mx) % my, c / (mx * my) }, ext[3] = { mx, my, mz };
    const uint32_t stride = AXIS == 0 ? 1u : AXIS == 1 ? mx : mx * my;
    // m = smallest value within distance r of c; radius r + 1 is good when m >= r + 1
    uint32_t m = at(c), r = 0;
    while (r < m && r < kSkipDistCap) {
        ++r;
        if (xyz[AXIS] >= r) { const uint32_t v = at(c - r * stride); m = v < m ? v : m; }
        if (xyz[AXIS] + r < ext[AXIS]) { const uint32_t v = at(c + r * stride); m = v < m ? v : m; }
    }
    return r;
}
MRIRT_HD uint32_t skip_bit_value(const uint32_t* mask, uint32_t cell) { return ((mask[cell >> 5] >> (cell & 31u)) & 1u) != 0 ? kSkipDistCap : 0u; }

// MapWindow's index arithmetic (csrc/brats_march.hip): a 4 x 4 x 4 block of macro cells at origin (ox, oy, oz), one per lane
MRIRT_HD uint32_t window_origin(bool towardsPlus, uint32_t lo, uint32_t hi) { return towardsPlus ? lo : max(hi, 3u) - 3u; }
MRIRT_HD bool window_holds(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t ox, uint32_t oy, uint32_t oz) {
    return (cx - ox) < 4u && (cy - oy) < 4u && (cz - oz) < 4u;
}
MRIRT_HD uint32_t window_slot(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t ox, uint32_t oy, uint32_t oz) {
    return ((cx - ox) + 4u * (cy - oy) + 16u * (cz - oz)) & 63u;
}
// the macro cell lane `lane` fetches when the window moves to (ox, oy, oz): clamped into the map
MRIRT_HD uint32_t window_fetch_index(uint32_t ox, uint32_t oy, uint32_t oz, uint32_t lane, uint32_t mX, uint32_t mY, uint32_t mZ, uint32_t mXY) {
    const uint32_t gx = min(ox + (lane & 3u), mX - 1u), gy = min(oy + ((lane >> 2) & 3u), mY - 1u), gz = min(oz + (lane >> 4), mZ - 1u);
    return gx + gy * mX + gz * mXY;
}

}  // namespace mrirt
