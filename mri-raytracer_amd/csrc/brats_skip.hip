// The pre-pass of exact empty-space skipping (K1): from the per-launch "contributes nothing" flag of every 8^3 macro cell
// to the empty-radius map the skipping march reads (brats_march.hip: MapWindow, march_skip).  The map's layout and index
// arithmetic are skip_map.h's; the macro-cell summaries the flags are computed from are built once per volume by
// mrirt_build_macro_max / mrirt_build_macro_labels (grid_ops.hip).
#include "brats_host.h"
#include "skip_map.h"

namespace mrirt {

// ---------------------------------------------------------------------------------------
// Exact empty-space skipping: the per-launch mask.  Bit = 1 when, for every sample whose base cell lies in
// the macro cell, val <= 0 is certain (the same weighted sum / wSum division / window test as the march,
// evaluated on per-cell upper bounds of the trilinear fetch: every step is monotone, so bound in -> bound
// out) and no shown label grid holds a label there.
// ---------------------------------------------------------------------------------------
struct SkipArgs {
    uint32_t cells, nch;
    const float* ub[4];          // compacted like K1Args::chan
    float w[4];
    UDiv wsum;
    float tfLo;
    const uint32_t* seg;
    const uint32_t* pred;
    uint32_t* mask;
};

template <bool STRICT>
__global__ __launch_bounds__(256) void skip_mask_kernel(const SkipArgs k) {
    using Mm = M<STRICT>;
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    bool empty = false;
    if (cell < k.cells) {
        float v = 0.0f;
        for (uint32_t c = 0; c < k.nch; ++c) v = Mm::mad(k.ub[c][cell], k.w[c], v);
        if (k.wsum.d > 0.0f) v = Mm::divu_data(v, k.wsum);
        empty = v <= k.tfLo;                                         // NaN / inf bounds: not empty
        if (k.seg != nullptr && k.seg[cell] != 0u) empty = false;
        if (k.pred != nullptr && k.pred[cell] != 0u) empty = false;
    }
    const uint64_t bits = __ballot(empty);
    const int64_t w = skip_ballot_word(cell, k.cells);               // mask holds whole ballots only
    if ((threadIdx.x & 63u) == 0u && w >= 0) {
        k.mask[w] = (uint32_t)bits;
        k.mask[w + 1] = (uint32_t)(bits >> 32);
    }
}

// one separable pass of the distance map (skip_dist_cell, skip_map.h): pass x reads the bits, passes y and z the previous bytes
template <int AXIS>
__global__ __launch_bounds__(256) void skip_dist_kernel(const uint32_t* __restrict__ mask, const uint8_t* __restrict__ prev,
                                                        uint8_t* __restrict__ next, uint32_t mx, uint32_t my, uint32_t mz) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= mx * my * mz) return;
    next[c] = (uint8_t)skip_dist_cell<AXIS>(c, mx, my, mz, [&](uint32_t cell) -> uint32_t {
        if constexpr (AXIS == 0) return skip_bit_value(mask, cell);
        else return prev[cell];
    });
}

int launch_skip_prepass(const MrirtBratsParams* p, const MrirtSkip* skip, bool strict, hipStream_t s, K1Args& a) {
    const uint32_t mx = (p->dims[0] + 7) / 8, my = (p->dims[1] + 7) / 8, mz = (p->dims[2] + 7) / 8, cells = mx * my * mz;
    // bits -> distance bytes; the two byte maps follow the bit words in the same scratch (mrirt_skip_mask_words)
    uint8_t* mapA = reinterpret_cast<uint8_t*>(skip->mask + skip_bit_words(cells));
    if (skip->mapReady == 0) {       // (otherwise the scratch already holds this configuration's map: the caller vouches for it)
        SkipArgs k;
        k.cells = cells; k.nch = a.nch;
        for (uint32_t c = 0; c < 4; ++c) { k.ub[c] = c < a.nch ? skip->macroUb[a.chan[c]] : nullptr; k.w[c] = c < a.nch ? a.weight[a.chan[c]] : 0.0f; }
        k.wsum = a.wsum; k.tfLo = a.tfLo;
        k.seg = p->showSeg != 0 ? skip->macroSeg : nullptr;
        k.pred = p->showPred != 0 ? skip->macroPred : nullptr;
        k.mask = skip->mask;
        const dim3 grid((k.cells + 255) / 256), block(256);
        if (strict) hipLaunchKernelGGL(skip_mask_kernel<true>, grid, block, 0, s, k);
        else        hipLaunchKernelGGL(skip_mask_kernel<false>, grid, block, 0, s, k);
        MRIRT_HIP(hipGetLastError());
        uint8_t* mapB = mapA + skip_map_stride(k.cells);
        hipLaunchKernelGGL(skip_dist_kernel<0>, grid, block, 0, s, skip->mask, (const uint8_t*)nullptr, mapA, mx, my, mz);
        hipLaunchKernelGGL(skip_dist_kernel<1>, grid, block, 0, s, skip->mask, (const uint8_t*)mapA, mapB, mx, my, mz);
        hipLaunchKernelGGL(skip_dist_kernel<2>, grid, block, 0, s, skip->mask, (const uint8_t*)mapB, mapA, mx, my, mz);
        MRIRT_HIP(hipGetLastError());
    }
    a.skipDist = mapA; a.mX = mx; a.mXY = mx * my; a.mY = my; a.mZ = mz;
    return MRIRT_OK;
}

}  // namespace mrirt
