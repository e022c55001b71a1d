// Dispatch order of the K1 march: which position of the pixel map each workgroup of a launch marches (PixelMap::order,
// mrirt_device.h), built from the step counts the previous frame recorded per workgroup (PixelMap::steps, finish()).
//
// The hardware deals workgroup b to XCD b % 8, so XCD x owns the slots x, x + 8, x + 16, ... of the launch and the table is a
// permutation of each XCD's own slots: a workgroup never changes XCD, and the bands fill_pixel_map gave each L2 stay its own.
// Inside an XCD the slots are binned into `classes` classes by predicted steps, thresholds at the XCD's own quantiles, and
// emitted longest class first, in slot order inside a class (stable): the long packets start in the first rounds of the
// launch, so the frame's tail is made of short ones, while neighbours — similar lengths, one class — still run together and
// share their lines in L2.  An all-zero record (first frame) gives the identity.
//
// This header is the permutation logic alone, plain C++ without HIP: the builder kernel (brats_order.hip) counts with wave
// ballots what order_build_xcd below counts in a loop, through the same order_rank / order_refine / order_class, and the
// host tests and the sanitizer harness (tests/native/order_harness.cpp) run order_build_table without a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRIRT_ORDER_HD __host__ __device__ inline
#else
#define MRIRT_ORDER_HD inline
#endif

namespace mrirt {

constexpr uint32_t kOrderXcds = 8;             // == kXcds (mrirt_device.h)
constexpr uint32_t kOrderMaxClasses = 16;
constexpr uint32_t kOrderDefaultClasses = 4;

// MrirtOrder::classes as the builder uses it
MRIRT_ORDER_HD uint32_t order_classes(uint32_t classes) {
    return classes == 0 ? kOrderDefaultClasses : classes > kOrderMaxClasses ? kOrderMaxClasses : classes;
}
// slots XCD `xcd` owns of a launch of `words` workgroups
MRIRT_ORDER_HD uint32_t order_slots(uint32_t words, uint32_t xcd) {
    return xcd < words ? (words - xcd + kOrderXcds - 1) / kOrderXcds : 0u;
}
// threshold j (1 .. C - 1) is the value of this rank (0-based) among the XCD's n values in ascending order
MRIRT_ORDER_HD uint32_t order_rank(uint32_t j, uint32_t n, uint32_t C) { return (uint32_t)(((uint64_t)j * n) / C); }
// One step of the bitwise selection of the value of rank k: `below` values are smaller than ans | bit.  The value of rank
// k is the largest x with at most k values below it, so the bit stays exactly when below <= k.
MRIRT_ORDER_HD uint32_t order_refine(uint32_t ans, uint32_t bit, uint32_t below, uint32_t k) { return below <= k ? (ans | bit) : ans; }
// the highest bit the selection starts from (maxValue != 0)
MRIRT_ORDER_HD uint32_t order_top_bit(uint32_t maxValue) {
    uint32_t bit = 1u;
    while ((maxValue >> 1) >= bit) bit <<= 1;
    return bit;
}
// class of a value: how many of the C - 1 thresholds it reaches (0 = shortest, C - 1 = longest)
MRIRT_ORDER_HD uint32_t order_class(uint32_t v, const uint32_t* thr, uint32_t C) {
    uint32_t c = 0;
    for (uint32_t j = 0; j + 1 < C; ++j) c += v >= thr[j] ? 1u : 0u;
    return c;
}

// One XCD's part of the table, serially: steps[k * 8 + xcd] is the record of slot k, order[pos * 8 + xcd] the slot marched
// pos-th.  Reads and writes nothing outside [0, words).
inline void order_build_xcd(const uint32_t* steps, uint32_t words, uint32_t xcd, uint32_t classes, uint32_t* order) {
    const uint32_t n = order_slots(words, xcd), C = order_classes(classes);
    uint32_t maxValue = 0;
    for (uint32_t k = 0; k < n; ++k) { const uint32_t v = steps[k * kOrderXcds + xcd]; maxValue = v > maxValue ? v : maxValue; }
    if (maxValue == 0) {
        for (uint32_t k = 0; k < n; ++k) order[k * kOrderXcds + xcd] = k * kOrderXcds + xcd;
        return;
    }
    uint32_t thr[kOrderMaxClasses] = {};
    for (uint32_t j = 1; j < C; ++j) {
        const uint32_t rank = order_rank(j, n, C);
        uint32_t ans = 0;
        for (uint32_t bit = order_top_bit(maxValue); bit != 0; bit >>= 1) {
            uint32_t below = 0;
            for (uint32_t k = 0; k < n; ++k) below += steps[k * kOrderXcds + xcd] < (ans | bit) ? 1u : 0u;
            ans = order_refine(ans, bit, below, rank);
        }
        thr[j - 1] = ans;
    }
    uint32_t pos = 0;
    for (uint32_t c = C; c-- > 0;)
        for (uint32_t k = 0; k < n; ++k)
            if (order_class(steps[k * kOrderXcds + xcd], thr, C) == c) order[(pos++) * kOrderXcds + xcd] = k * kOrderXcds + xcd;
}

inline void order_build_table(const uint32_t* steps, uint32_t words, uint32_t classes, uint32_t* order) {
    for (uint32_t xcd = 0; xcd < kOrderXcds; ++xcd) order_build_xcd(steps, words, xcd, classes, order);
}

}  // namespace mrirt
