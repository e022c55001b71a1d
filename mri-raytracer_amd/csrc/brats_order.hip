// K1: the builder of the march's dispatch order (k1_order.h), one small launch ahead of the march on the same stream.
// One workgroup per XCD reads the steps the last frame recorded for that XCD's slots, selects the class thresholds, writes
// the XCD's part of the order table — longest class first, slot order inside a class — and zeroes the record for the march
// that follows.  The counting is wave ballots; every decision goes through the functions of k1_order.h that the serial
// host version uses.
#include "brats_host.h"
#include "k1_order.h"

namespace mrirt {

static_assert(kOrderXcds == kXcds, "the order table is a permutation inside each XCD's slots");

constexpr uint32_t kOrderThreads = 256, kOrderWaves = kOrderThreads / 64;
constexpr uint32_t kOrderStaged = 4096;         // slots per XCD held in LDS (a 4096 x 4096 frame of 16-px workgroups has 8192)

__global__ __launch_bounds__(kOrderThreads) void order_build_kernel(uint32_t* steps, uint32_t words, uint32_t classes, uint32_t* order) {
    __shared__ uint32_t staged[kOrderStaged];
    __shared__ uint32_t below[32][kOrderMaxClasses];                 // per bit of the selection, per threshold
    __shared__ uint32_t total[kOrderMaxClasses], run[kOrderMaxClasses], thrShared[kOrderMaxClasses];
    __shared__ uint32_t waveCnt[2][kOrderWaves][kOrderMaxClasses];
    __shared__ uint32_t maxShared;
    const uint32_t xcd = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = order_slots(words, xcd), C = order_classes(classes);
    const bool inLds = n <= kOrderStaged;
    // slot k of this XCD is the position k * 8 + xcd of the pixel map, which is what the record is filed by (finish())
    auto record = [&](uint32_t k) { return steps[k * kXcds + xcd]; };
    auto value = [&](uint32_t k) { return inLds ? staged[k] : record(k); };

    for (uint32_t i = tid; i < 32u * kOrderMaxClasses; i += kOrderThreads) (&below[0][0])[i] = 0u;
    if (tid < kOrderMaxClasses) { total[tid] = 0u; run[tid] = 0u; }
    if (tid == 0) maxShared = 0u;
    __syncthreads();
    uint32_t vmax = 0;
    for (uint32_t k = tid; k < n; k += kOrderThreads) {
        const uint32_t v = record(k);
        if (inLds) staged[k] = v;
        vmax = max(vmax, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor(vmax, o));
    if (lane == 0 && vmax != 0u) atomicMax(&maxShared, vmax);
    __syncthreads();
    const uint32_t maxValue = maxShared;
    if (maxValue == 0u) {                                            // nothing recorded (first frame): the identity
        for (uint32_t k = tid; k < n; k += kOrderThreads) order[k * kXcds + xcd] = k * kXcds + xcd;
        return;
    }

    // the C - 1 thresholds together, one bit per trip (order_refine)
    uint32_t thr[kOrderMaxClasses];
#pragma unroll
    for (uint32_t j = 0; j < kOrderMaxClasses; ++j) thr[j] = 0u;
    uint32_t trip = 0;
    for (uint32_t bit = order_top_bit(maxValue); bit != 0u; bit >>= 1, ++trip) {
        for (uint32_t base = 0; base < n; base += kOrderThreads) {
            const uint32_t k = base + tid;
            const bool have = k < n;
            const uint32_t v = have ? value(k) : 0u;
#pragma unroll
            for (uint32_t j = 0; j < kOrderMaxClasses - 1; ++j) {
                if (j + 1 < C) {
                    const uint32_t cnt = (uint32_t)__popcll(__ballot(have && v < (thr[j] | bit)));
                    if (lane == 0 && cnt != 0u) atomicAdd(&below[trip][j], cnt);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kOrderMaxClasses - 1; ++j)
            if (j + 1 < C) thr[j] = order_refine(thr[j], bit, below[trip][j], order_rank(j + 1, n, C));
    }

    if (tid == 0) {
#pragma unroll
        for (uint32_t j = 0; j < kOrderMaxClasses; ++j) thrShared[j] = thr[j];
    }
    __syncthreads();

    // class sizes, then the stable emission: 256 slots per trip, in slot order
    for (uint32_t base = 0; base < n; base += kOrderThreads) {
        const uint32_t k = base + tid;
        const uint32_t c = k < n ? order_class(value(k), thrShared, C) : ~0u;
        for (uint32_t cc = 0; cc < C; ++cc) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(c == cc));
            if (lane == 0 && cnt != 0u) atomicAdd(&total[cc], cnt);
        }
    }
    __syncthreads();
    uint32_t it = 0;
    for (uint32_t base = 0; base < n; base += kOrderThreads, ++it) {
        const uint32_t k = base + tid, buf = it & 1u;
        const uint32_t c = k < n ? order_class(value(k), thrShared, C) : ~0u;
        uint32_t rankInWave = 0;
        for (uint32_t cc = 0; cc < C; ++cc) {
            const uint64_t b = __ballot(c == cc);
            if (c == cc) rankInWave = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) waveCnt[buf][wave][cc] = (uint32_t)__popcll(b);
        }
        __syncthreads();
        if (k < n) {
            uint32_t pos = run[c] + rankInWave;
            for (uint32_t cc = c + 1; cc < C; ++cc) pos += total[cc];               // the longer classes go first
            for (uint32_t w = 0; w < wave; ++w) pos += waveCnt[buf][w][c];
            if (pos < n) order[pos * kXcds + xcd] = k * kXcds + xcd;                // (pos < n by construction)
        }
        __syncthreads();
        if (tid < C) { uint32_t s = 0; for (uint32_t w = 0; w < kOrderWaves; ++w) s += waveCnt[buf][w][tid]; run[tid] += s; }
    }
    __syncthreads();
    for (uint32_t k = tid; k < n; k += kOrderThreads) steps[k * kXcds + xcd] = 0u;
}

// the builder for the launch `a` describes (a.map.order / a.map.steps bound, both of at least a.map.chunk * 8 words)
int launch_order_build(const K1Args& a, uint32_t classes, hipStream_t s) {
    uint32_t* order = const_cast<uint32_t*>(a.map.order);
    uint32_t* steps = a.map.steps;
    uint32_t words = a.map.chunk * kXcds;
    void* args[] = { &steps, &words, &classes, &order };
    MRIRT_HIP(hipLaunchKernel(reinterpret_cast<const void*>(order_build_kernel), dim3(kXcds), dim3(kOrderThreads), args, 0, s));
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

// the builder's table for the same record, computed on the host
extern "C" int mrirt_order_build_host(const uint32_t* steps, uint32_t words, uint32_t classes, uint32_t* order) {
    if (words != 0 && (!steps || !order)) return MRIRT_ERR_NULL;
    order_build_table(steps, words, classes, order);
    return MRIRT_OK;
}
