// Connected components of a label volume (6, 18 or 26 neighbours), their sizes, the small-component filter and the slice
// counts of the notebook's consistency score.  What a thread does to the parent array — the inside rule, the forward
// neighbours, the union-find, the numbering's encodings — and the scratch layout are csrc/cc_index.h (shared with the host
// harness); this file is the staging in LDS, the prefix sums and the entry points.
//
// mrirt_cc_label, on one stream, nothing synchronises with the host and no workgroup waits for another:
//   local     one workgroup per 8 x 8 x 32 tile labels the tile in LDS and writes each voxel's tile root (-1: outside)
//   merge     every voxel on a tile's rim unites with its forward neighbours in other tiles (agent-scope atomics only)
//   flatten   every voxel points at its root
//   number    roots per 1024-element chunk, reduce-then-scan over the chunk sums in separate launches (the scheme of
//             csrc/surface.hip on uint32 sums: a second copy, surface.hip's object code stays what it was), N, then three
//             launches: roots take -(k) - 1, non-roots read their root's, every negative entry flips
#include "cc_index.h"
#include "mrirt_host.h"

namespace mrirt {

// exclusive prefix of x over the workgroup's threads (and the sum over all of them); lds: kCcThreads elements
__device__ __forceinline__ uint32_t cc_block_scan(uint32_t x, uint32_t* lds, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    // ends: off doubles up to kCcThreads (kCcThreads - off strictly decreases)
    for (uint32_t off = 1; off < kCcThreads; off <<= 1) {
        uint32_t y = 0;
        if (t >= off) y = lds[t - off];
        __syncthreads();
        lds[t] += y;
        __syncthreads();
    }
    *total = lds[kCcThreads - 1];
    const uint32_t excl = t > 0 ? lds[t - 1] : 0u;
    __syncthreads();                                    // lds may be reused by the caller
    return excl;
}

__global__ __launch_bounds__(kCcThreads) void cc_local_kernel(const CcGeom g, const int16_t* labels, uint32_t classMask,
                                                              uint32_t connectivity, int32_t* parent) {
    __shared__ int32_t tile[kCcTileVox];
    // ends: numTiles - tileId strictly decreases (gridDim.x >= 1) and the loop stops when it is <= 0
    for (uint32_t tileId = blockIdx.x; tileId < g.numTiles; tileId += gridDim.x) {
        uint32_t o[3];
        cc_tile_origin(g, tileId, o);
        cc_tile_load(g, labels, classMask, o, tile, threadIdx.x);
        __syncthreads();
        cc_tile_link(connectivity, tile, threadIdx.x);
        __syncthreads();
        int32_t root[kCcPerThread];
        cc_tile_roots(tile, threadIdx.x, root);
        cc_tile_store(g, o, root, parent, threadIdx.x);
        __syncthreads();                                 // the next tile overwrites the LDS
    }
}

__global__ __launch_bounds__(kCcThreads) void cc_merge_kernel(const CcGeom g, uint32_t connectivity, int32_t* parent) {
    // ends: as in cc_local_kernel
    for (uint32_t tileId = blockIdx.x; tileId < g.numTiles; tileId += gridDim.x) {
        uint32_t o[3];
        cc_tile_origin(g, tileId, o);
        cc_merge_thread(g, connectivity, o, parent, threadIdx.x);
    }
}

// element j * kCcThreads + t of chunk blockIdx.x, j < kCcItems: consecutive threads, consecutive elements
#define CC_FOR_CHUNK_ELEMENTS(i, total)                                                                   \
    for (uint32_t j_ = 0, i = blockIdx.x * kCcChunk + threadIdx.x; j_ < kCcItems; ++j_, i += kCcThreads)  \
        if (i < (total))

__global__ __launch_bounds__(kCcThreads) void cc_flatten_kernel(int32_t* parent, uint32_t total) {
    CC_FOR_CHUNK_ELEMENTS(i, total) cc_flatten_element(parent, i);
}

// the roots among a thread's kCcItems consecutive elements, bit i for element base + i
__device__ __forceinline__ uint32_t cc_thread_roots(const int32_t* parent, uint32_t total, uint32_t base) {
    uint32_t bits = 0;
    for (uint32_t i = 0; i < kCcItems; ++i)
        if (base + i < total) bits |= cc_is_root(parent, base + i) << i;
    return bits;
}

__global__ __launch_bounds__(kCcThreads) void cc_count_roots_kernel(const int32_t* parent, uint32_t total, uint32_t* sums) {
    __shared__ uint32_t lds[kCcThreads];
    const uint32_t bits = cc_thread_roots(parent, total, blockIdx.x * kCcChunk + threadIdx.x * kCcItems);
    uint32_t sum;
    cc_block_scan((uint32_t)__popc(bits), lds, &sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kCcThreads) void cc_reduce_level_kernel(const uint32_t* in, uint32_t n, uint32_t* out) {
    __shared__ uint32_t lds[kCcThreads];
    const uint32_t base = blockIdx.x * kCcChunk + threadIdx.x * kCcItems;
    uint32_t s = 0;
    for (uint32_t i = 0; i < kCcItems; ++i)
        if (base + i < n) s += in[base + i];
    uint32_t sum;
    cc_block_scan(s, lds, &sum);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// data[n] -> its exclusive prefixes, in place, chunk by chunk (a thread rewrites only the elements it read itself);
// offsets: the (already scanned) level above, or nullptr for the top level (one workgroup), which also writes count[0] = N
__global__ __launch_bounds__(kCcThreads) void cc_scan_level_kernel(uint32_t* data, uint32_t n, const uint32_t* offsets, int64_t* count) {
    __shared__ uint32_t lds[kCcThreads];
    const uint32_t base = blockIdx.x * kCcChunk + threadIdx.x * kCcItems;
    uint32_t item[kCcItems], s = 0;
    for (uint32_t i = 0; i < kCcItems; ++i) {
        item[i] = base + i < n ? data[base + i] : 0u;
        s += item[i];
    }
    uint32_t sum;
    uint32_t run = cc_block_scan(s, lds, &sum);
    if (offsets != nullptr) run += offsets[blockIdx.x];
    for (uint32_t i = 0; i < kCcItems; ++i) {
        if (base + i < n) data[base + i] = run;
        run += item[i];
    }
    if (count != nullptr && threadIdx.x == 0) count[0] = (int64_t)sum;
}

// roots write their encoded number into their own entry (nothing else is read or written)
__global__ __launch_bounds__(kCcThreads) void cc_mark_roots_kernel(int32_t* parent, uint32_t total, const uint32_t* offsets) {
    __shared__ uint32_t lds[kCcThreads];
    const uint32_t base = blockIdx.x * kCcChunk + threadIdx.x * kCcItems;
    const uint32_t bits = cc_thread_roots(parent, total, base);
    uint32_t sum;
    uint32_t k = offsets[blockIdx.x] + cc_block_scan((uint32_t)__popc(bits), lds, &sum);
    for (uint32_t i = 0; i < kCcItems; ++i)
        if ((bits >> i) & 1u) parent[base + i] = cc_encode_number(++k);
}

__global__ __launch_bounds__(kCcThreads) void cc_spread_kernel(int32_t* parent, uint32_t total) {
    CC_FOR_CHUNK_ELEMENTS(i, total) cc_spread_element(parent, i);
}

__global__ __launch_bounds__(kCcThreads) void cc_flip_kernel(int32_t* parent, uint32_t total) {
    CC_FOR_CHUNK_ELEMENTS(i, total) cc_flip_element(parent, i);
}

__global__ __launch_bounds__(kCcThreads) void cc_sizes_kernel(const int32_t* components, uint32_t total, uint32_t chunks, int64_t nComponents,
                                                              int32_t* sizes) {
    __shared__ int32_t tags[kCcSizeSlots], counts[kCcSizeSlots];
    static_assert(kCcSizeSlots <= kCcThreads, "one thread per slot");
    if (threadIdx.x < kCcSizeSlots) { tags[threadIdx.x] = 0; counts[threadIdx.x] = 0; }
    __syncthreads();
    for (uint32_t q = 0; q < kCcSizeChunks; ++q) {
        const uint32_t chunk = blockIdx.x * kCcSizeChunks + q;
        if (chunk < chunks) cc_sizes_thread(components, total, nComponents, tags, counts, sizes, chunk * kCcChunk + threadIdx.x * kCcItems);
    }
    __syncthreads();
    if (threadIdx.x < kCcSizeSlots) cc_sizes_flush(tags, counts, sizes, threadIdx.x);
}

__global__ __launch_bounds__(kCcThreads) void cc_filter_kernel(const int16_t* labels, const int32_t* components, const int32_t* sizes,
                                                               int64_t nComponents, uint32_t total, uint32_t chunks, int64_t minVoxels,
                                                               uint32_t keepLargest, int16_t fill, int16_t* out) {
    __shared__ unsigned long long lds[kCcThreads];
    unsigned long long best = 0;
    if (keepLargest != 0u) {                             // the same in every thread
        // ends: nComponents - k strictly decreases and the loop stops when it is <= 0
        for (int64_t k = threadIdx.x; k < nComponents; k += kCcThreads) {
            const unsigned long long key = cc_size_key(sizes[k], (uint32_t)k);
            best = key > best ? key : best;
        }
        lds[threadIdx.x] = best;
        __syncthreads();
        // ends: off halves down to 0
        for (uint32_t off = kCcThreads / 2; off > 0; off >>= 1) {
            if (threadIdx.x < off && lds[threadIdx.x + off] > lds[threadIdx.x]) lds[threadIdx.x] = lds[threadIdx.x + off];
            __syncthreads();
        }
        best = lds[0];
    }
    // ends: chunks - chunk strictly decreases (gridDim.x >= 1) and the loop stops when it is <= 0
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x)
        for (uint32_t j = 0, i = chunk * kCcChunk + threadIdx.x; j < kCcItems; ++j, i += kCcThreads)
            if (i < total) out[i] = cc_filter_value(labels[i], components[i], sizes, nComponents, minVoxels, keepLargest, best, fill);
}

// block b: indices [32 (b % zsegs), +32) of the last axis, rows [256 (b / zsegs), +256); thread t: index t % 32, rows t / 32 + 8 m
__global__ __launch_bounds__(kCcThreads) void cc_slice_counts_kernel(const int16_t* labels, uint32_t rows, uint32_t n2, uint32_t zsegs,
                                                                     uint32_t blocks, unsigned long long* counts) {
    __shared__ uint32_t lds[kCcSliceZ * 3];
    constexpr uint32_t kGroups = kCcThreads / kCcSliceZ;
    const uint32_t zl = threadIdx.x % kCcSliceZ, rg = threadIdx.x / kCcSliceZ;
    // ends: blocks - b strictly decreases (gridDim.x >= 1) and the loop stops when it is <= 0
    for (uint32_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        if (threadIdx.x < kCcSliceZ * 3) lds[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t z0 = (b % zsegs) * kCcSliceZ, z = z0 + zl, row0 = (b / zsegs) * kCcSliceRows;
        uint32_t a = 0, in = 0, un = 0;
        if (z < n2) {
            for (uint32_t m = 0; m < kCcSliceRows / kGroups; ++m) {
                const uint32_t row = row0 + rg + m * kGroups;
                if (row >= rows) break;
                const uint32_t v = row * n2 + z;
                const uint32_t f = cc_slice_flags(labels[v], z > 0 ? labels[v - 1] : (int16_t)0, z > 0);
                a += f & 1u; in += (f >> 1) & 1u; un += f >> 2;
            }
            if (a) atomicAdd(&lds[zl * 3 + 0], a);
            if (in) atomicAdd(&lds[zl * 3 + 1], in);
            if (un) atomicAdd(&lds[zl * 3 + 2], un);
        }
        __syncthreads();
        if (threadIdx.x < kCcSliceZ * 3 && z0 + threadIdx.x / 3 < n2 && lds[threadIdx.x] != 0u)
            atomicAdd(&counts[(size_t)z0 * 3 + threadIdx.x], (unsigned long long)lds[threadIdx.x]);
        __syncthreads();                                 // the next block's zeroing
    }
}

static int cc_label_stages(const CcPlan& p, const int16_t* labels, uint32_t classMask, uint32_t connectivity, int32_t* parent,
                           int64_t* count, char* base, hipStream_t s) {
    const CcGeom& g = p.g;
    uint32_t* level[kCcMaxLevels];
    for (uint32_t l = 0; l < p.levels; ++l) level[l] = reinterpret_cast<uint32_t*>(base + p.level[l]);
    const dim3 block(kCcThreads), tiles(g.numTiles < kCcMaxGrid ? g.numTiles : kCcMaxGrid), chunks(p.count[0]);
    hipLaunchKernelGGL(cc_local_kernel, tiles, block, 0, s, g, labels, classMask, connectivity, parent);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_merge_kernel, tiles, block, 0, s, g, connectivity, parent);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_flatten_kernel, chunks, block, 0, s, parent, g.total);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_count_roots_kernel, chunks, block, 0, s, (const int32_t*)parent, g.total, level[0]);
    MRIRT_HIP(hipGetLastError());
    for (uint32_t l = 1; l < p.levels; ++l) {
        hipLaunchKernelGGL(cc_reduce_level_kernel, dim3(p.count[l]), block, 0, s, (const uint32_t*)level[l - 1], p.count[l - 1], level[l]);
        MRIRT_HIP(hipGetLastError());
    }
    const uint32_t top = p.levels - 1;
    hipLaunchKernelGGL(cc_scan_level_kernel, dim3(1), block, 0, s, level[top], p.count[top], (const uint32_t*)nullptr, count);
    MRIRT_HIP(hipGetLastError());
    for (uint32_t l = top; l-- > 0;) {
        hipLaunchKernelGGL(cc_scan_level_kernel, dim3(p.count[l + 1]), block, 0, s, level[l], p.count[l], (const uint32_t*)level[l + 1],
                           (int64_t*)nullptr);
        MRIRT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(cc_mark_roots_kernel, chunks, block, 0, s, parent, g.total, (const uint32_t*)level[0]);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_spread_kernel, chunks, block, 0, s, parent, g.total);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_flip_kernel, chunks, block, 0, s, parent, g.total);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_cc_scratch_bytes(const uint32_t hwd[3]) {
    CcPlan p;
    if (!hwd || cc_plan(hwd, &p) != 0) return 0;
    return p.total;
}

extern "C" int mrirt_cc_label(const int16_t* labels, const uint32_t hwd[3], uint32_t class_mask, uint32_t connectivity,
                              int32_t* components, int64_t* count_dev, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!labels || !hwd || !components || !count_dev || !scratch) return MRIRT_ERR_NULL;
    CcPlan p;
    const int rc = cc_plan(hwd, &p);
    if (rc != MRIRT_OK) return rc;
    if (connectivity < 1 || connectivity > 3) return MRIRT_ERR_ARG;
    if (scratch_bytes < p.total || (reinterpret_cast<uintptr_t>(scratch) & 15u) != 0u) return MRIRT_ERR_ARG;
    return cc_label_stages(p, labels, class_mask, connectivity, components, count_dev, static_cast<char*>(scratch),
                           static_cast<hipStream_t>(stream));
}

extern "C" int mrirt_cc_sizes(const int32_t* components, const uint32_t hwd[3], int64_t n_components, int32_t* sizes, void* stream) {
    if (!components || !hwd || (!sizes && n_components > 0)) return MRIRT_ERR_NULL;
    CcGeom g;
    const int rc = cc_geom(hwd, &g);
    if (rc != MRIRT_OK) return rc;
    if (n_components < 0 || n_components > (int64_t)g.total) return MRIRT_ERR_ARG;
    if (n_components == 0) return MRIRT_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    MRIRT_HIP(hipMemsetAsync(sizes, 0, (size_t)n_components * sizeof(int32_t), s));
    const uint32_t chunks = (g.total + kCcChunk - 1) / kCcChunk;
    hipLaunchKernelGGL(cc_sizes_kernel, dim3((chunks + kCcSizeChunks - 1) / kCcSizeChunks), dim3(kCcThreads), 0, s, components, g.total,
                       chunks, n_components, sizes);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_cc_filter(const int16_t* labels, const int32_t* components, const int32_t* sizes, int64_t n_components,
                               const uint32_t hwd[3], int64_t min_voxels, int32_t keep_largest, int16_t fill, int16_t* out, void* stream) {
    if (!labels || !components || !hwd || !out || (!sizes && n_components > 0)) return MRIRT_ERR_NULL;
    CcGeom g;
    const int rc = cc_geom(hwd, &g);
    if (rc != MRIRT_OK) return rc;
    if (n_components < 0 || n_components > (int64_t)g.total || min_voxels < 0 || (keep_largest != 0 && keep_largest != 1)) return MRIRT_ERR_ARG;
    const uint32_t chunks = (g.total + kCcChunk - 1) / kCcChunk;
    hipLaunchKernelGGL(cc_filter_kernel, dim3(chunks < kCcFilterGrid ? chunks : kCcFilterGrid), dim3(kCcThreads), 0,
                       static_cast<hipStream_t>(stream), labels, components, sizes, n_components, g.total, chunks, min_voxels,
                       (uint32_t)keep_largest, fill, out);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_slice_counts(const int16_t* labels, const uint32_t hwd[3], int64_t* counts, void* stream) {
    if (!labels || !hwd || !counts) return MRIRT_ERR_NULL;
    CcGeom g;
    const int rc = cc_geom(hwd, &g);
    if (rc != MRIRT_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t rows = g.n[0] * g.n[1], n2 = g.n[2];
    const uint32_t zsegs = (n2 + kCcSliceZ - 1) / kCcSliceZ, blocks = zsegs * ((rows + kCcSliceRows - 1) / kCcSliceRows);   // <= total
    MRIRT_HIP(hipMemsetAsync(counts, 0, (size_t)n2 * 3 * sizeof(int64_t), s));
    hipLaunchKernelGGL(cc_slice_counts_kernel, dim3(blocks < kCcMaxGrid ? blocks : kCcMaxGrid), dim3(kCcThreads), 0, s, labels, rows, n2,
                       zsegs, blocks, reinterpret_cast<unsigned long long*>(counts));
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
