// Class surfaces of a label volume by naive surface nets: a watertight, outward-oriented triangle mesh in the frame of the
// K1 volume, ready for K4.  What a cell contributes — its corner mask, its vertex, the quads it owns and their winding — and
// the scratch layout are csrc/surface_cells.h (shared with the host harness); this file is the staging of the labels in LDS,
// the prefix sums and the entry points.
//
// Three stages on one stream, nothing synchronises with the host:
//   classify   one workgroup per 4 x 4 x 64 tile of cells stages the tile's 5 x 5 x 65 voxels as inside flags (every label
//              is read once per tile, not eight times) and writes one corner mask per cell
//   scan       reduce-then-scan over the cells in linear order, in separate launches: per-chunk sums of (vertex flag, owned
//              quads) upwards until one chunk holds a level, one workgroup scans that level and writes the totals, then
//              every level below is scanned in place with its chunk's offset.  No workgroup ever waits for another one.
//   emit       a chunk's workgroup scans its cells once more (from the masks), adds the chunk's offset, and writes the
//              vertices and vertex numbers (first launch), then the triangles (second launch: a quad reads the vertex
//              numbers of four cells)
#include "surface_cells.h"
#include "mrirt_host.h"

namespace mrirt {

// exclusive prefix of x over the workgroup's threads (and the sum over all of them); lds: kSurfThreads elements
template <class T>
__device__ __forceinline__ T surf_block_scan(T x, T* lds, T* total) {
    const uint32_t t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    for (uint32_t off = 1; off < kSurfThreads; off <<= 1) {
        T y = T{};
        if (t >= off) y = lds[t - off];
        __syncthreads();
        lds[t] = lds[t] + y;
        __syncthreads();
    }
    *total = lds[kSurfThreads - 1];
    const T excl = t > 0 ? lds[t - 1] : T{};
    __syncthreads();                                    // lds may be reused by the caller
    return excl;
}

// the kSurfItems consecutive cells of a thread: their masks, coordinates and packed counts (surf_cell_counts; 0 past the end)
struct SurfThreadCells {
    uint32_t base, mask[kSurfItems], counts[kSurfItems], c[kSurfItems][3], sum;
};

__device__ __forceinline__ SurfThreadCells surf_thread_cells(const SurfGeom& g, const uint8_t* code) {
    SurfThreadCells r;
    r.base = blockIdx.x * kSurfChunk + threadIdx.x * kSurfItems;
    r.sum = 0;
    const uint32_t word = reinterpret_cast<const uint32_t*>(code)[r.base / 4];      // code is padded to whole chunks
    uint32_t c[3];
    surf_cell_coords(g, r.base, c);
    for (uint32_t i = 0; i < kSurfItems; ++i) {
        r.mask[i] = (word >> (8 * i)) & 255u;
        for (int k = 0; k < 3; ++k) r.c[i][k] = c[k];
        r.counts[i] = r.base + i < g.cells ? surf_cell_counts(r.mask[i], c) : 0u;
        r.sum += r.counts[i];
        if (++c[2] == g.nc[2]) {
            c[2] = 0;
            if (++c[1] == g.nc[1]) { c[1] = 0; ++c[0]; }
        }
    }
    return r;
}

__global__ __launch_bounds__(kSurfThreads) void surf_classify_kernel(const SurfGeom g, const int16_t* labels, uint32_t classMask,
                                                                     uint8_t* code) {
    __shared__ uint8_t tile[kSurfTileBytes];
    uint32_t o[3];
    surf_tile_origin(g, blockIdx.x, o);
    surf_tile_load(g, labels, classMask, o, tile, threadIdx.x, kSurfThreads);
    __syncthreads();
    surf_tile_classify(g, o, tile, code, threadIdx.x);
}

__global__ __launch_bounds__(kSurfThreads) void surf_reduce_cells_kernel(const SurfGeom g, const uint8_t* code, SurfCount* sums) {
    __shared__ uint32_t lds[kSurfThreads];
    const SurfThreadCells tc = surf_thread_cells(g, code);
    uint32_t total;
    surf_block_scan(tc.sum, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = SurfCount{ total & 0xFFFFu, total >> 16 };
}

__global__ __launch_bounds__(kSurfThreads) void surf_reduce_level_kernel(const SurfCount* in, uint32_t n, SurfCount* out) {
    __shared__ SurfCount lds[kSurfThreads];
    const uint32_t base = blockIdx.x * kSurfChunk + threadIdx.x * kSurfItems;
    SurfCount s{};
    for (uint32_t i = 0; i < kSurfItems; ++i)
        if (base + i < n) s = s + in[base + i];
    SurfCount total;
    surf_block_scan(s, lds, &total);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

// data[n] -> its exclusive prefixes, in place, chunk by chunk; offsets: the (already scanned) level above, or nullptr for the
// top level (one workgroup), which also writes counts = { V, T = 2 * quads }
__global__ __launch_bounds__(kSurfThreads) void surf_scan_level_kernel(SurfCount* data, uint32_t n, const SurfCount* offsets,
                                                                       int64_t* counts) {
    __shared__ SurfCount lds[kSurfThreads];
    const uint32_t base = blockIdx.x * kSurfChunk + threadIdx.x * kSurfItems;
    SurfCount item[kSurfItems], s{};
    for (uint32_t i = 0; i < kSurfItems; ++i) {
        item[i] = base + i < n ? data[base + i] : SurfCount{};
        s = s + item[i];
    }
    SurfCount total;
    SurfCount run = surf_block_scan(s, lds, &total);
    if (offsets != nullptr) run = run + offsets[blockIdx.x];
    for (uint32_t i = 0; i < kSurfItems; ++i) {
        if (base + i < n) data[base + i] = run;
        run = run + item[i];
    }
    if (counts != nullptr && threadIdx.x == 0) {
        counts[0] = (int64_t)total.v;
        counts[1] = (int64_t)(2 * total.q);
    }
}

struct SurfEmitArgs {
    SurfGeom g;
    const uint8_t* code;
    const SurfCount* offsets;      // exclusive prefix per chunk of cells
    const int64_t* counts;         // { V, T }, written earlier on this stream
    uint32_t* vidx;
    float* verts;
    int32_t* tris;
    int64_t vertCap, triCap;
    float spacing[3], origin[3];
};

__device__ __forceinline__ bool surf_fits(const SurfEmitArgs& a) { return a.counts[0] <= a.vertCap && a.counts[1] <= a.triCap; }

__global__ __launch_bounds__(kSurfThreads) void surf_emit_verts_kernel(const SurfEmitArgs a) {
    __shared__ uint32_t lds[kSurfThreads];
    if (!surf_fits(a)) return;                           // the same in every thread
    const SurfThreadCells tc = surf_thread_cells(a.g, a.code);
    uint32_t total;
    const uint32_t excl = surf_block_scan(tc.sum, lds, &total);
    if ((total & 0xFFFFu) == 0u) return;
    unsigned long long v = a.offsets[blockIdx.x].v + (excl & 0xFFFFu);
    for (uint32_t i = 0; i < kSurfItems; ++i) {
        if ((tc.counts[i] & 1u) == 0u) continue;
        float x[3];
        surf_vertex(tc.mask[i], tc.c[i], a.spacing, a.origin, x);
        a.vidx[tc.base + i] = (uint32_t)v;
        float* dst = a.verts + 3 * v;
        dst[0] = x[0]; dst[1] = x[1]; dst[2] = x[2];
        ++v;
    }
}

__global__ __launch_bounds__(kSurfThreads) void surf_emit_tris_kernel(const SurfEmitArgs a) {
    __shared__ uint32_t lds[kSurfThreads];
    if (!surf_fits(a)) return;
    const SurfThreadCells tc = surf_thread_cells(a.g, a.code);
    uint32_t total;
    const uint32_t excl = surf_block_scan(tc.sum, lds, &total);
    if ((total >> 16) == 0u) return;
    unsigned long long q = a.offsets[blockIdx.x].q + (excl >> 16);
    for (uint32_t i = 0; i < kSurfItems; ++i) {
        if ((tc.counts[i] >> 16) == 0u) continue;
        const uint32_t axes = surf_quad_axes(tc.mask[i], tc.c[i]);
        for (int ax = 0; ax < 3; ++ax) {
            if (((axes >> ax) & 1u) == 0u) continue;
            int32_t tri[6];
            surf_quad(a.g, ax, tc.mask[i], tc.base + i, a.vidx, tri);
            int32_t* dst = a.tris + 6 * q;
            for (int k = 0; k < 6; ++k) dst[k] = tri[k];
            ++q;
        }
    }
}

// classify + the prefix sums: leaves the masks in code, the chunks' exclusive prefixes in level 0 and { V, T } in counts
static int surf_count_stages(const SurfPlan& p, const int16_t* labels, uint32_t classMask, char* base, int64_t* counts, hipStream_t s) {
    uint8_t* code = reinterpret_cast<uint8_t*>(base + p.code);
    SurfCount* level[kSurfMaxLevels];
    for (uint32_t l = 0; l < p.levels; ++l) level[l] = reinterpret_cast<SurfCount*>(base + p.level[l]);
    const dim3 block(kSurfThreads);
    hipLaunchKernelGGL(surf_classify_kernel, dim3(p.g.tiles[0] * p.g.tiles[1] * p.g.tiles[2]), block, 0, s, p.g, labels, classMask, code);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(surf_reduce_cells_kernel, dim3(p.count[0]), block, 0, s, p.g, code, level[0]);
    MRIRT_HIP(hipGetLastError());
    for (uint32_t l = 1; l < p.levels; ++l) {
        hipLaunchKernelGGL(surf_reduce_level_kernel, dim3(p.count[l]), block, 0, s, level[l - 1], p.count[l - 1], level[l]);
        MRIRT_HIP(hipGetLastError());
    }
    const uint32_t top = p.levels - 1;
    hipLaunchKernelGGL(surf_scan_level_kernel, dim3(1), block, 0, s, level[top], p.count[top], (const SurfCount*)nullptr, counts);
    MRIRT_HIP(hipGetLastError());
    for (uint32_t l = top; l-- > 0;) {
        hipLaunchKernelGGL(surf_scan_level_kernel, dim3(p.count[l + 1]), block, 0, s, level[l], p.count[l], (const SurfCount*)level[l + 1],
                           (int64_t*)nullptr);
        MRIRT_HIP(hipGetLastError());
    }
    return MRIRT_OK;
}

static int surf_check(const uint32_t hwd[3], const void* scratch, int64_t scratchBytes, SurfPlan* p) {
    const int rc = surf_plan(hwd, p);
    if (rc != MRIRT_OK) return rc;
    if (scratchBytes < p->total || (reinterpret_cast<uintptr_t>(scratch) & 15u) != 0u) return MRIRT_ERR_ARG;
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_surface_scratch_bytes(const uint32_t hwd[3]) {
    SurfPlan p;
    if (!hwd || surf_plan(hwd, &p) != 0) return 0;
    return p.total;
}

extern "C" int mrirt_surface_count(const int16_t* labels, const uint32_t hwd[3], uint32_t class_mask, void* scratch,
                                   int64_t scratch_bytes, int64_t* counts_dev, void* stream) {
    if (!labels || !hwd || !scratch || !counts_dev) return MRIRT_ERR_NULL;
    SurfPlan p;
    const int rc = surf_check(hwd, scratch, scratch_bytes, &p);
    if (rc != MRIRT_OK) return rc;
    return surf_count_stages(p, labels, class_mask, static_cast<char*>(scratch), counts_dev, static_cast<hipStream_t>(stream));
}

extern "C" int mrirt_surface_extract(const int16_t* labels, const uint32_t hwd[3], uint32_t class_mask, const float spacing[3],
                                     const float origin[3], float* verts, int64_t vert_cap, int32_t* tris, int64_t tri_cap,
                                     void* scratch, int64_t scratch_bytes, int64_t* counts_dev, void* stream) {
    if (!labels || !hwd || !spacing || !origin || !scratch || !counts_dev) return MRIRT_ERR_NULL;
    if ((!verts && vert_cap != 0) || (!tris && tri_cap != 0)) return MRIRT_ERR_NULL;
    if (vert_cap < 0 || tri_cap < 0) return MRIRT_ERR_ARG;
    SurfPlan p;
    int rc = surf_check(hwd, scratch, scratch_bytes, &p);
    if (rc == MRIRT_OK) rc = surf_check_frame(spacing, origin);
    if (rc != MRIRT_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    rc = surf_count_stages(p, labels, class_mask, base, counts_dev, s);
    if (rc != MRIRT_OK) return rc;
    // a surface has vertices and triangles or neither: with room for none of one kind there is no geometry to write
    if (vert_cap == 0 || tri_cap == 0) return MRIRT_OK;
    SurfEmitArgs a;
    a.g = p.g;
    a.code = reinterpret_cast<const uint8_t*>(base + p.code);
    a.offsets = reinterpret_cast<const SurfCount*>(base + p.level[0]);
    a.counts = counts_dev;
    a.vidx = reinterpret_cast<uint32_t*>(base + p.vidx);
    a.verts = verts; a.tris = tris;
    a.vertCap = vert_cap; a.triCap = tri_cap;
    for (int k = 0; k < 3; ++k) { a.spacing[k] = spacing[k]; a.origin[k] = origin[k]; }
    hipLaunchKernelGGL(surf_emit_verts_kernel, dim3(p.count[0]), dim3(kSurfThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(surf_emit_tris_kernel, dim3(p.count[0]), dim3(kSurfThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
