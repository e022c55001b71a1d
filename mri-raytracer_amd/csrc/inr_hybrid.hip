// The hybrid, uncertainty-guided sampler of the reference's notebooks/improved.ipynb (cell 9) and its coordinate noise (cell 12);
// DESIGN.md section 26.  The entropy it ranks by is mrirt_inject_uncertainty's (csrc/inr_inject.hip).
//   cls_count_kernel        voxels per (case, class): one LDS histogram per block, one integer atomic per (block, class)
//   cls_chunk_kernel        voxels per (case, chunk of 4096, class)
//   cls_scan_kernel         ... scanned over the chunks of a (case, class), in a launch of its own
//   cls_emit_kernel         the ascending voxel offsets of every (class, case): no workgroup waits for another, no atomic append
//   select_largest_kernel   the k largest of n <= 65536 values in ONE workgroup: an MSD radix select of the k-th key over LDS
//                           histograms, then a workgroup scan and the emit in ascending index order
//   normal3_kernel          the unit normals of the coordinate noise
//   candidates_kernel       the candidate voxels the uncertainty is computed on
//   sample_hybrid_kernel    one micro-batch: picked candidates, class-balanced voxels, uniform voxels; labels, modalities, a
//                           per-voxel field (the boundary weights) and the noise on the coordinates in the same launch
// Integer atomics only, one writer per element: the same inputs give the same bits.
#include "inr_device.h"
#include "inr_hybrid.h"
#include "mrirt_host.h"

namespace mrirt {

struct ClsArgs {
    const int16_t* const* seg;
    uint64_t hwd;
    uint32_t ncases, chunks, C;
    unsigned long long* counts;  // [ncases][C]
    uint32_t* chunkSums;         // [ncases][chunks][C]
    const int64_t* offsets;
    uint32_t* index;
};

// this thread's voxels of `chunk` into the block's histogram (LDS integer atomics: a sum has no order)
__device__ __forceinline__ void cls_tally(const int16_t* seg, uint32_t chunk, uint64_t hwd, uint32_t C, uint32_t* hist) {
    const uint64_t first = tum_first(chunk, threadIdx.x);
    for (uint32_t j = 0; j < kTumPerThread; ++j) {
        const uint64_t v = first + j;
        if (v < hwd) {
            const int16_t lab = seg[v];
            if (cls_in(lab, C)) atomicAdd(&hist[lab], 1u);
        }
    }
}

// grid (x, ncases): block x of a case strides over its chunks
__global__ __launch_bounds__(kTumThreads) void cls_count_kernel(ClsArgs a) {
    __shared__ uint32_t hist[kLossMaxClasses];
    __shared__ unsigned long long total[kLossMaxClasses];
    const int16_t* seg = a.seg[blockIdx.y];
    if (threadIdx.x < kLossMaxClasses) total[threadIdx.x] = 0;
    for (uint32_t chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        if (threadIdx.x < kLossMaxClasses) hist[threadIdx.x] = 0;
        __syncthreads();
        cls_tally(seg, chunk, a.hwd, a.C, hist);
        __syncthreads();
        if (threadIdx.x < a.C) total[threadIdx.x] += hist[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < a.C && total[threadIdx.x]) atomicAdd(a.counts + (uint64_t)blockIdx.y * a.C + threadIdx.x, total[threadIdx.x]);
}

// grid (chunks, ncases)
__global__ __launch_bounds__(kTumThreads) void cls_chunk_kernel(ClsArgs a) {
    __shared__ uint32_t hist[kLossMaxClasses];
    if (threadIdx.x < kLossMaxClasses) hist[threadIdx.x] = 0;
    __syncthreads();
    cls_tally(a.seg[blockIdx.y], blockIdx.x, a.hwd, a.C, hist);
    __syncthreads();
    if (threadIdx.x < a.C) a.chunkSums[cls_chunk_slot(blockIdx.y, blockIdx.x, threadIdx.x, a.chunks, a.C)] = hist[threadIdx.x];
}

// grid (ncases, C): the chunk sums of a (case, class) -> their exclusive prefix, in place
__global__ __launch_bounds__(kTumThreads) void cls_scan_kernel(ClsArgs a) {
    __shared__ uint32_t lds[kTumThreads];
    const uint32_t len = tum_scan_len(a.chunks), first = threadIdx.x * len;
    uint32_t mine = 0;
    for (uint32_t j = first; j < first + len && j < a.chunks; ++j) mine += a.chunkSums[cls_chunk_slot(blockIdx.x, j, blockIdx.y, a.chunks, a.C)];
    lds[threadIdx.x] = mine;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) before += lds[t];
    for (uint32_t j = first; j < first + len && j < a.chunks; ++j) {
        uint32_t* s = a.chunkSums + cls_chunk_slot(blockIdx.x, j, blockIdx.y, a.chunks, a.C);
        const uint32_t c = *s;
        *s = before;
        before += c;
    }
}

// grid (chunks, ncases): class by class, thread t's voxels land behind those of threads < t of its chunk, behind the chunks before it
__global__ __launch_bounds__(kTumThreads) void cls_emit_kernel(ClsArgs a) {
    __shared__ uint32_t lds[kTumThreads];
    const int16_t* seg = a.seg[blockIdx.y];
    const uint64_t first = tum_first(blockIdx.x, threadIdx.x);
    int32_t lab[kTumPerThread];
#pragma unroll
    for (uint32_t j = 0; j < kTumPerThread; ++j) lab[j] = first + j < a.hwd ? (int32_t)seg[first + j] : -1;
    for (uint32_t k = 0; k < a.C; ++k) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < kTumPerThread; ++j) mine += lab[j] == (int32_t)k ? 1u : 0u;
        lds[threadIdx.x] = mine;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t t = 0; t < threadIdx.x; ++t) before += lds[t];
        __syncthreads();
        const uint32_t list = cls_list(k, blockIdx.y, a.ncases);
        const int64_t lo = a.offsets[list], hi = a.offsets[list + 1];
        int64_t at = lo + (int64_t)a.chunkSums[cls_chunk_slot(blockIdx.y, blockIdx.x, k, a.chunks, a.C)] + before;
#pragma unroll
        for (uint32_t j = 0; j < kTumPerThread; ++j) {
            if (lab[j] == (int32_t)k) {
                if (at >= lo && at < hi) a.index[at] = (uint32_t)(first + j);      // offsets that do not match the counts write nothing outside a list
                ++at;
            }
        }
    }
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------

// inclusive scan of one value per thread over the workgroup (Hillis-Steele on two LDS rows); every thread gets its inclusive
// sum, *total the workgroup's
__device__ __forceinline__ uint32_t sel_block_scan(uint32_t v, uint32_t (*rows)[kSelThreads], uint32_t* total) {
    uint32_t cur = 0;
    rows[0][threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kSelThreads; d <<= 1) {
        const uint32_t x = rows[cur][threadIdx.x] + (threadIdx.x >= d ? rows[cur][threadIdx.x - d] : 0u);
        rows[cur ^ 1u][threadIdx.x] = x;
        cur ^= 1u;
        __syncthreads();
    }
    const uint32_t mine = rows[cur][threadIdx.x];
    *total = rows[cur][kSelThreads - 1];
    __syncthreads();
    return mine;
}

// One workgroup.  The keys are not staged: every pass reads the values again (n <= 65536 floats stay in L2) and forms the key
// in registers.
__global__ __launch_bounds__(kSelThreads) void select_largest_kernel(const float* __restrict__ values, uint32_t n, uint32_t k,
                                                                     uint32_t* __restrict__ out) {
    __shared__ uint32_t hist[kSelBins];
    __shared__ uint32_t rows[2][kSelThreads];
    __shared__ uint32_t chosen[2];           // the digit of this pass, the keys above it
    const uint32_t t = threadIdx.x;
    uint32_t prefix = 0, need = k, equal = n;
    for (uint32_t pass = 0; pass < kSelPasses; ++pass) {
        const uint32_t shift = sel_shift(pass), mask = sel_mask(pass);
        if (t < kSelBins) hist[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += kSelThreads) {
            const uint32_t key = sel_key(values[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFFu], 1u);
        }
        __syncthreads();
        if (t < kSelBins) {
            const uint32_t above = sel_above(hist, t);
            if (sel_is_digit(above, hist[t], need)) { chosen[0] = t; chosen[1] = above; }
        }
        __syncthreads();
        prefix |= chosen[0] << shift;
        need -= chosen[1];
        equal = hist[chosen[0]];
        __syncthreads();
    }
    // prefix is the k-th largest key; `need` of the `equal` keys that match it are still wanted: the highest-indexed ones
    const uint32_t lo = sel_first(t, n), hi = sel_first(t + 1, n);
    uint32_t eq = 0;
    for (uint32_t i = lo; i < hi; ++i) eq += sel_key(values[i]) == prefix ? 1u : 0u;
    uint32_t total;
    uint32_t rank = sel_block_scan(eq, rows, &total) - eq;
    uint32_t take = 0, r = rank;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t key = sel_key(values[i]);
        take += sel_takes(key, prefix, r, equal, need) ? 1u : 0u;
        r += key == prefix ? 1u : 0u;
    }
    uint32_t at = sel_block_scan(take, rows, &total) - take;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t key = sel_key(values[i]);
        if (sel_takes(key, prefix, rank, equal, need)) {
            if (at < k) out[at] = i;
            ++at;
        }
        rank += key == prefix ? 1u : 0u;
    }
}

// ---- normals, candidates, the hybrid micro-batch -----------------------------------------------------------------------------------

__global__ __launch_bounds__(kOptThreads) void normal3_kernel(uint64_t seed, uint64_t batch, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (i >= n) return;
    const Normal3 z = nrm_point(seed, batch, (uint32_t)i);
    out[3 * i + 0] = z.x;
    out[3 * i + 1] = z.y;
    out[3 * i + 2] = z.z;
}

struct HybArgs {
    const float* const* mods;
    const int16_t* const* seg;
    const float* const* fields;
    uint32_t ncases, M, H, W, D, C;
    int64_t hwd;
    uint64_t seed, batch;
    int64_t n, U, P;
    const uint32_t* picks;
    const uint32_t* index;
    const int64_t* offsets;
    float sigma;
    float* coords;
    float* feats;
    int32_t* labels;
    float* fieldOut;
};

__global__ __launch_bounds__(kOptThreads) void candidates_kernel(HybArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (j >= a.n) return;
    const SamplePoint p = mix_uniform(hyb_words(a.seed, a.batch, (uint32_t)j, 1u), a.ncases, a.H, a.W, a.D);
    sample_write(j, p, a.mods, a.seg, a.M, a.H, a.W, a.D, a.hwd, a.coords, a.feats, a.labels);
}

__global__ __launch_bounds__(kOptThreads) void sample_hybrid_kernel(HybArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
    if (i >= a.n) return;
    const SamplePoint p = hyb_row(a.seed, a.batch, (uint32_t)i, a.U, a.P, a.C, a.picks, a.index, a.offsets, a.ncases, a.H, a.W, a.D, a.hwd);
    sample_write(i, p, a.mods, a.seg, a.M, a.H, a.W, a.D, a.hwd, a.coords, a.feats, a.labels);
    if (a.fields) a.fieldOut[i] = a.fields[p.cs][voxel_offset(p.x, p.y, p.z, a.W, a.D)];
    if (a.sigma > 0.0f) {
        const Normal3 z = nrm_point(a.seed, a.batch, (uint32_t)i);
        a.coords[3 * i + 0] = hyb_noise(sample_coord(p.x, a.H), a.sigma, z.x);
        a.coords[3 * i + 1] = hyb_noise(sample_coord(p.y, a.W), a.sigma, z.y);
        a.coords[3 * i + 2] = hyb_noise(sample_coord(p.z, a.D), a.sigma, z.z);
    }
}

// the cache checks of the tumour index, and C
static int cls_check(const MrirtInrCache* c, uint32_t C) {
    if (!c) return MRIRT_ERR_NULL;
    const uint64_t hw = (uint64_t)c->hwd[0] * c->hwd[1];                // < 2^64; hw < 2^32 keeps hw * D there too
    if (hw >= (1ull << 32) || hw * c->hwd[2] >= (1ull << 32)) return MRIRT_ERR_ARG;
    const int rc = opt_check_cache(c);
    if (rc != MRIRT_OK) return rc;
    return (C < 1 || C > kLossMaxClasses) ? MRIRT_ERR_ARG : MRIRT_OK;
}

static ClsArgs cls_args(const MrirtInrCache* c, uint32_t C) {
    ClsArgs a = {};
    a.seg = c->seg;
    a.hwd = (uint64_t)c->hwd[0] * c->hwd[1] * c->hwd[2];
    a.ncases = c->ncases;
    a.chunks = tum_chunks(a.hwd);
    a.C = C;
    return a;
}

static HybArgs hyb_args(const MrirtInrCache* cache, uint64_t seed, uint64_t batch, int64_t n, float* coords, float* feats, int32_t* labels) {
    HybArgs a = {};
    a.mods = cache->mods; a.seg = cache->seg; a.ncases = cache->ncases; a.M = cache->numMods;
    a.H = cache->hwd[0]; a.W = cache->hwd[1]; a.D = cache->hwd[2];
    a.hwd = (int64_t)a.H * a.W * a.D;
    a.seed = seed; a.batch = batch; a.n = n;
    a.coords = coords; a.feats = feats; a.labels = labels;
    return a;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_inr_class_count(const MrirtInrCache* cache, uint32_t num_classes, int64_t* counts, void* stream) {
    if (!cache || !counts) return MRIRT_ERR_NULL;
    const int rc = cls_check(cache, num_classes);
    if (rc != MRIRT_OK) return rc;
    ClsArgs a = cls_args(cache, num_classes);
    a.counts = (unsigned long long*)counts;
    hipStream_t s = (hipStream_t)stream;
    MRIRT_HIP(hipMemsetAsync(counts, 0, (size_t)cache->ncases * num_classes * sizeof(int64_t), s));
    hipLaunchKernelGGL(cls_count_kernel, dim3(a.chunks < 64u ? a.chunks : 64u, a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int64_t mrirt_inr_class_index_scratch_bytes(const MrirtInrCache* cache, uint32_t num_classes) {
    if (cls_check(cache, num_classes) != MRIRT_OK) return 0;
    return (int64_t)cls_scratch_bytes(cache->ncases, (uint64_t)cache->hwd[0] * cache->hwd[1] * cache->hwd[2], num_classes);
}

extern "C" int mrirt_inr_class_index(const MrirtInrCache* cache, uint32_t num_classes, const int64_t* offsets, uint32_t* index, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
    if (!cache || !offsets || !index) return MRIRT_ERR_NULL;
    int rc = cls_check(cache, num_classes);
    if (rc != MRIRT_OK) return rc;
    ClsArgs a = cls_args(cache, num_classes);
    if ((rc = check_scratch(scratch, scratch_bytes, cls_scratch_bytes(a.ncases, a.hwd, a.C))) != MRIRT_OK) return rc;
    a.chunkSums = (uint32_t*)scratch; a.offsets = offsets; a.index = index;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cls_chunk_kernel, dim3(a.chunks, a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cls_scan_kernel, dim3(a.ncases, a.C), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cls_emit_kernel, dim3(a.chunks, a.ncases), dim3(kTumThreads), 0, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_select_largest(const float* values, int64_t n, int64_t k, uint32_t* out, void* stream) {
    if (!values || !out) return MRIRT_ERR_NULL;
    if (n < 1 || n > (int64_t)kSelMaxN || k < 1 || k > n) return MRIRT_ERR_ARG;
    hipLaunchKernelGGL(select_largest_kernel, dim3(1), dim3(kSelThreads), 0, (hipStream_t)stream, values, (uint32_t)n, (uint32_t)k, out);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_inr_normal3(uint64_t seed, uint64_t batch_index, int64_t n, float* out, void* stream) {
    if (!out) return MRIRT_ERR_NULL;
    if (n < 1 || n >= (1ll << 31)) return MRIRT_ERR_ARG;
    hipLaunchKernelGGL(normal3_kernel, dim3((uint32_t)((n + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, (hipStream_t)stream, seed,
                       batch_index, n, out);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_inr_sample_candidates(const MrirtInrCache* cache, uint64_t seed, uint64_t batch_index, int64_t n_cand, float* coords,
                                           float* feats, int32_t* labels, void* stream) {
    if (!cache || !coords || !labels || (cache->numMods > 0 && !feats)) return MRIRT_ERR_NULL;
    const int rc = opt_check_cache(cache);                              // its own NULLs (seg, mods) first
    if (rc != MRIRT_OK) return rc;
    if (n_cand < 1 || n_cand >= (1ll << 31)) return MRIRT_ERR_ARG;
    const HybArgs a = hyb_args(cache, seed, batch_index, n_cand, coords, feats, labels);
    hipLaunchKernelGGL(candidates_kernel, dim3((uint32_t)((n_cand + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, (hipStream_t)stream, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_inr_sample_batch_hybrid(const MrirtInrCache* cache, const MrirtInrClassIndex* classes, const MrirtInrHybrid* hybrid,
                                             const float* const* fields, uint64_t seed, uint64_t batch_index, int64_t n, float* coords,
                                             float* feats, int32_t* labels, float* field_out, void* stream) {
    if (!cache || !hybrid || !coords || !labels || (cache->numMods > 0 && !feats)) return MRIRT_ERR_NULL;
    if (!cache->seg || (cache->numMods > 0 && !cache->mods)) return MRIRT_ERR_NULL;
    if ((fields != nullptr) != (field_out != nullptr)) return MRIRT_ERR_NULL;
    if (hybrid->nUncertain > 0 && !hybrid->picks) return MRIRT_ERR_NULL;
    if (hybrid->nPerClass > 0 && (!classes || !classes->index || !classes->offsets)) return MRIRT_ERR_NULL;
    const int rc = opt_check_cache(cache);
    if (rc != MRIRT_OK) return rc;
    if (n < 1 || n >= (1ll << 31) || hybrid->nUncertain < 0 || hybrid->nUncertain > n || hybrid->nPerClass < 0 || hybrid->nPerClass > n) return MRIRT_ERR_ARG;
    const uint32_t C = hybrid->nPerClass > 0 ? classes->numClasses : 0u;
    if (hybrid->nPerClass > 0 && (C < 1 || C > kLossMaxClasses || classes->reserved != 0u)) return MRIRT_ERR_ARG;
    if (hybrid->nUncertain + (int64_t)C * hybrid->nPerClass > n) return MRIRT_ERR_ARG;
    if (!(hybrid->noiseSigma >= 0.0f) || !isfinite(hybrid->noiseSigma) || hybrid->reserved != 0u) return MRIRT_ERR_ARG;
    HybArgs a = hyb_args(cache, seed, batch_index, n, coords, feats, labels);
    a.fields = fields; a.fieldOut = field_out;
    a.U = hybrid->nUncertain; a.P = hybrid->nPerClass; a.C = C;
    a.picks = hybrid->picks;
    if (a.P > 0) { a.index = classes->index; a.offsets = classes->offsets; }
    a.sigma = hybrid->noiseSigma;
    hipLaunchKernelGGL(sample_hybrid_kernel, dim3((uint32_t)((n + kOptThreads - 1) / kOptThreads)), dim3(kOptThreads), 0, (hipStream_t)stream, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
