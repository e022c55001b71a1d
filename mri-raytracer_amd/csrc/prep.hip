// Case preparation on the device: the exact percentile window of np.percentile (fp32, `linear`), the [0,1] normalisation in
// both layouts, the z-score over non-zero voxels and scipy.ndimage's separable Gaussian filter (mode `reflect`).  The index
// arithmetic — keys, ranks, bin selection, the reflected index, the tiles and the scratch layouts — is csrc/prep_index.h
// (shared with the host harness); this file is the kernels and the entry points.
//
// Every stage is a chain of launches on the caller's stream: no workgroup waits for another one, nothing synchronises with
// the host, the only atomics are integer ones on LDS, and every fp64 sum is taken in an order fixed by n alone — two calls
// give the same bits.
//   window     init | 4 x ( histogram per block and live prefix -> totals in block order -> select ) | evaluate
//   normalise  one tile kernel: reads (X,Y,Z) rows, writes the (X,Y,Z) array and, through an LDS tile, the x-fastest buffer
//   z-score    2 x ( per-block fp64 partials -> one workgroup per modality ) | apply
//   gaussian   3 line passes through LDS tiles with an r-wide halo, ping-pong between the output and the scratch volume
#include "prep_index.h"
#include "mrirt_host.h"

namespace mrirt {

// --- percentile window ------------------------------------------------------------------------------------------------
struct PrepRanks { uint32_t k[kPrepRanks]; float g[2]; };

__global__ void prep_init_kernel(PrepSelectState* st, const PrepRanks rk) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (uint32_t r = 0; r < kPrepRanks; ++r) { st->prefix[r] = 0u; st->rem[r] = rk.k[r]; st->slot[r] = 0u; }
    st->nslots = 1u;
    st->minKey = kPrepNanKey;
    st->maxKey = 0u;
    st->pad = 0u;
}

// pass p counts digit p (most significant first) of every key whose higher digits equal a live prefix
__global__ __launch_bounds__(kPrepHistThreads) void prep_hist_kernel(const float* __restrict__ in, int64_t n, uint32_t pass,
                                                                 const PrepSelectState* __restrict__ st,
                                                                 uint32_t* __restrict__ partial, uint32_t* __restrict__ minmax) {
    __shared__ uint32_t h[kPrepRanks * kPrepBins];
    __shared__ uint32_t mm[2];
    const uint32_t t = threadIdx.x;
    for (uint32_t e = t; e < kPrepRanks * kPrepBins; e += kPrepHistThreads) h[e] = 0u;
    if (t == 0) { mm[0] = kPrepNanKey; mm[1] = 0u; }
    const uint32_t nslots = st->nslots;
    uint32_t prefix[kPrepRanks];
    for (uint32_t s = 0; s < kPrepRanks; ++s) prefix[s] = 0u;
    for (uint32_t r = 0; r < kPrepRanks; ++r) prefix[st->slot[r]] = st->prefix[r];
    __syncthreads();
    const uint32_t shift = 32u - kPrepDigitBits * (pass + 1u);      // of this pass's digit
    const uint32_t upper = shift + kPrepDigitBits;                  // 32 in pass 0: shifted as 64 bits below
    uint32_t lo = kPrepNanKey, hi = 0u;
    // a thread's loads depend on nothing but i: 16 waves per workgroup and four strides in flight hide their latency
    const int64_t stride = (int64_t)gridDim.x * kPrepHistThreads;
#pragma unroll 4
    for (int64_t i = (int64_t)blockIdx.x * kPrepHistThreads + t; i < n; i += stride) {
        const uint32_t key = prep_key(__float_as_uint(in[i]));
        lo = key < lo ? key : lo;
        hi = key > hi ? key : hi;
        const uint32_t up = (uint32_t)((uint64_t)key >> upper), bin = (key >> shift) & (kPrepBins - 1u);
        for (uint32_t s = 0; s < nslots; ++s)
            if (up == prefix[s]) atomicAdd(&h[s * kPrepBins + bin], 1u);
    }
    if (pass == 0u) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
    __syncthreads();
    uint32_t* dst = partial + (size_t)blockIdx.x * (kPrepRanks * kPrepBins);
    for (uint32_t e = t; e < kPrepRanks * kPrepBins; e += kPrepHistThreads) dst[e] = h[e];
    if (pass == 0u && t == 0) { minmax[2 * blockIdx.x] = mm[0]; minmax[2 * blockIdx.x + 1] = mm[1]; }
}

// totals[slot][bin] = the partials of blocks 0, 1, 2, ... added in that order; one workgroup per slot.  Quarter q of the
// workgroup adds the q-th quarter of the blocks (independent loads, eight in flight), then the quarters are added in order.
constexpr uint32_t kPrepReduceParts = 4;
__global__ __launch_bounds__(kPrepBins * kPrepReduceParts) void prep_reduce_kernel(const uint32_t* __restrict__ partial, uint32_t blocks,
                                                                                   const PrepSelectState* __restrict__ st,
                                                                                   uint32_t* __restrict__ totals) {
    __shared__ uint32_t part[kPrepReduceParts][kPrepBins];
    const uint32_t bin = threadIdx.x % kPrepBins, q = threadIdx.x / kPrepBins;
    const uint32_t e = blockIdx.x * kPrepBins + bin;
    const uint32_t per = (blocks + kPrepReduceParts - 1) / kPrepReduceParts;
    const uint32_t b0 = q * per, b1 = b0 + per < blocks ? b0 + per : blocks;
    uint32_t sum = 0u;
    if (blockIdx.x < st->nslots) {
#pragma unroll 8
        for (uint32_t b = b0; b < b1; ++b) sum += partial[(size_t)b * (kPrepRanks * kPrepBins) + e];
    }
    part[q][bin] = sum;
    __syncthreads();
    if (q == 0u) {
        for (uint32_t k = 1; k < kPrepReduceParts; ++k) sum += part[k][bin];
        totals[e] = sum;
    }
}

__global__ __launch_bounds__(64) void prep_select_kernel(PrepSelectState* st, const uint32_t* __restrict__ totals,
                                                         const uint32_t* __restrict__ minmax, uint32_t blocks, uint32_t pass) {
    __shared__ uint32_t mm[2];
    const uint32_t t = threadIdx.x;
    if (t == 0) { mm[0] = kPrepNanKey; mm[1] = 0u; }
    __syncthreads();
    if (pass == 0u) {
        uint32_t lo = kPrepNanKey, hi = 0u;
        for (uint32_t b = t; b < blocks; b += 64u) {
            const uint32_t a = minmax[2 * b], c = minmax[2 * b + 1];
            lo = a < lo ? a : lo;
            hi = c > hi ? c : hi;
        }
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
    if (t < kPrepRanks) {
        uint32_t rem;
        const uint32_t bin = prep_select_bin(totals + st->slot[t] * kPrepBins, st->rem[t], &rem);
        st->prefix[t] = (st->prefix[t] << kPrepDigitBits) | bin;
        st->rem[t] = rem;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t prefix[kPrepRanks], slot[kPrepRanks];
        for (uint32_t r = 0; r < kPrepRanks; ++r) prefix[r] = st->prefix[r];
        st->nslots = prep_assign_slots(prefix, slot);
        for (uint32_t r = 0; r < kPrepRanks; ++r) st->slot[r] = slot[r];
        if (pass == 0u) { st->minKey = mm[0]; st->maxKey = mm[1]; }
    }
}

// np.percentile's interpolation between the order statistics a = s[k] and b = s[min(k + 1, n - 1)], every step fp32
__device__ __forceinline__ float prep_lerp(float a, float b, float g) {
    const float d = b - a;
    if (g < 0.5f) return a + d * g;
    return b - d * (1.0f - g);
}

// record: { lo, hi, span, min, max, p_lo, p_hi, 0 }
__global__ void prep_window_kernel(const PrepSelectState* st, const PrepRanks rk, float* record) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool anyNan = st->maxKey == kPrepNanKey;                  // NaN sorts last; NumPy then answers NaN throughout
    const float nan = __uint_as_float(0x7FC00000u);
    float s[kPrepRanks];
    for (uint32_t r = 0; r < kPrepRanks; ++r) s[r] = __uint_as_float(prep_key_inverse(st->prefix[r]));
    const float pLo = anyNan ? nan : prep_lerp(s[0], s[1], rk.g[0]);
    const float pHi = anyNan ? nan : prep_lerp(s[2], s[3], rk.g[1]);
    const float mn = anyNan ? nan : __uint_as_float(prep_key_inverse(st->minKey));
    const float mx = anyNan ? nan : __uint_as_float(prep_key_inverse(st->maxKey));
    float lo = pLo, hi = pHi;
    if (hi <= lo) { lo = mn; hi = mx; }
    const double d = (double)hi - (double)lo;
    const float span = (float)(d > 1e-6 ? d : 1e-6);               // max(1e-6, d) as Python evaluates it (NaN -> 1e-6)
    record[0] = lo; record[1] = hi; record[2] = span; record[3] = mn; record[4] = mx; record[5] = pLo; record[6] = pHi;
    record[7] = 0.0f;
}

// --- normalise --------------------------------------------------------------------------------------------------------
constexpr uint32_t kPrepTile = 32;

__device__ __forceinline__ float prep_norm1(float v, float lo, float span) {
    float q = (v - lo) / span;
    q = q < 0.0f ? 0.0f : q;                                        // a NaN stays a NaN, as in np.clip
    q = q > 1.0f ? 1.0f : q;
    return q;
}

// in: (X,Y,Z) C order.  norm (may be NULL): the same order.  linear (may be NULL): x + y X + z X Y.  A tile is 32 x by 32 z
// of one y: read and written along z, transposed in LDS, written along x.
__global__ __launch_bounds__(kPrepThreads) void prep_normalize_kernel(const float* in, uint32_t X, uint32_t Y, uint32_t Z,
                                                                      const float* __restrict__ record, float* norm,
                                                                      float* __restrict__ linear, int64_t tiles, uint32_t tilesX, uint32_t tilesZ) {
    __shared__ float tile[kPrepTile][kPrepTile + 1];
    const float lo = record[0], span = record[2];
    const uint32_t tx = threadIdx.x % kPrepTile, ty = threadIdx.x / kPrepTile;          // ty in 0..7
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t z0 = (uint32_t)(t % tilesZ) * kPrepTile;
        const int64_t u = t / tilesZ;
        const uint32_t x0 = (uint32_t)(u % tilesX) * kPrepTile, y = (uint32_t)(u / tilesX);
        for (uint32_t j = ty; j < kPrepTile; j += kPrepThreads / kPrepTile) {
            const uint32_t x = x0 + j, z = z0 + tx;
            if (x < X && z < Z) {
                const size_t idx = ((size_t)x * Y + y) * Z + z;
                const float q = prep_norm1(in[idx], lo, span);
                if (norm) norm[idx] = q;
                tile[j][tx] = q;
            }
        }
        if (linear) {
            __syncthreads();
            for (uint32_t j = ty; j < kPrepTile; j += kPrepThreads / kPrepTile) {
                const uint32_t z = z0 + j, x = x0 + tx;
                if (x < X && z < Z) linear[((size_t)z * Y + y) * X + x] = tile[tx][j];
            }
            __syncthreads();
        }
    }
}

// --- z-score ----------------------------------------------------------------------------------------------------------
struct PrepZState { double sum, mu, count, pad; };
struct PrepZPartial { double sum; unsigned long long count; };

// the workgroup's sum of x and c in a fixed tree; valid in thread 0
__device__ __forceinline__ void prep_block_sum(double& x, unsigned long long& c, double* lx, unsigned long long* lc) {
    const uint32_t t = threadIdx.x;
    lx[t] = x; lc[t] = c;
    __syncthreads();
    for (uint32_t off = kPrepThreads / 2; off > 0; off >>= 1) {
        if (t < off) { lx[t] = lx[t] + lx[t + off]; lc[t] += lc[t + off]; }
        __syncthreads();
    }
    x = lx[0]; c = lc[0];
    __syncthreads();
}

// SECOND = false: sum and count of v != 0; SECOND = true: sum of (v - mu)^2 over v != 0.  grid (blocks, M).
template <bool SECOND>
__global__ __launch_bounds__(kPrepThreads) void prep_zpartial_kernel(const float* __restrict__ in, int64_t n, const PrepZState* __restrict__ st,
                                                                     PrepZPartial* __restrict__ partial) {
    __shared__ double lx[kPrepThreads];
    __shared__ unsigned long long lc[kPrepThreads];
    const float* src = in + (size_t)blockIdx.y * (size_t)n;
    const double mu = SECOND ? st[blockIdx.y].mu : 0.0;
    double x = 0.0;
    unsigned long long c = 0;
    const int64_t stride = (int64_t)gridDim.x * kPrepThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; i < n; i += stride) {
        const float v = src[i];
        if (v != 0.0f) {
            if (SECOND) { const double d = (double)v - mu; x += d * d; }
            else x += (double)v;
            ++c;
        }
    }
    prep_block_sum(x, c, lx, lc);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = PrepZPartial{ x, c };
}

// one workgroup per modality adds the blocks' partials in a fixed tree.  stats: [4][M] words { mu, sigma, sigma + 1e-6, count }
template <bool SECOND>
__global__ __launch_bounds__(kPrepThreads) void prep_zfinal_kernel(const PrepZPartial* __restrict__ partial, uint32_t blocks, PrepZState* st,
                                                                   uint32_t M, uint32_t* stats) {
    __shared__ double lx[kPrepThreads];
    __shared__ unsigned long long lc[kPrepThreads];
    const uint32_t m = blockIdx.x;
    double x = 0.0;
    unsigned long long c = 0;
    if (threadIdx.x < blocks) { x = partial[(size_t)m * blocks + threadIdx.x].sum; c = partial[(size_t)m * blocks + threadIdx.x].count; }
    prep_block_sum(x, c, lx, lc);
    if (threadIdx.x != 0) return;
    if (!SECOND) {
        st[m].sum = x;
        st[m].count = (double)c;
        st[m].mu = c ? x / (double)c : 0.0;
        st[m].pad = 0.0;
    } else {
        const double cnt = st[m].count;
        const float mu32 = (float)st[m].mu;
        const float sg32 = cnt > 0.0 ? (float)sqrt(x / cnt) : 0.0f;
        stats[m] = __float_as_uint(mu32);
        stats[M + m] = __float_as_uint(sg32);
        stats[2 * M + m] = __float_as_uint(sg32 + 1e-6f);
        stats[3 * M + m] = (uint32_t)cnt;
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_zapply_kernel(const float* in, int64_t n, uint32_t M, const uint32_t* __restrict__ stats,
                                                                   float* out) {
    const uint32_t m = blockIdx.y;
    const float mu = __uint_as_float(stats[m]), div = __uint_as_float(stats[2 * M + m]);
    const bool any = stats[3 * M + m] != 0u;
    const float* src = in + (size_t)m * (size_t)n;
    float* dst = out + (size_t)m * (size_t)n;
    const int64_t stride = (int64_t)gridDim.x * kPrepThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; i < n; i += stride) {
        const float v = src[i];
        dst[i] = any ? (v - mu) / div : v;
    }
}

// --- Gaussian filter --------------------------------------------------------------------------------------------------
struct PrepWeights { double w[2 * kPrepMaxRadius + 1]; };

// one pass along `axis` of a [outer][len][inner] volume; tile TO x TL x TI outputs, staged with an r-wide halo along the line
template <uint32_t TO, uint32_t TL, uint32_t TI>
__global__ __launch_bounds__(kPrepThreads) void prep_gauss_line_kernel(const float* __restrict__ in, float* __restrict__ out, const PrepLineGeom g,
                                                                       int r, const PrepWeights wt) {
    constexpr uint32_t kRowsMax = TL + 2 * kPrepMaxRadius;
    __shared__ float stage[TO * kRowsMax * TI];
    const uint32_t rows = TL + 2u * (uint32_t)r;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int64_t o0, l0, i0;
        prep_tile_origin(g, t, TO, TL, TI, &o0, &l0, &i0);
        for (uint32_t e = threadIdx.x; e < TO * rows * TI; e += kPrepThreads) {
            uint32_t o, l, i;
            prep_stage_coords(e, rows, TI, &o, &l, &i);
            float v = 0.0f;
            if (o0 + o < g.outer && i0 + i < g.inner) {
                const int64_t src = prep_reflect(l0 + (int64_t)l - r, g.len);
                v = in[((o0 + o) * g.len + src) * g.inner + (i0 + i)];
            }
            stage[e] = v;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < TO * TL * TI; e += kPrepThreads) {
            uint32_t o, l, i;
            prep_stage_coords(e, TL, TI, &o, &l, &i);
            if (o0 + o < g.outer && l0 + l < g.len && i0 + i < g.inner) {
                const float* x = stage + ((size_t)o * rows + (l + r)) * TI + i;       // x[j * TI]: the input at line position + j
                double acc = (double)x[0] * wt.w[r];
                for (int j = -r; j < 0; ++j) acc += ((double)x[j * (int)TI] + (double)x[-j * (int)TI]) * wt.w[j + r];
                out[((o0 + o) * g.len + (l0 + l)) * g.inner + (i0 + i)] = (float)acc;
            }
        }
        __syncthreads();
    }
}

static int prep_gauss_pass(const float* in, float* out, const uint32_t dims[3], int axis, int r, const PrepWeights& wt, hipStream_t s) {
    int64_t inner = 1;
    for (int k = axis + 1; k < 3; ++k) inner *= dims[k];
    const int64_t maxGrid = 1 << 16;
    if (inner >= 8) {
        const PrepLineGeom g = prep_line_geom(dims, axis, 1, 32, 32);
        hipLaunchKernelGGL((prep_gauss_line_kernel<1, 32, 32>), dim3((uint32_t)(g.tiles < maxGrid ? g.tiles : maxGrid)), dim3(kPrepThreads), 0, s,
                           in, out, g, r, wt);
    } else {
        const PrepLineGeom g = prep_line_geom(dims, axis, 4, 64, 1);
        hipLaunchKernelGGL((prep_gauss_line_kernel<4, 64, 1>), dim3((uint32_t)(g.tiles < maxGrid ? g.tiles : maxGrid)), dim3(kPrepThreads), 0, s,
                           in, out, g, r, wt);
    }
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

// n = the product of the extents when every extent is >= 1 and n <= 2^31 - 1, else 0
static int64_t prep_volume_elems(const uint32_t dims[3]) {
    uint64_t n = 1;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] == 0u) return 0;
        n *= dims[k];
        if (n > (uint64_t)kPrepMaxN) return 0;
    }
    return (int64_t)n;
}

static bool prep_percentile_ok(float q) { return q >= 0.0f && q <= 100.0f; }      // false for NaN

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_prep_scratch_bytes(int64_t n) {
    PrepWindowPlan p;
    return prep_window_plan(n, &p) ? p.total : 0;
}

extern "C" int mrirt_prep_window(const float* vol, int64_t n, float q_lo, float q_hi, float* record, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
    if (!vol || !record || !scratch) return MRIRT_ERR_NULL;
    PrepWindowPlan p;
    if (!prep_window_plan(n, &p)) return MRIRT_ERR_ARG;
    if (!prep_percentile_ok(q_lo) || !prep_percentile_ok(q_hi)) return MRIRT_ERR_ARG;
    if (scratch_bytes < p.total || (reinterpret_cast<uintptr_t>(scratch) & 15u) != 0u) return MRIRT_ERR_ARG;
    PrepRanks rk;
    prep_rank(n, q_lo, &rk.k[0], &rk.g[0]);
    prep_rank(n, q_hi, &rk.k[2], &rk.g[1]);
    for (int h = 0; h < 2; ++h) rk.k[2 * h + 1] = (int64_t)rk.k[2 * h] + 1 < n ? rk.k[2 * h] + 1u : (uint32_t)(n - 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    PrepSelectState* st = reinterpret_cast<PrepSelectState*>(base + p.state);
    uint32_t* minmax = reinterpret_cast<uint32_t*>(base + p.minmax);
    uint32_t* totals = reinterpret_cast<uint32_t*>(base + p.totals);
    uint32_t* partial = reinterpret_cast<uint32_t*>(base + p.partial);
    hipLaunchKernelGGL(prep_init_kernel, dim3(1), dim3(64), 0, s, st, rk);
    MRIRT_HIP(hipGetLastError());
    for (uint32_t pass = 0; pass < kPrepPasses; ++pass) {
        hipLaunchKernelGGL(prep_hist_kernel, dim3(p.blocks), dim3(kPrepHistThreads), 0, s, vol, n, pass, (const PrepSelectState*)st, partial, minmax);
        MRIRT_HIP(hipGetLastError());
        hipLaunchKernelGGL(prep_reduce_kernel, dim3(kPrepRanks), dim3(kPrepBins * kPrepReduceParts), 0, s, (const uint32_t*)partial, p.blocks,
                           (const PrepSelectState*)st, totals);
        MRIRT_HIP(hipGetLastError());
        hipLaunchKernelGGL(prep_select_kernel, dim3(1), dim3(64), 0, s, st, (const uint32_t*)totals, (const uint32_t*)minmax, p.blocks, pass);
        MRIRT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(prep_window_kernel, dim3(1), dim3(64), 0, s, (const PrepSelectState*)st, rk, record);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_prep_normalize(const float* vol, const uint32_t dims[3], const float* record, float* norm, float* linear, void* stream) {
    if (!vol || !dims || !record) return MRIRT_ERR_NULL;
    if (!norm && !linear) return MRIRT_ERR_NULL;
    if (dims[0] == 0u || dims[1] == 0u || dims[2] == 0u) return MRIRT_ERR_DIMS;
    if (prep_volume_elems(dims) == 0) return MRIRT_ERR_ARG;
    if (linear == vol) return MRIRT_ERR_ARG;                        // the transposed layout cannot be written in place
    const uint32_t tilesX = (dims[0] + kPrepTile - 1) / kPrepTile, tilesZ = (dims[2] + kPrepTile - 1) / kPrepTile;
    const int64_t tiles = (int64_t)tilesX * tilesZ * dims[1];
    const int64_t maxGrid = 1 << 16;
    hipLaunchKernelGGL(prep_normalize_kernel, dim3((uint32_t)(tiles < maxGrid ? tiles : maxGrid)), dim3(kPrepThreads), 0,
                       static_cast<hipStream_t>(stream), vol, dims[0], dims[1], dims[2], record, norm, linear, tiles, tilesX, tilesZ);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int64_t mrirt_prep_zscore_scratch_bytes(int64_t n, uint32_t num_mods) { return prep_zscore_scratch(n, num_mods); }

extern "C" int mrirt_prep_zscore_stats(const float* mods, int64_t n, uint32_t num_mods, void* stats, void* scratch, int64_t scratch_bytes,
                                       void* stream) {
    if (!mods || !stats || !scratch) return MRIRT_ERR_NULL;
    const int64_t need = prep_zscore_scratch(n, num_mods);
    if (need == 0) return MRIRT_ERR_ARG;
    if (scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 15u) != 0u) return MRIRT_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t blocks = prep_zscore_blocks(n);
    PrepZState* st = reinterpret_cast<PrepZState*>(scratch);
    PrepZPartial* partial = reinterpret_cast<PrepZPartial*>(static_cast<char*>(scratch) + prep_align256(32ll * num_mods));
    hipLaunchKernelGGL(prep_zpartial_kernel<false>, dim3(blocks, num_mods), dim3(kPrepThreads), 0, s, mods, n, (const PrepZState*)st, partial);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(prep_zfinal_kernel<false>, dim3(num_mods), dim3(kPrepThreads), 0, s, (const PrepZPartial*)partial, blocks, st, num_mods,
                       static_cast<uint32_t*>(stats));
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(prep_zpartial_kernel<true>, dim3(blocks, num_mods), dim3(kPrepThreads), 0, s, mods, n, (const PrepZState*)st, partial);
    MRIRT_HIP(hipGetLastError());
    hipLaunchKernelGGL(prep_zfinal_kernel<true>, dim3(num_mods), dim3(kPrepThreads), 0, s, (const PrepZPartial*)partial, blocks, st, num_mods,
                       static_cast<uint32_t*>(stats));
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_prep_zscore_apply(const float* mods, int64_t n, uint32_t num_mods, const void* stats, float* out, void* stream) {
    if (!mods || !stats || !out) return MRIRT_ERR_NULL;
    if (n < 1 || n > kPrepMaxN || num_mods < 1u || num_mods > 64u) return MRIRT_ERR_ARG;
    const int64_t per = (int64_t)kPrepThreads * kPrepZItems;
    int64_t blocks = (n + per - 1) / per;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(prep_zapply_kernel, dim3((uint32_t)blocks, num_mods), dim3(kPrepThreads), 0, static_cast<hipStream_t>(stream), mods, n,
                       num_mods, static_cast<const uint32_t*>(stats), out);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

extern "C" int mrirt_prep_gaussian3d(const float* vol, const uint32_t dims[3], const double* weights, int32_t radius, float* out, float* scratch,
                                     void* stream) {
    if (!vol || !dims || !weights || !out || !scratch) return MRIRT_ERR_NULL;
    if (dims[0] == 0u || dims[1] == 0u || dims[2] == 0u) return MRIRT_ERR_DIMS;
    const int64_t n = prep_volume_elems(dims);
    if (n == 0 || radius < 0 || radius > kPrepMaxRadius) return MRIRT_ERR_ARG;
    // out may be vol itself; every other overlap of the three volumes is refused
    const uintptr_t a = reinterpret_cast<uintptr_t>(vol), b = reinterpret_cast<uintptr_t>(out), c = reinterpret_cast<uintptr_t>(scratch);
    const uintptr_t bytes = (uintptr_t)n * 4u;
    auto overlap = [bytes](uintptr_t p, uintptr_t q) { return p < q + bytes && q < p + bytes; };
    if ((a != b && overlap(a, b)) || overlap(a, c) || overlap(b, c)) return MRIRT_ERR_ARG;
    PrepWeights wt;
    for (int j = 0; j < 2 * kPrepMaxRadius + 1; ++j) wt.w[j] = j < 2 * radius + 1 ? weights[j] : 0.0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if (vol == out) {
        // in place: vol -> scratch -> out -> scratch, then one copy on the stream
        if ((rc = prep_gauss_pass(vol, scratch, dims, 0, radius, wt, s)) != MRIRT_OK) return rc;
        if ((rc = prep_gauss_pass(scratch, out, dims, 1, radius, wt, s)) != MRIRT_OK) return rc;
        if ((rc = prep_gauss_pass(out, scratch, dims, 2, radius, wt, s)) != MRIRT_OK) return rc;
        MRIRT_HIP(hipMemcpyAsync(out, scratch, (size_t)bytes, hipMemcpyDeviceToDevice, s));
        return MRIRT_OK;
    }
    if ((rc = prep_gauss_pass(vol, out, dims, 0, radius, wt, s)) != MRIRT_OK) return rc;
    if ((rc = prep_gauss_pass(out, scratch, dims, 1, radius, wt, s)) != MRIRT_OK) return rc;
    return prep_gauss_pass(scratch, out, dims, 2, radius, wt, s);
}
