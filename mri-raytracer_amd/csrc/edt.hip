// Exact squared Euclidean distance transform and the Hausdorff distance of two label volumes — the GPU form of
// hausdorff_distance, inr/inr/model.py:164-195 (two cKDTrees per class over every voxel of the class), bit-identical to it.
// The arithmetic, the pass geometry and the scratch layout are csrc/edt_line.h (shared with the host harness); this file
// is the staging in LDS, the masked maximum and the entry points.
//
// Per class: three line passes over two fields at once (grid.z: F_T from the truth, F_P from the prediction; the first
// pass reads the labels directly), then one masked max-reduction into the class's accumulators; one last launch turns the
// accumulators into directed_sq.  Nothing synchronises with the host.
#include "edt_line.h"
#include "mrirt_host.h"

namespace mrirt {

struct EdtPassArgs {
    EdtPass pass;
    const int16_t* labels[2];      // first pass: the volume each field is masked from (else nullptr)
    double* field[2];
    int32_t cls;
};

__global__ __launch_bounds__(kEdtThreads) void edt_pass_kernel(const EdtPassArgs a) {
    extern __shared__ double edtLds[];
    double* tile = edtLds;
    double* ctab = edtLds + (size_t)a.pass.n * a.pass.tl;
    const uint32_t o = blockIdx.x / a.pass.chunks, chunk = blockIdx.x % a.pass.chunks, f = blockIdx.z;
    edt_tile_load(a.pass, o, chunk, a.field[f], a.labels[f], a.cls, tile, ctab, threadIdx.x, kEdtThreads);
    __syncthreads();
    edt_tile_compute(a.pass, o, chunk, tile, ctab, a.field[f], threadIdx.x, kEdtThreads);
}

// acc[0] = bits of max over (pred == cls) of fT, acc[1] = bits of max over (truth == cls) of fP, acc[2] / acc[3] = 1 when
// the class occurs in pred / truth
__global__ __launch_bounds__(256) void edt_reduce_kernel(const int16_t* pred, const int16_t* truth, const double* fT, const double* fP,
                                                         int64_t voxels, int32_t cls, unsigned long long* acc) {
    __shared__ unsigned long long part[4][256];
    unsigned long long m[4] = { 0, 0, 0, 0 };
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < voxels; v += (int64_t)gridDim.x * 256) {
        if ((int32_t)pred[v] == cls) { const uint64_t b = edt_bits(fT[v]); m[0] = b > m[0] ? b : m[0]; m[2] = 1; }
        if ((int32_t)truth[v] == cls) { const uint64_t b = edt_bits(fP[v]); m[1] = b > m[1] ? b : m[1]; m[3] = 1; }
    }
    for (int k = 0; k < 4; ++k) part[k][threadIdx.x] = m[k];
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int k = 0; k < 4; ++k) {
                const unsigned long long x = part[k][threadIdx.x + w];
                if (x > part[k][threadIdx.x]) part[k][threadIdx.x] = x;
            }
        __syncthreads();
    }
    if (threadIdx.x < 4 && part[threadIdx.x][0] != 0) atomicMax(acc + threadIdx.x, part[threadIdx.x][0]);
}

__global__ void edt_zero_kernel(unsigned long long* acc, uint32_t words) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < words) acc[t] = 0;
}

__global__ void edt_finish_kernel(const unsigned long long* acc, uint32_t numClasses, double* directedSq) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;       // one thread per directed distance
    if (t >= 2 * numClasses) return;
    const unsigned long long* a = acc + (size_t)(t >> 1) * kEdtAccWords;
    directedSq[t] = (a[2] != 0 && a[3] != 0) ? edt_from_bits(a[t & 1]) : (double)NAN;
}

static int launch_pass(const uint32_t hwd[3], int axis, float s, const int16_t* lab0, const int16_t* lab1, double* f0, double* f1,
                       int32_t cls, uint32_t fields, hipStream_t stream) {
    EdtPassArgs a;
    a.pass = edt_pass(hwd, axis, s);
    a.labels[0] = lab0; a.labels[1] = lab1;
    a.field[0] = f0; a.field[1] = f1;
    a.cls = cls;
    const size_t lds = ((size_t)a.pass.n * a.pass.tl + a.pass.n) * sizeof(double);
    const dim3 grid(a.pass.outer * a.pass.chunks, 1, fields), block(kEdtThreads);
    hipLaunchKernelGGL(edt_pass_kernel, grid, block, lds, stream, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int64_t mrirt_edt_scratch_bytes(const uint32_t hwd[3], uint32_t num_classes) {
    if (!hwd || num_classes > kEdtMaxClasses || edt_check_volume(hwd, nullptr) != 0) return 0;
    if (num_classes == 0) return kEdtSquaredScratch;
    return edt_scratch((int64_t)hwd[0] * hwd[1] * hwd[2], num_classes).total;
}

extern "C" int mrirt_edt_squared(const int16_t* labels, const uint32_t hwd[3], int32_t cls, const float spacing[3],
                                 double* field_sq, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!labels || !hwd || !spacing || !field_sq || !scratch) return MRIRT_ERR_NULL;
    int rc = edt_check_volume(hwd, spacing);
    if (rc != MRIRT_OK) return rc;
    if (scratch_bytes < kEdtSquaredScratch) return MRIRT_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int axis = 0; axis < 3; ++axis) {
        rc =launch_pass(hwd, axis, spacing[axis], axis == 0 ? labels : nullptr, nullptr, field_sq, nullptr, cls, 1, s);
        if (rc != MRIRT_OK) return rc;
    }
    return MRIRT_OK;
}

extern "C" int mrirt_hausdorff(const int16_t* pred, const int16_t* truth, const uint32_t hwd[3], const float spacing[3],
                               uint32_t num_classes, double* directed_sq, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!pred || !truth || !hwd || !spacing || !directed_sq || !scratch) return MRIRT_ERR_NULL;
    int rc = edt_check_volume(hwd, spacing);
    if (rc != MRIRT_OK) return rc;
    if (num_classes == 0 || num_classes > kEdtMaxClasses) return MRIRT_ERR_ARG;
    const int64_t voxels = (int64_t)hwd[0] * hwd[1] * hwd[2];
    const EdtScratch lay = edt_scratch(voxels, num_classes);
    if (scratch_bytes < lay.total) return MRIRT_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    double* fT = reinterpret_cast<double*>(base + lay.field[0]);
    double* fP = reinterpret_cast<double*>(base + lay.field[1]);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(base + lay.acc);
    const uint32_t words = num_classes * kEdtAccWords;
    hipLaunchKernelGGL(edt_zero_kernel, dim3(1), dim3(128), 0, s, acc, words);
    MRIRT_HIP(hipGetLastError());
    const uint32_t blocks = (uint32_t)((voxels + 256 * 8 - 1) / (256 * 8));
    for (uint32_t c = 0; c < num_classes; ++c) {
        for (int axis = 0; axis < 3; ++axis) {
            rc = launch_pass(hwd, axis, spacing[axis], axis == 0 ? truth : nullptr, axis == 0 ? pred : nullptr, fT, fP, (int32_t)c, 2, s);
            if (rc != MRIRT_OK) return rc;
        }
        hipLaunchKernelGGL(edt_reduce_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(256), 0, s, pred, truth, fT, fP, voxels,
                           (int32_t)c, acc + (size_t)c * kEdtAccWords);
        MRIRT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(edt_finish_kernel, dim3(1), dim3(64), 0, s, acc, num_classes, directed_sq);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
