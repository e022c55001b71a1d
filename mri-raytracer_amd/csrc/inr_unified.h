// The unified focal + Dice + TV + boundary loss of the reference's notebooks/improved.ipynb (cell 8) and the field gather
// that goes with the samplers (csrc/inr_unified.hip): the layout of the loss's partial sums and of its
// coefficient row, and the voxel a sampled point reads, written once for the device kernels and for the host
// (tests/native/unified_loss_harness.hip walks them under AddressSanitizer + UBSan over buffers of exactly the real sizes).
#pragma once
#include <stdint.h>

#include "inr_lossx.h"

namespace mrirt {

// ---- loss ----------------------------------------------------------------------------------------------------------------------
// per block (and once more for the totals), doubles, with K = kLossMaxClasses:
//   [0..K) P_k = sum pc_k   [K..2K) A_k = sum pc_k t_k   [2K..3K) T_k = sum t_k   [3K..4K) S_k = sum pu_k   [4K..5K) Q_k = sum pu_k^2
//   [5K] FL   [5K + 1] Bd   [5K + 2] Acc
constexpr uint32_t kUnP = 0, kUnA = kLossMaxClasses, kUnT = 2 * kLossMaxClasses, kUnS = 3 * kLossMaxClasses, kUnQ = 4 * kLossMaxClasses;
constexpr uint32_t kUnFL = 5 * kLossMaxClasses, kUnBd = kUnFL + 1, kUnAcc = kUnFL + 2;
constexpr uint32_t kUnVals = kUnFL + 3;
constexpr uint32_t kUnFinalThreads = 128;     // >= kUnVals: thread v adds value v of every block, in block order
constexpr uint32_t kUnAux = 8;                // aux[]: ufl, mFTL, mFL, dl, tv, bl, mean tumour Dice, accuracy; then Dice per class
// the coefficient row the final kernel leaves for the gradient (one more row of kUnVals doubles, each holding an fp32 value):
//   [0..K) GP_k = dloss/dP_k   [K..2K) GA_k = dloss/dA_k   [2K..3K) S_k / n   [3K] the focal scale uflWeight gate (1 - lambda) / n
//   [3K + 1] the TV scale 2 tvWeight / n
constexpr uint32_t kUnGP = 0, kUnGA = kLossMaxClasses, kUnMean = 2 * kLossMaxClasses, kUnFocal = 3 * kLossMaxClasses, kUnTv = kUnFocal + 1;
constexpr uint32_t kUnCoefs = kUnTv + 1;

constexpr float kUnLogitClip = 10.0f;
constexpr float kUnProbLo = 1e-7f, kUnProbHi = 1.0f - 1e-7f;

// doubles: [loss_blocks(n)][kUnVals] partial sums, [kUnVals] totals, [kUnVals] coefficients
MRIRT_HD uint64_t unified_scratch_bytes(int64_t n) { return tr_align((uint64_t)(loss_blocks(n) + 2) * kUnVals * sizeof(double)); }
// where block b keeps value v; b == loss_blocks(n) is the totals' row, b == loss_blocks(n) + 1 the coefficients'
MRIRT_HD uint64_t unified_sum_index(uint32_t block, uint32_t v) { return (uint64_t)block * kUnVals + v; }
// the points thread t of block b sums: unified_first(b, t), + unified_stride(blocks), ... below n
MRIRT_HD int64_t unified_first(uint32_t block, uint32_t thread) { return (int64_t)block * kLossThreads + thread; }
MRIRT_HD int64_t unified_stride(uint32_t blocks) { return (int64_t)blocks * kLossThreads; }
// the gradient pass: one thread per point, unified_grad_blocks(n) blocks of kLossThreads
MRIRT_HD uint32_t unified_grad_blocks(int64_t n) { return (uint32_t)(((uint64_t)n + kLossThreads - 1) / kLossThreads); }
MRIRT_HD int64_t unified_logit_index(int64_t i, uint32_t C, uint32_t k) { return i * (int64_t)C + k; }

// ---- field gather ----------------------------------------------------------------------------------------------------------------
// The voxel point i of micro-batch `batch` reads: sample_point's when i >= nTumour, else the mixed sampler's (index / offsets
// may be NULL when nTumour == 0).  Exactly the draw of sample_kernel / sample_mix_kernel, through their own functions.
struct FieldVoxel { uint32_t cs; int64_t voxel; };
MRIRT_HD FieldVoxel field_voxel(uint64_t seed, uint64_t batch, uint32_t i, int64_t nTumour, uint32_t ncases, uint32_t H, uint32_t W,
                                uint32_t D, int64_t hwd, const uint32_t* index, const int64_t* offsets) {
    SamplePoint p;
    if (nTumour == 0) {
        p = sample_point(seed, batch, i, ncases, H, W, D);
    } else {
        const MixDraw dr = mix_words(seed, batch, i);
        p = mix_uniform(dr, ncases, H, W, D);
        if ((int64_t)i < nTumour) {
            const int64_t first = offsets[p.cs], cnt = offsets[p.cs + 1] - first;
            if (cnt > 0) {
                const uint32_t v = index[mix_slot(dr.r[1], first, cnt)];
                if ((int64_t)v < hwd) tum_decode(v, W, D, p.x, p.y, p.z);
            }
        }
    }
    FieldVoxel f;
    f.cs = p.cs;
    f.voxel = voxel_offset(p.x, p.y, p.z, W, D);
    return f;
}

}  // namespace mrirt
