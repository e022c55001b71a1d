// The extended INR loss and the tumour-ratio sampler (csrc/inr_lossx.hip): the layout of the loss's
// partial sums, the chunking of the tumour-index compaction and the mixed sampler's draw, written once for the device kernels
// and for the host (tests/native/inr_lossx_harness.hip walks them under AddressSanitizer + UBSan over buffers of exactly the
// real sizes).
#pragma once
#include <stdint.h>

#include "inr_optim.h"

namespace mrirt {

// ---- extended loss ------------------------------------------------------------------------------------------------------------
// per block (and once more for the totals), doubles.  The first kLossVals are mrirt_inr_loss's own, in its order:
//   [0..16) sum p_k   [16..32) sum p_k y_k   [32..48) count_k   [48..64) sum ce yh_k   [64] sum ce w
// then  [65] sum m ce (focal)  [66] sum w  [67] TP  [68] FP  [69] FN  [70] sum softplus(z_e) (1 - g)
constexpr uint32_t kLxFocal = kLossVals, kLxW = kLossVals + 1, kLxTp = kLossVals + 2, kLxFp = kLossVals + 3, kLxFn = kLossVals + 4,
                   kLxReg = kLossVals + 5;
constexpr uint32_t kLossXVals = kLossVals + 6;
constexpr uint32_t kLossXFinalThreads = 128;  // >= kLossXVals: thread v adds value v of every block, in block order
constexpr uint32_t kLossXTerms = 5;           // terms[]: CE, DL, FP / n, Tversky index, logit-regulariser mean

// doubles: [loss_blocks(n)][kLossXVals] partial sums, then [kLossXVals] totals
MRIRT_HD uint64_t lossx_scratch_bytes(int64_t n) { return tr_align((uint64_t)(loss_blocks(n) + 1) * kLossXVals * sizeof(double)); }
// where block b keeps value v; b == loss_blocks(n) is the totals' row
MRIRT_HD uint64_t lossx_sum_index(uint32_t block, uint32_t v) { return (uint64_t)block * kLossXVals + v; }
// the points thread t of block b sums: lossx_first(b, t), + lossx_stride(blocks), ... below n
MRIRT_HD int64_t lossx_first(uint32_t block, uint32_t thread) { return (int64_t)block * kLossThreads + thread; }
MRIRT_HD int64_t lossx_stride(uint32_t blocks) { return (int64_t)blocks * kLossThreads; }

// ---- tumour index: a deterministic compaction of the voxels with seg > 0 -------------------------------------------------------
// A case's H W D voxels are cut into chunks of kTumChunk; one block per (chunk, case); thread t owns the kTumPerThread
// consecutive voxels from tum_first(chunk, t) on, so that ascending (thread, voxel) is ascending voxel order.
constexpr uint32_t kTumThreads = 256;
constexpr uint32_t kTumPerThread = 16;
constexpr uint32_t kTumChunk = kTumThreads * kTumPerThread;

MRIRT_HD uint32_t tum_chunks(uint64_t hwd) { return (uint32_t)((hwd + kTumChunk - 1) / kTumChunk); }
MRIRT_HD uint64_t tum_first(uint32_t chunk, uint32_t thread) { return (uint64_t)chunk * kTumChunk + (uint64_t)thread * kTumPerThread; }
// uint32: [ncases][tum_chunks] tumour voxels per chunk, scanned in place to the exclusive prefix inside the case
MRIRT_HD uint64_t tum_scratch_bytes(uint32_t ncases, uint64_t hwd) { return tr_align((uint64_t)ncases * tum_chunks(hwd) * sizeof(uint32_t)); }
MRIRT_HD uint64_t tum_chunk_slot(uint32_t cs, uint32_t chunk, uint32_t chunksPerCase) { return (uint64_t)cs * chunksPerCase + chunk; }
// the scan: thread t of a case's block owns the tum_scan_len consecutive chunks from t * tum_scan_len on
MRIRT_HD uint32_t tum_scan_len(uint32_t chunksPerCase) { return (chunksPerCase + kTumThreads - 1) / kTumThreads; }

// flat voxel offset (x W D + y D + z) -> (x, y, z)
MRIRT_HD void tum_decode(uint32_t v, uint32_t W, uint32_t D, uint32_t& x, uint32_t& y, uint32_t& z) {
    const uint32_t xy = v / D;
    z = v - xy * D;
    x = xy / W;
    y = xy - x * W;
}

// ---- mixed sampler ------------------------------------------------------------------------------------------------------------
// Point i of micro-batch b under `seed`: the Philox words of sample_point (same key, same counter).  i >= nTumour: exactly
// sample_point.  i < nTumour: case = mulhi32(r0, ncases); with cnt = offsets[case + 1] - offsets[case] > 0 the voxel is
// index[offsets[case] + ((uint64) r1 cnt >> 32)], else the uniform draw from r1..r3 (the "fallback fill").
struct MixDraw { uint32_t r[4]; };
MRIRT_HD MixDraw mix_words(uint64_t seed, uint64_t batch, uint32_t i) {
    MixDraw d;
    d.r[0] = i; d.r[1] = (uint32_t)batch; d.r[2] = (uint32_t)(batch >> 32); d.r[3] = 0u;
    philox4x32_10(d.r, (uint32_t)seed, (uint32_t)(seed >> 32));
    return d;
}
MRIRT_HD SamplePoint mix_uniform(const MixDraw& d, uint32_t ncases, uint32_t H, uint32_t W, uint32_t D) {
    SamplePoint p;
    p.cs = mulhi32(d.r[0], ncases); p.x = mulhi32(d.r[1], H); p.y = mulhi32(d.r[2], W); p.z = mulhi32(d.r[3], D);
    return p;
}
// slot of a tumour draw inside the index: offsets[case] + floor(r1 cnt / 2^32), 0 < cnt < 2^32
MRIRT_HD int64_t mix_slot(uint32_t r1, int64_t first, int64_t cnt) { return first + (int64_t)(((uint64_t)r1 * (uint64_t)cnt) >> 32); }

}  // namespace mrirt
