// The index arithmetic of the unified loss and of the samplers' field gather (csrc/inr_unified.h) on the CPU under
// AddressSanitizer + UBSan.  Every item replays a launch block by block and thread by thread with the functions the kernels
// call, over heap buffers of EXACTLY the real sizes: an index past one is an ASan report.  Items:
//   l <n> <C>                         unified_partial / unified_final / unified_grad: every point is summed exactly once, every
//                                     partial-sum, total and coefficient slot lies inside mrirt_unified_loss_scratch_bytes(n),
//                                     every logit is read and every dlogits element written exactly once
//   f <ncases> <H> <W> <D> <n> <nt>   field_gather_kernel over a cache with a tumour index (case 0 without tumour: the fallback
//                                     fill; case 1 all tumour): every read inside its case's field, the value that of the voxel
//                                     sample_point / the mixed draw names, points from the index on tumour voxels
//   big                               n = 2^31 - 1: block counts, strides, the last point and the last logit index (arithmetic
//                                     only, no such buffer)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_unified.h"

using namespace mrirt;

static int loss_item(int64_t n, uint32_t C) {
    const uint32_t blocks = loss_blocks(n);
    const uint64_t bytes = unified_scratch_bytes(n);
    double* sums = (double*)malloc(bytes);
    float* logits = (float*)malloc((size_t)n * C * sizeof(float));
    float* dlogits = (float*)malloc((size_t)n * C * sizeof(float));
    unsigned char* seen = (unsigned char*)calloc((size_t)n, 1);
    unsigned char* wrote = (unsigned char*)calloc((size_t)n * C, 1);
    if (!sums || !logits || !dlogits || !seen || !wrote) return 2;
    for (int64_t e = 0; e < n * (int64_t)C; ++e) logits[e] = (float)(e % 7);
    long long bad = 0;
    bad += blocks < 1 || blocks > kLossMaxBlocks || kUnVals > kUnFinalThreads || kUnVals != 5 * kLossMaxClasses + 3 || kUnCoefs > kUnVals ||
           kUnCoefs > kLossThreads;
    bad += bytes < (uint64_t)(blocks + 2) * kUnVals * sizeof(double) || (bytes & 255u) != 0;
    for (uint32_t b = 0; b < blocks; ++b) {                  // unified_partial_kernel
        double block[kUnVals] = { 0 };
        for (uint32_t t = 0; t < kLossThreads; ++t)
            for (int64_t i = unified_first(b, t); i < n; i += unified_stride(blocks)) {
                bad += seen[i]++ != 0;
                for (uint32_t k = 0; k < C; ++k) block[kUnP + k] += (double)logits[unified_logit_index(i, C, k)];
                block[kUnAcc] += 1.0;
            }
        for (uint32_t v = 0; v < kUnVals; ++v) sums[unified_sum_index(b, v)] = block[v];
    }
    for (int64_t i = 0; i < n; ++i) bad += seen[i] != 1;
    for (uint32_t v = 0; v < kUnVals; ++v) {                 // unified_final_kernel: thread v adds the blocks, writes the totals' row
        double s = 0.0;
        for (uint32_t b = 0; b < blocks; ++b) s += sums[unified_sum_index(b, v)];
        sums[unified_sum_index(blocks, v)] = s;
    }
    bad += sums[unified_sum_index(blocks, kUnAcc)] != (double)n;
    for (uint32_t v = 0; v < kUnCoefs; ++v) sums[unified_sum_index(blocks + 1, v)] = (double)v;      // ... and the coefficients' row
    const uint32_t gblocks = unified_grad_blocks(n);         // unified_grad_kernel
    bad += (uint64_t)gblocks * kLossThreads < (uint64_t)n || (uint64_t)(gblocks - 1) * kLossThreads >= (uint64_t)n;
    for (uint32_t b = 0; b < gblocks; ++b) {
        float co[kUnCoefs];
        for (uint32_t t = 0; t < kLossThreads; ++t)
            if (t < kUnCoefs) co[t] = (float)sums[unified_sum_index(blocks + 1, t)];
        for (uint32_t t = 0; t < kLossThreads; ++t) {
            const int64_t i = (int64_t)b * kLossThreads + t;
            if (i >= n) continue;
            for (uint32_t k = 0; k < C; ++k) {
                const int64_t e = unified_logit_index(i, C, k);
                bad += wrote[e]++ != 0;
                dlogits[e] = logits[e] + co[kUnTv];
            }
        }
    }
    for (int64_t e = 0; e < n * (int64_t)C; ++e) bad += wrote[e] != 1 || dlogits[e] != logits[e] + (float)kUnTv;
    printf("item l %lld %u blocks %u grad blocks %u bytes %llu mismatches %lld\n", (long long)n, C, blocks, gblocks, (unsigned long long)bytes, bad);
    free(sums); free(logits); free(dlogits); free(seen); free(wrote);
    return bad ? 1 : 0;
}

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static int field_item(uint32_t ncases, uint32_t H, uint32_t W, uint32_t D, int64_t n, int64_t nt) {
    const int64_t hwd = (int64_t)H * W * D;
    std::vector<int16_t*> seg;
    std::vector<float*> fields;
    std::vector<int64_t> offsets(ncases + 1, 0);
    uint64_t s = 777u + ncases + D;
    for (uint32_t k = 0; k < ncases; ++k) {
        int16_t* sg = (int16_t*)malloc((size_t)hwd * sizeof(int16_t));
        float* f = (float*)malloc((size_t)hwd * sizeof(float));
        if (!sg || !f) return 2;
        int64_t cnt = 0;
        for (int64_t v = 0; v < hwd; ++v) {
            sg[v] = k == 0 ? 0 : k == 1 ? (int16_t)(1 + rnd(s) % 3) : (int16_t)(rnd(s) % 5 == 0 ? 1 + rnd(s) % 3 : 0);
            f[v] = (float)(k * 4096 + (v % 4096));
            cnt += sg[v] > 0;
        }
        seg.push_back(sg); fields.push_back(f);
        offsets[k + 1] = offsets[k] + cnt;
    }
    const int64_t total = offsets[ncases];
    uint32_t* index = (uint32_t*)malloc((size_t)(total ? total : 1) * sizeof(uint32_t));
    float* out = (float*)malloc((size_t)n * sizeof(float));
    if (!index || !out) return 2;
    for (uint32_t k = 0; k < ncases; ++k) {                  // the ascending index mrirt_inr_tumour_index builds
        int64_t at = offsets[k];
        for (int64_t v = 0; v < hwd; ++v)
            if (seg[k][v] > 0) index[at++] = (uint32_t)v;
    }
    long long bad = 0, fromIndex = 0, fallback = 0;
    const uint64_t seeds[2] = { 42u, 0xC0FFEE0000004Dull }, batches[2] = { 0, (1ull << 32) + 5 };
    for (uint64_t seed : seeds)
        for (uint64_t batch : batches) {
            const uint32_t gblocks = (uint32_t)((n + kOptThreads - 1) / kOptThreads);
            for (uint32_t b = 0; b < gblocks; ++b)
                for (uint32_t t = 0; t < kOptThreads; ++t) { // field_gather_kernel
                    const int64_t i = (int64_t)b * kOptThreads + t;
                    if (i >= n) continue;
                    const FieldVoxel f = field_voxel(seed, batch, (uint32_t)i, nt, ncases, H, W, D, hwd, nt ? index : nullptr,
                                                     nt ? offsets.data() : nullptr);
                    bad += f.cs >= ncases || f.voxel < 0 || f.voxel >= hwd;
                    out[i] = fields[f.cs][f.voxel];
                    // what the samplers draw for this point
                    const SamplePoint plain = sample_point(seed, batch, (uint32_t)i, ncases, H, W, D);
                    int64_t want = voxel_offset(plain.x, plain.y, plain.z, W, D);
                    if (i < nt) {
                        const MixDraw dr = mix_words(seed, batch, (uint32_t)i);
                        const int64_t first = offsets[plain.cs], cnt = offsets[plain.cs + 1] - first;
                        if (cnt > 0) {
                            want = (int64_t)index[mix_slot(dr.r[1], first, cnt)];
                            bad += seg[plain.cs][want] <= 0;
                            ++fromIndex;
                        } else {
                            ++fallback;
                        }
                    }
                    bad += f.cs != plain.cs || f.voxel != want || out[i] != (float)(plain.cs * 4096 + (want % 4096));
                }
        }
    printf("item f %u %u %u %u %lld %lld from the index %lld fallback %lld mismatches %lld\n", ncases, H, W, D, (long long)n, (long long)nt, fromIndex,
           fallback, bad);
    for (int16_t* p : seg) free(p);
    for (float* p : fields) free(p);
    free(index); free(out);
    return bad ? 1 : 0;
}

static int big_item() {
    const int64_t n = (1ll << 31) - 1;
    long long bad = 0;
    const uint32_t blocks = loss_blocks(n), gblocks = unified_grad_blocks(n);
    bad += blocks != kLossMaxBlocks || unified_scratch_bytes(n) != tr_align((uint64_t)(kLossMaxBlocks + 2) * kUnVals * 8);
    bad += (uint64_t)gblocks * kLossThreads < (uint64_t)n || (uint64_t)(gblocks - 1) * kLossThreads >= (uint64_t)n;
    // the last point: the thread that sums it reaches it by whole strides and steps past n without wrapping
    const int64_t last = n - 1, stride = unified_stride(blocks);
    const uint32_t b = (uint32_t)((last % stride) / kLossThreads), t = (uint32_t)((last % stride) % kLossThreads);
    bad += (last - unified_first(b, t)) % stride != 0 || last + stride <= last;
    bad += unified_logit_index(last, 16, 15) != ((1ll << 31) - 2) * 16 + 15 || unified_logit_index(last, 16, 15) <= (1ll << 31);
    bad += unified_sum_index(blocks + 1, kUnVals - 1) * sizeof(double) >= unified_scratch_bytes(n);
    printf("item big mismatches %lld\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    int items = 0, failed = 0;
    for (int a = 1; a < argc;) {
        int rc;
        if (!strcmp(argv[a], "l") && a + 2 < argc) {
            rc = loss_item(atoll(argv[a + 1]), (uint32_t)atoi(argv[a + 2]));
            a += 3;
        } else if (!strcmp(argv[a], "f") && a + 6 < argc) {
            rc = field_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                            atoll(argv[a + 5]), atoll(argv[a + 6]));
            a += 7;
        } else if (!strcmp(argv[a], "big")) {
            rc = big_item();
            a += 1;
        } else {
            fprintf(stderr, "usage: unified_loss_harness (l <n> <C> | f <ncases> <H> <W> <D> <n> <nt> | big)...\n");
            return 2;
        }
        if (rc == 2) return 2;
        failed += rc;
        ++items;
    }
    printf("unified_loss_harness: %d items, %d failed\n", items, failed);
    return failed ? 1 : 0;
}
