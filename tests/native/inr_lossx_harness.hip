// The index arithmetic of the extended loss, the tumour-index compaction and the mixed sampler (csrc/inr_lossx.h) on the CPU
// under AddressSanitizer + UBSan.  Every item replays a launch block by block and thread by thread with the functions the
// kernels call, over heap buffers of EXACTLY the real sizes: an index past one is an ASan report.  Items:
//   l <n>                          lossx_partial / lossx_final: every point is summed exactly once, every partial-sum slot lies
//                                  inside mrirt_inr_loss_ext_scratch_bytes(n)
//   t <ncases> <H> <W> <D>         tum_chunk / tum_scan / tum_emit over random label volumes (case 0 empty, case 1 full, case 2
//                                  with the last voxel only): the index equals a plain ascending scan, in a buffer of exactly
//                                  its size, with a scratch of exactly tum_scratch_bytes
//   m <ncases> <H> <W> <D> <n> <nt>   sample_mix_kernel's draw over such a cache: every slot inside its case's range, every
//                                  decoded voxel inside the volume and a tumour voxel, the other points sample_point's
//   big                            volumes with H W D just below 2^32: chunk counts, first voxels, the decode of the last voxel
//                                  and the slot of the largest draw (arithmetic only, no such buffer)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_lossx.h"

using namespace mrirt;

static int loss_item(int64_t n) {
    const uint32_t blocks = loss_blocks(n);
    const uint64_t bytes = lossx_scratch_bytes(n);
    double* sums = (double*)malloc(bytes);
    unsigned char* seen = (unsigned char*)calloc((size_t)n, 1);
    if (!sums || !seen) return 2;
    long long bad = 0;
    bad += blocks < 1 || blocks > kLossMaxBlocks || kLossXVals > kLossXFinalThreads || kLossXVals != kLossVals + 6;
    bad += bytes < (uint64_t)(blocks + 1) * kLossXVals * sizeof(double) || (bytes & 255u) != 0;
    for (uint32_t b = 0; b < blocks; ++b) {
        for (uint32_t t = 0; t < kLossThreads; ++t)
            for (int64_t i = lossx_first(b, t); i < n; i += lossx_stride(blocks)) bad += seen[i]++ != 0;
        for (uint32_t v = 0; v < kLossXVals; ++v) sums[lossx_sum_index(b, v)] = 1.0;
    }
    for (int64_t i = 0; i < n; ++i) bad += seen[i] != 1;
    for (uint32_t v = 0; v < kLossXVals; ++v) {              // lossx_final_kernel: thread v adds the blocks, writes the totals' row
        double s = 0.0;
        for (uint32_t b = 0; b < blocks; ++b) s += sums[lossx_sum_index(b, v)];
        sums[lossx_sum_index(blocks, v)] = s;
        bad += s != (double)blocks;
    }
    printf("item l %lld blocks %u bytes %llu mismatches %lld\n", (long long)n, blocks, (unsigned long long)bytes, bad);
    free(sums); free(seen);
    return bad ? 1 : 0;
}

struct Cache {
    uint32_t ncases, H, W, D;
    uint64_t hwd;
    std::vector<int16_t*> seg;
    std::vector<int64_t> offsets;
    uint32_t* index;
    int64_t total;
};

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static int make_cache(Cache& c, uint32_t ncases, uint32_t H, uint32_t W, uint32_t D) {
    c.ncases = ncases; c.H = H; c.W = W; c.D = D; c.hwd = (uint64_t)H * W * D;
    uint64_t s = 12345u + ncases + H;
    c.offsets.assign(ncases + 1, 0);
    for (uint32_t k = 0; k < ncases; ++k) {
        int16_t* seg = (int16_t*)malloc((size_t)c.hwd * sizeof(int16_t));
        if (!seg) return 2;
        for (uint64_t v = 0; v < c.hwd; ++v)
            seg[v] = k == 0 ? 0 : k == 1 ? (int16_t)(1 + rnd(s) % 3) : k == 2 ? (int16_t)(v + 1 == c.hwd ? 3 : 0) : (int16_t)(rnd(s) % 10 == 0 ? 1 + rnd(s) % 3 : -(int16_t)(rnd(s) % 2));
        c.seg.push_back(seg);
        int64_t cnt = 0;
        for (uint64_t v = 0; v < c.hwd; ++v) cnt += seg[v] > 0;
        c.offsets[k + 1] = c.offsets[k] + cnt;
    }
    c.total = c.offsets[ncases];
    c.index = (uint32_t*)malloc((size_t)(c.total ? c.total : 1) * sizeof(uint32_t));
    return c.index ? 0 : 2;
}
static void free_cache(Cache& c) { for (int16_t* p : c.seg) free(p); free(c.index); }

static uint32_t thread_count(const int16_t* seg, uint64_t first, uint64_t hwd) {
    uint32_t n = 0;
    for (uint32_t j = 0; j < kTumPerThread; ++j) n += first + j < hwd && seg[first + j] > 0;
    return n;
}

// tum_chunk_kernel, tum_scan_kernel, tum_emit_kernel as the library launches them
static long long build_index(Cache& c) {
    long long bad = 0;
    const uint32_t chunks = tum_chunks(c.hwd);
    const uint64_t bytes = tum_scratch_bytes(c.ncases, c.hwd);
    uint32_t* sums = (uint32_t*)malloc(bytes);
    if (!sums) return 1 << 20;
    bad += bytes < (uint64_t)c.ncases * chunks * 4 || (uint64_t)chunks * kTumChunk < c.hwd || (uint64_t)(chunks - 1) * kTumChunk >= c.hwd;
    for (uint32_t cs = 0; cs < c.ncases; ++cs)
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            uint32_t t = 0;
            for (uint32_t th = 0; th < kTumThreads; ++th) t += thread_count(c.seg[cs], tum_first(ch, th), c.hwd);
            sums[tum_chunk_slot(cs, ch, chunks)] = t;
        }
    for (uint32_t cs = 0; cs < c.ncases; ++cs) {
        const uint32_t len = tum_scan_len(chunks);
        bad += (uint64_t)len * kTumThreads < chunks;
        uint32_t* s = sums + tum_chunk_slot(cs, 0, chunks);
        uint32_t lds[kTumThreads];
        for (uint32_t th = 0; th < kTumThreads; ++th) {
            uint32_t mine = 0;
            for (uint32_t j = th * len; j < th * len + len && j < chunks; ++j) mine += s[j];
            lds[th] = mine;
        }
        for (uint32_t th = 0; th < kTumThreads; ++th) {
            uint32_t before = 0;
            for (uint32_t t = 0; t < th; ++t) before += lds[t];
            for (uint32_t j = th * len; j < th * len + len && j < chunks; ++j) { const uint32_t v = s[j]; s[j] = before; before += v; }
        }
    }
    for (uint32_t cs = 0; cs < c.ncases; ++cs)
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            uint32_t lds[kTumThreads];
            for (uint32_t th = 0; th < kTumThreads; ++th) lds[th] = thread_count(c.seg[cs], tum_first(ch, th), c.hwd);
            for (uint32_t th = 0; th < kTumThreads; ++th) {
                uint32_t before = 0;
                for (uint32_t t = 0; t < th; ++t) before += lds[t];
                const int64_t lo = c.offsets[cs], hi = c.offsets[cs + 1];
                int64_t at = lo + (int64_t)sums[tum_chunk_slot(cs, ch, chunks)] + before;
                const uint64_t first = tum_first(ch, th);
                for (uint32_t j = 0; j < kTumPerThread; ++j) {
                    const uint64_t v = first + j;
                    if (v < c.hwd && c.seg[cs][v] > 0) {
                        bad += !(at >= lo && at < hi);
                        if (at >= lo && at < hi) c.index[at] = (uint32_t)v;
                        ++at;
                    }
                }
            }
        }
    free(sums);
    for (uint32_t cs = 0; cs < c.ncases; ++cs) {             // against a plain ascending scan
        int64_t at = c.offsets[cs];
        for (uint64_t v = 0; v < c.hwd; ++v)
            if (c.seg[cs][v] > 0) bad += c.index[at++] != (uint32_t)v;
        bad += at != c.offsets[cs + 1];
    }
    return bad;
}

static int tumour_item(uint32_t ncases, uint32_t H, uint32_t W, uint32_t D) {
    Cache c;
    if (make_cache(c, ncases, H, W, D)) return 2;
    const long long bad = build_index(c);
    printf("item t %u %u %u %u tumour voxels %lld mismatches %lld\n", ncases, H, W, D, (long long)c.total, bad);
    free_cache(c);
    return bad ? 1 : 0;
}

static int mix_item(uint32_t ncases, uint32_t H, uint32_t W, uint32_t D, int64_t n, int64_t nt) {
    Cache c;
    if (make_cache(c, ncases, H, W, D)) return 2;
    long long bad = build_index(c), fromIndex = 0;
    int32_t* labels = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    if (!labels) return 2;
    const uint64_t seeds[2] = { 12345u, 0xC0FFEE0000004Dull }, batches[2] = { 0, (1ull << 32) + 5 };
    for (uint64_t seed : seeds)
        for (uint64_t batch : batches)
            for (int64_t i = 0; i < n; ++i) {                // sample_mix_kernel
                const MixDraw dr = mix_words(seed, batch, (uint32_t)i);
                SamplePoint p = mix_uniform(dr, c.ncases, H, W, D);
                const SamplePoint plain = sample_point(seed, batch, (uint32_t)i, c.ncases, H, W, D);
                bad += p.cs != plain.cs || p.x != plain.x || p.y != plain.y || p.z != plain.z;
                bool used = false;
                if (i < nt) {
                    const int64_t first = c.offsets[p.cs], cnt = c.offsets[p.cs + 1] - first;
                    if (cnt > 0) {
                        const int64_t slot = mix_slot(dr.r[1], first, cnt);
                        bad += slot < first || slot >= first + cnt;
                        const uint32_t v = c.index[slot];
                        bad += v >= c.hwd;
                        tum_decode(v, W, D, p.x, p.y, p.z);
                        bad += (uint64_t)voxel_offset(p.x, p.y, p.z, W, D) != v;
                        used = true;
                        ++fromIndex;
                    }
                }
                bad += p.x >= H || p.y >= W || p.z >= D;
                labels[i] = (int32_t)c.seg[p.cs][voxel_offset(p.x, p.y, p.z, W, D)];
                bad += used && labels[i] <= 0;
            }
    printf("item m %u %u %u %u %lld %lld from the index %lld mismatches %lld\n", ncases, H, W, D, (long long)n, (long long)nt, fromIndex, bad);
    free(labels);
    free_cache(c);
    return bad ? 1 : 0;
}

static int big_item() {
    struct Vol { uint32_t H, W, D; };
    const Vol vols[4] = { { 2048, 2048, 1023 }, { 1625, 1625, 1626 }, { 2, 2, 1073741823 }, { 65535, 65537, 1 } };
    long long bad = 0;
    for (const Vol& v : vols) {
        const uint64_t hwd = (uint64_t)v.H * v.W * v.D;
        bad += hwd >= (1ull << 32);
        const uint32_t chunks = tum_chunks(hwd);
        bad += (uint64_t)chunks * kTumChunk < hwd || (uint64_t)(chunks - 1) * kTumChunk >= hwd;
        bad += tum_first(chunks - 1, kTumThreads - 1) + kTumPerThread < hwd;          // the last thread of the last chunk reaches the end
        bad += tum_first(chunks - 1, 0) >= hwd;
        bad += tum_scratch_bytes(65535, hwd) < (uint64_t)65535 * chunks * 4;
        bad += (uint64_t)tum_scan_len(chunks) * kTumThreads < chunks;
        const uint32_t probes[5] = { 0u, 1u, (uint32_t)(hwd / 2), (uint32_t)(hwd - 2), (uint32_t)(hwd - 1) };
        for (uint32_t p : probes) {
            uint32_t x, y, z;
            tum_decode(p, v.W, v.D, x, y, z);
            bad += x >= v.H || y >= v.W || z >= v.D || (uint64_t)voxel_offset(x, y, z, v.W, v.D) != p;
        }
        const int64_t cnt = (int64_t)hwd, first = (int64_t)65534 * (int64_t)hwd;          // the last of 65535 full cases
        bad += mix_slot(0xffffffffu, first, cnt) != first + cnt - 1 || mix_slot(0u, first, cnt) != first;
        bad += mix_slot(0x80000000u, first, cnt) != first + cnt / 2;
    }
    printf("item big mismatches %lld\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    int items = 0, failed = 0;
    for (int a = 1; a < argc;) {
        int rc;
        if (!strcmp(argv[a], "l") && a + 1 < argc) {
            rc = loss_item(atoll(argv[a + 1]));
            a += 2;
        } else if (!strcmp(argv[a], "t") && a + 4 < argc) {
            rc = tumour_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]));
            a += 5;
        } else if (!strcmp(argv[a], "m") && a + 6 < argc) {
            rc = mix_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                          atoll(argv[a + 5]), atoll(argv[a + 6]));
            a += 7;
        } else if (!strcmp(argv[a], "big")) {
            rc = big_item();
            a += 1;
        } else {
            fprintf(stderr, "usage: inr_lossx_harness (l <n> | t <ncases> <H> <W> <D> | m <ncases> <H> <W> <D> <n> <nt> | big)...\n");
            return 2;
        }
        if (rc == 2) return 2;
        failed += rc;
        ++items;
    }
    printf("inr_lossx_harness: %d items, %d failed\n", items, failed);
    return failed ? 1 : 0;
}
