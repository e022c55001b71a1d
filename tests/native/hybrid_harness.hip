// The index arithmetic and the draws of the hybrid sampler (csrc/inr_hybrid.h) on the CPU under AddressSanitizer + UBSan.  Every
// item replays a launch block by block and thread by thread with the functions the kernels call, over heap buffers of EXACTLY
// the real sizes: an index past one is an ASan report.  Items:
//   c <ncases> <H> <W> <D> <C>            cls_chunk / cls_scan / cls_emit: every slot of the chunk sums inside
//                                         mrirt_inr_class_index_scratch_bytes, every index slot written exactly once and equal
//                                         to the (class, case, offset) order; cls_case_of at both ends of every list
//   s <n> <k> <pattern>                   select_largest_kernel's per-thread steps (histogram, digit, ranks, emit) against a
//                                         stable sort; pattern 0 equal, 1 distinct, 2 eight values, 3 low byte, 4 high byte, 5 specials
//   r <ncases> <H> <W> <D> <C> <n> <U> <P>   sample_hybrid_kernel's rows: every read inside its buffer, class rows on voxels of
//                                         their class (or the fallback), uniform rows those of sample_point
//   z                                     nrm_of_words at the edge words; mulhi64 against unsigned __int128
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_hybrid.h"

using namespace mrirt;

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

// labels -1 .. C and 32767; case 0 lacks class C - 1 (when C > 1); class 1 is absent everywhere when C > 2
static int16_t label_of(uint64_t& s, uint32_t cs, uint32_t C) {
    const uint32_t r = rnd(s) % (C + 3);
    int16_t lab = r == C + 2 ? (int16_t)32767 : (int16_t)((int)r - 1);
    if (C > 2 && lab == 1) lab = 0;
    if (C > 1 && cs == 0 && lab == (int16_t)(C - 1)) lab = 0;
    return lab;
}

struct Cache {
    std::vector<int16_t*> seg;
    std::vector<int64_t> offsets;
    uint32_t* index = nullptr;
    int64_t total = 0;
};

static void build_naive(Cache& c, uint32_t ncases, uint64_t hwd, uint32_t C, uint64_t seed) {
    uint64_t s = seed;
    for (uint32_t k = 0; k < ncases; ++k) {
        int16_t* sg = (int16_t*)malloc((size_t)hwd * sizeof(int16_t));
        for (uint64_t v = 0; v < hwd; ++v) sg[v] = label_of(s, k, C);
        c.seg.push_back(sg);
    }
    c.offsets.assign((size_t)C * ncases + 1, 0);
    for (uint32_t k = 0; k < C; ++k)
        for (uint32_t cs = 0; cs < ncases; ++cs) {
            int64_t cnt = 0;
            for (uint64_t v = 0; v < hwd; ++v) cnt += c.seg[cs][v] == (int16_t)k;
            c.offsets[cls_list(k, cs, ncases) + 1] = c.offsets[cls_list(k, cs, ncases)] + cnt;
        }
    c.total = c.offsets[(size_t)C * ncases];
    c.index = (uint32_t*)malloc((size_t)(c.total ? c.total : 1) * sizeof(uint32_t));
    for (uint32_t k = 0; k < C; ++k)
        for (uint32_t cs = 0; cs < ncases; ++cs) {
            int64_t at = c.offsets[cls_list(k, cs, ncases)];
            for (uint64_t v = 0; v < hwd; ++v)
                if (c.seg[cs][v] == (int16_t)k) c.index[at++] = (uint32_t)v;
        }
}

static void free_cache(Cache& c) {
    for (int16_t* p : c.seg) free(p);
    free(c.index);
}

static int class_item(uint32_t ncases, uint32_t H, uint32_t W, uint32_t D, uint32_t C) {
    const uint64_t hwd = (uint64_t)H * W * D;
    Cache ref;
    build_naive(ref, ncases, hwd, C, 99u + hwd + C);
    const uint32_t chunks = tum_chunks(hwd);
    const uint64_t bytes = cls_scratch_bytes(ncases, hwd, C);
    uint32_t* sums = (uint32_t*)malloc(bytes);
    uint32_t* index = (uint32_t*)malloc((size_t)(ref.total ? ref.total : 1) * sizeof(uint32_t));
    unsigned char* wrote = (unsigned char*)calloc((size_t)(ref.total ? ref.total : 1), 1);
    if (!sums || !index || !wrote) return 2;
    long long bad = 0;
    bad += bytes < (uint64_t)ncases * chunks * C * 4 || (bytes & 255u) != 0;
    for (uint32_t cs = 0; cs < ncases; ++cs)                       // cls_chunk_kernel
        for (uint32_t b = 0; b < chunks; ++b) {
            uint32_t hist[kLossMaxClasses] = { 0 };
            for (uint32_t t = 0; t < kTumThreads; ++t)
                for (uint32_t j = 0; j < kTumPerThread; ++j) {
                    const uint64_t v = tum_first(b, t) + j;
                    if (v < hwd && cls_in(ref.seg[cs][v], C)) ++hist[ref.seg[cs][v]];
                }
            for (uint32_t t = 0; t < kTumThreads; ++t)
                if (t < C) sums[cls_chunk_slot(cs, b, t, chunks, C)] = hist[t];
        }
    for (uint32_t cs = 0; cs < ncases; ++cs)                       // cls_scan_kernel, grid (ncases, C)
        for (uint32_t k = 0; k < C; ++k) {
            uint32_t lds[kTumThreads];
            const uint32_t len = tum_scan_len(chunks);
            for (uint32_t t = 0; t < kTumThreads; ++t) {
                uint32_t mine = 0;
                for (uint32_t j = t * len; j < t * len + len && j < chunks; ++j) mine += sums[cls_chunk_slot(cs, j, k, chunks, C)];
                lds[t] = mine;
            }
            for (uint32_t t = 0; t < kTumThreads; ++t) {
                uint32_t before = 0;
                for (uint32_t u = 0; u < t; ++u) before += lds[u];
                for (uint32_t j = t * len; j < t * len + len && j < chunks; ++j) {
                    uint32_t* s = sums + cls_chunk_slot(cs, j, k, chunks, C);
                    const uint32_t c = *s;
                    *s = before;
                    before += c;
                }
            }
        }
    for (uint32_t cs = 0; cs < ncases; ++cs)                       // cls_emit_kernel
        for (uint32_t b = 0; b < chunks; ++b)
            for (uint32_t k = 0; k < C; ++k) {
                uint32_t lds[kTumThreads];
                for (uint32_t t = 0; t < kTumThreads; ++t) {
                    uint32_t mine = 0;
                    for (uint32_t j = 0; j < kTumPerThread; ++j) {
                        const uint64_t v = tum_first(b, t) + j;
                        mine += v < hwd && ref.seg[cs][v] == (int16_t)k;
                    }
                    lds[t] = mine;
                }
                const uint32_t list = cls_list(k, cs, ncases);
                const int64_t lo = ref.offsets[list], hi = ref.offsets[list + 1];
                for (uint32_t t = 0; t < kTumThreads; ++t) {
                    uint32_t before = 0;
                    for (uint32_t u = 0; u < t; ++u) before += lds[u];
                    int64_t at = lo + (int64_t)sums[cls_chunk_slot(cs, b, k, chunks, C)] + before;
                    for (uint32_t j = 0; j < kTumPerThread; ++j) {
                        const uint64_t v = tum_first(b, t) + j;
                        if (v < hwd && ref.seg[cs][v] == (int16_t)k) {
                            if (at >= lo && at < hi) { bad += wrote[at]++ != 0; index[at] = (uint32_t)v; }
                            else ++bad;
                            ++at;
                        }
                    }
                }
            }
    for (int64_t e = 0; e < ref.total; ++e) bad += wrote[e] != 1 || index[e] != ref.index[e];
    long long searched = 0;
    for (uint32_t k = 0; k < C; ++k)                               // the binary search at both ends of every list
        for (uint32_t cs = 0; cs < ncases; ++cs) {
            const int64_t lo = ref.offsets[cls_list(k, cs, ncases)], hi = ref.offsets[cls_list(k, cs, ncases) + 1];
            if (hi > lo) {
                bad += cls_case_of(ref.offsets.data(), k, ncases, lo) != cs || cls_case_of(ref.offsets.data(), k, ncases, hi - 1) != cs;
                searched += 2;
            }
        }
    printf("item c %u %u %u %u %u chunks %u bytes %llu voxels %lld searched %lld mismatches %lld\n", ncases, H, W, D, C, chunks,
           (unsigned long long)bytes, (long long)ref.total, searched, bad);
    free(sums); free(index); free(wrote);
    free_cache(ref);
    return bad ? 1 : 0;
}

static float pattern_value(uint32_t pattern, uint32_t i, uint64_t& s) {
    union { float f; uint32_t u; } c;
    switch (pattern) {
        case 0: return 0.25f;
        case 1: c.u = 0x3F000000u + (uint32_t)(((uint64_t)i * 2654435761u) % 8388608u); return c.f;      // distinct: an odd multiplier mod 2^23
        case 2: return (float)(rnd(s) % 8) - 3.0f;
        case 3: c.u = 0x40490F00u | (rnd(s) & 0xFFu); return c.f;
        case 4: c.u = ((rnd(s) & 0x7Fu) << 24) | 0x00345678u; if ((c.u & 0x7F800000u) == 0x7F800000u) c.u &= ~0x00800000u; return c.f;
        default: {
            static const uint32_t sp[] = { 0x7FC00000u, 0xFFC00001u, 0x7F800000u, 0xFF800000u, 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u,
                                           0xBF800000u, 0x3F800000u, 0x007FFFFFu, 0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800001u };
            c.u = sp[rnd(s) % (sizeof sp / sizeof sp[0])];
            return c.f;
        }
    }
}

static int select_item(uint32_t n, uint32_t k, uint32_t pattern) {
    float* values = (float*)malloc((size_t)n * sizeof(float));
    uint32_t* out = (uint32_t*)malloc((size_t)k * sizeof(uint32_t));
    if (!values || !out) return 2;
    uint64_t s = 5u + n + pattern;
    for (uint32_t i = 0; i < n; ++i) values[i] = pattern_value(pattern, i, s);
    long long bad = 0;
    uint32_t prefix = 0, need = k, equal = n;
    for (uint32_t pass = 0; pass < kSelPasses; ++pass) {
        uint32_t hist[kSelBins] = { 0 };
        const uint32_t shift = sel_shift(pass), mask = sel_mask(pass);
        for (uint32_t t = 0; t < kSelThreads; ++t)
            for (uint32_t i = t; i < n; i += kSelThreads) {
                const uint32_t key = sel_key(values[i]);
                if ((key & mask) == prefix) ++hist[(key >> shift) & 0xFFu];
            }
        uint32_t found = 0, digit = 0, aboveOf = 0;
        for (uint32_t t = 0; t < kSelThreads; ++t)
            if (t < kSelBins) {
                const uint32_t above = sel_above(hist, t);
                if (sel_is_digit(above, hist[t], need)) { digit = t; aboveOf = above; ++found; }
            }
        bad += found != 1;
        prefix |= digit << shift;
        need -= aboveOf;
        equal = hist[digit];
    }
    bad += need < 1 || need > equal;
    std::vector<uint32_t> eq(kSelThreads), take(kSelThreads);
    std::vector<unsigned char> seen(n, 0);
    for (uint32_t t = 0; t < kSelThreads; ++t) {
        const uint32_t lo = sel_first(t, n), hi = sel_first(t + 1, n);
        bad += lo > hi || hi > n;
        uint32_t e = 0;
        for (uint32_t i = lo; i < hi; ++i) { e += sel_key(values[i]) == prefix; bad += seen[i]++ != 0; }
        eq[t] = e;
    }
    for (uint32_t i = 0; i < n; ++i) bad += seen[i] != 1;
    uint32_t rankBefore = 0;
    for (uint32_t t = 0; t < kSelThreads; ++t) {
        uint32_t r = rankBefore, c = 0;
        for (uint32_t i = sel_first(t, n); i < sel_first(t + 1, n); ++i) {
            const uint32_t key = sel_key(values[i]);
            c += sel_takes(key, prefix, r, equal, need);
            r += key == prefix;
        }
        take[t] = c;
        rankBefore += eq[t];
    }
    uint32_t at = 0;
    rankBefore = 0;
    for (uint32_t t = 0; t < kSelThreads; ++t) {
        uint32_t r = rankBefore, mine = at;
        for (uint32_t i = sel_first(t, n); i < sel_first(t + 1, n); ++i) {
            const uint32_t key = sel_key(values[i]);
            if (sel_takes(key, prefix, r, equal, need)) {
                if (mine < k) out[mine] = i;
                else ++bad;
                ++mine;
            }
            r += key == prefix;
        }
        at += take[t];
        rankBefore += eq[t];
    }
    bad += at != k;
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sel_key(values[a]) < sel_key(values[b]); });
    std::vector<uint32_t> want(order.end() - k, order.end());
    std::sort(want.begin(), want.end());
    for (uint32_t i = 0; i < k && at == k; ++i) bad += out[i] != want[i];
    printf("item s %u %u %u threshold %08x need %u of %u mismatches %lld\n", n, k, pattern, prefix, need, equal, bad);
    free(values); free(out);
    return bad ? 1 : 0;
}

static int rows_item(uint32_t ncases, uint32_t H, uint32_t W, uint32_t D, uint32_t C, int64_t n, int64_t U, int64_t P) {
    const int64_t hwd = (int64_t)H * W * D;
    Cache ref;
    build_naive(ref, ncases, (uint64_t)hwd, C, 31u + ncases + D);
    uint32_t* picks = (uint32_t*)malloc((size_t)(U ? U : 1) * sizeof(uint32_t));
    int32_t* labels = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    if (!picks || !labels) return 2;
    uint64_t s = 17;
    for (int64_t i = 0; i < U; ++i) picks[i] = i == 0 ? 0u : i == 1 ? 0xFFFFFFFFu : i == 2 ? picks[0] : rnd(s);
    long long bad = 0, fromIndex = 0, fallback = 0;
    const uint64_t seeds[2] = { 42u, 0xC0FFEE0000004Dull }, batches[2] = { 0, (1ull << 32) + 5 };
    for (uint64_t seed : seeds)
        for (uint64_t batch : batches)
            for (uint32_t b = 0; b < (uint32_t)((n + kOptThreads - 1) / kOptThreads); ++b)
                for (uint32_t t = 0; t < kOptThreads; ++t) {
                    const int64_t i = (int64_t)b * kOptThreads + t;
                    if (i >= n) continue;
                    const SamplePoint p = hyb_row(seed, batch, (uint32_t)i, U, P, C, U ? picks : nullptr, P ? ref.index : nullptr,
                                                  P ? ref.offsets.data() : nullptr, ncases, H, W, D, hwd);
                    bad += p.cs >= ncases || p.x >= H || p.y >= W || p.z >= D;
                    if (p.cs >= ncases) continue;
                    const int64_t v = voxel_offset(p.x, p.y, p.z, W, D);
                    bad += v < 0 || v >= hwd;
                    labels[i] = ref.seg[p.cs][v];
                    const SamplePoint plain = sample_point(seed, batch, (uint32_t)i, ncases, H, W, D);
                    if (i < U) {
                        const SamplePoint cand = mix_uniform(hyb_words(seed, batch, picks[i], 1u), ncases, H, W, D);
                        bad += cand.cs != p.cs || cand.x != p.x || cand.y != p.y || cand.z != p.z;
                    } else if (i < U + (int64_t)C * P) {
                        const uint32_t k = (uint32_t)((i - U) / P);
                        const int64_t total = ref.offsets[cls_list(k + 1, 0, ncases)] - ref.offsets[cls_list(k, 0, ncases)];
                        if (total > 0) { bad += labels[i] != (int32_t)k; ++fromIndex; }
                        else { bad += plain.cs != p.cs || plain.x != p.x || plain.y != p.y || plain.z != p.z; ++fallback; }
                    } else {
                        bad += plain.cs != p.cs || plain.x != p.x || plain.y != p.y || plain.z != p.z;
                    }
                }
    printf("item r %u %u %u %u %u %lld %lld %lld from the index %lld fallback %lld mismatches %lld\n", ncases, H, W, D, C, (long long)n, (long long)U,
           (long long)P, fromIndex, fallback, bad);
    free(picks); free(labels);
    free_cache(ref);
    return bad ? 1 : 0;
}

static int edge_item() {
    long long bad = 0;
    const uint32_t r0s[] = { 0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu }, r1s[] = { 0u, 1u, 1u << 30, 1u << 31, 0xC0000000u, 0xFFFFFFFFu };
    for (uint32_t r0 : r0s)
        for (uint32_t r1 : r1s) {
            const uint32_t r[4] = { r0, r1, r1 ^ 0x5555u, r0 };
            const Normal3 z = nrm_of_words(r);
            const double R = std::sqrt(-2.0 * std::log(((double)r0 + 1.0) / 4294967296.0));
            bad += !std::isfinite(z.x) || !std::isfinite(z.y) || !std::isfinite(z.z);
            bad += std::fabs((double)z.x) > R * (1.0 + 1e-6) + 1e-30 || std::fabs((double)z.y) > R * (1.0 + 1e-6) + 1e-30;
            bad += R > 6.7;                                           // sqrt(2 * 32 * ln 2) = 6.66: no word gives a longer normal
            if (r0 == 0xFFFFFFFFu) bad += z.x != 0.0f || z.y != 0.0f;  // u1 == 1: R == 0
            if (r1 == 0u) bad += z.x != (float)R || z.y != 0.0f;
        }
    uint64_t s = 3;
    for (int i = 0; i < 4096; ++i) {
        const uint64_t a = ((uint64_t)rnd(s) << 33) ^ ((uint64_t)rnd(s) << 2) ^ rnd(s), b = i % 3 ? ((uint64_t)rnd(s) << 20) | rnd(s) : rnd(s);
        bad += mulhi64(a, b) != (uint64_t)(((unsigned __int128)a * b) >> 64);
    }
    bad += mulhi64(~0ull, ~0ull) != ~0ull - 1 || mulhi64(~0ull, 1) != 0 || mulhi64(~0ull, 7) != 6;
    bad += sel_key_bits(0x80000000u) >= sel_key_bits(0u) || sel_key_bits(0x7F800000u) >= sel_key_bits(0x7FC00000u) ||
           sel_key_bits(0xFFC00000u) != 0xFFFFFFFFu || sel_key_bits(0xFF800000u) != 0x007FFFFFu;
    bad += sel_mask(0) != 0u || sel_mask(1) != 0xFF000000u || sel_mask(3) != 0xFFFFFF00u || sel_shift(0) != 24u || sel_shift(3) != 0u;
    printf("item z mismatches %lld\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    int items = 0, failed = 0;
    for (int a = 1; a < argc;) {
        int rc;
        if (!strcmp(argv[a], "c") && a + 5 < argc) {
            rc = class_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                            (uint32_t)atoi(argv[a + 5]));
            a += 6;
        } else if (!strcmp(argv[a], "s") && a + 3 < argc) {
            rc = select_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]));
            a += 4;
        } else if (!strcmp(argv[a], "r") && a + 8 < argc) {
            rc = rows_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                           (uint32_t)atoi(argv[a + 5]), atoll(argv[a + 6]), atoll(argv[a + 7]), atoll(argv[a + 8]));
            a += 9;
        } else if (!strcmp(argv[a], "z")) {
            rc = edge_item();
            a += 1;
        } else {
            fprintf(stderr, "usage: hybrid_harness (c <ncases> <H> <W> <D> <C> | s <n> <k> <pattern> | r <ncases> <H> <W> <D> <C> <n> <U> <P> | z)...\n");
            return 2;
        }
        if (rc == 2) return 2;
        failed += rc;
        ++items;
    }
    printf("hybrid_harness: %d items, %d failed\n", items, failed);
    return failed ? 1 : 0;
}
