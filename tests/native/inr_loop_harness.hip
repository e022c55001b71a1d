// The index arithmetic of the INR training loop's kernels (csrc/inr_optim.h: the Philox draw, mulhi32, the 64-bit voxel
// offsets, the norm pass's grid-stride assignment, the update's float4 / scalar units, the scratch layout of a run) on the CPU
// under AddressSanitizer + UBSan.  Every item replays a launch block by block and thread by thread with the functions the
// kernels call, over heap buffers of EXACTLY the real sizes: an index past one is an ASan report.  Items:
//   s <ncases> <M> <H> <W> <D> <n>      sample_kernel over a cache whose voxels encode their own address; every output is checked
//   o <nw> <nb>                         sqnorm_partial_kernel and adamw_kernel: every element is visited exactly once
//   r <in> <hidden> <layers> <out> <n> <M>   the regions of mrirt_inr_train_run's scratch are disjoint and inside its size
//   big                                 offsets of volumes with H W D M just under 2^31 elements and H W D just under 2^31 voxels
//                                       (arithmetic only, no allocation of the volume)
// Philox is compared with its known answers first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_optim.h"

using namespace mrirt;

static int philox_known() {
    static const uint32_t kat[3][10] = {
        { 0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u },
        { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu },
        { 0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u },
    };
    int bad = 0;
    for (int k = 0; k < 3; ++k) {
        uint32_t c[4] = { kat[k][0], kat[k][1], kat[k][2], kat[k][3] };
        philox4x32_10(c, kat[k][4], kat[k][5]);
        for (int j = 0; j < 4; ++j) bad += c[j] != kat[k][6 + j];
    }
    bad += mulhi32(0xffffffffu, 7) != 6 || mulhi32(0, 7) != 0 || mulhi32(0x80000000u, 65535) != 32767;
    printf("philox known answers: mismatches %d\n", bad);
    return bad ? 1 : 0;
}

static float enc(uint32_t c, uint32_t m, uint32_t M, int64_t v, int64_t hwd) { return (float)((((int64_t)c * M + m) * hwd + v) % 1000003); }

static int sample_item(uint32_t ncases, uint32_t M, uint32_t H, uint32_t W, uint32_t D, int64_t n) {
    const int64_t hwd = (int64_t)H * W * D;
    std::vector<float*> mods(ncases, nullptr);
    std::vector<int16_t*> seg(ncases, nullptr);
    for (uint32_t c = 0; c < ncases; ++c) {
        if (M) mods[c] = (float*)malloc((size_t)M * hwd * sizeof(float));
        seg[c] = (int16_t*)malloc((size_t)hwd * sizeof(int16_t));
        if ((M && !mods[c]) || !seg[c]) return 2;
        for (uint32_t m = 0; m < M; ++m)
            for (int64_t v = 0; v < hwd; ++v) mods[c][(int64_t)m * hwd + v] = enc(c, m, M, v, hwd);
        for (int64_t v = 0; v < hwd; ++v) seg[c][v] = (int16_t)(((int64_t)c * hwd + v) % 30011);
    }
    float* coords = (float*)malloc((size_t)n * 3 * sizeof(float));
    float* feats = M ? (float*)malloc((size_t)n * M * sizeof(float)) : nullptr;
    int32_t* labels = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    if (!coords || (M && !feats) || !labels) return 2;
    long long bad = 0;
    const uint64_t seeds[2] = { 12345u, 0xC0FFEE0000004Dull }, batches[3] = { 0, 1, (1ull << 32) + 5 };
    for (uint64_t seed : seeds)
        for (uint64_t batch : batches) {
            const uint32_t blocks = (uint32_t)((n + kOptThreads - 1) / kOptThreads);
            for (uint32_t bx = 0; bx < blocks; ++bx)
                for (uint32_t t = 0; t < kOptThreads; ++t) {           // sample_kernel
                    const int64_t i = (int64_t)bx * kOptThreads + t;
                    if (i >= n) continue;
                    const SamplePoint p = sample_point(seed, batch, (uint32_t)i, ncases, H, W, D);
                    const int64_t v = voxel_offset(p.x, p.y, p.z, W, D);
                    coords[3 * i + 0] = sample_coord(p.x, H);
                    coords[3 * i + 1] = sample_coord(p.y, W);
                    coords[3 * i + 2] = sample_coord(p.z, D);
                    labels[i] = (int32_t)seg[p.cs][v];
                    for (uint32_t k = 0; k < M; ++k) feats[i * M + k] = mods[p.cs][mod_offset(k, v, hwd)];
                    bad += p.cs >= ncases || p.x >= H || p.y >= W || p.z >= D;
                    bad += labels[i] != (int32_t)(int16_t)(((int64_t)p.cs * hwd + v) % 30011);
                    for (uint32_t k = 0; k < M; ++k) bad += feats[i * M + k] != enc(p.cs, k, M, v, hwd);
                    bad += !(coords[3 * i] >= -1.0f && coords[3 * i] <= 1.0f && coords[3 * i + 2] >= -1.0f && coords[3 * i + 2] <= 1.0f);
                }
        }
    printf("item s %u %u %u %u %u %lld mismatches %lld\n", ncases, M, H, W, D, (long long)n, bad);
    for (uint32_t c = 0; c < ncases; ++c) { free(mods[c]); free(seg[c]); }
    free(coords); free(feats); free(labels);
    return bad ? 1 : 0;
}

static int optim_item(int64_t nw, int64_t nb) {
    const int64_t n = nw + nb;
    float* w = (float*)malloc((size_t)nw * sizeof(float));
    float* b = (float*)malloc((size_t)(nb ? nb : 1) * sizeof(float));
    double* partial = (double*)malloc(opt_scratch_bytes(n));
    if (!w || !b || !partial) return 2;
    for (int64_t i = 0; i < nw; ++i) w[i] = 0.0f;
    for (int64_t i = 0; i < nb; ++i) b[i] = 0.0f;
    long long bad = 0;
    const uint32_t blocks = opt_blocks(n);
    bad += blocks < 1 || blocks > kOptMaxBlocks;
    for (uint32_t bx = 0; bx < blocks; ++bx) {               // sqnorm_partial_kernel: count the visits in the arrays themselves
        for (uint32_t t = 0; t < kOptThreads; ++t)
            for (int64_t i = opt_first(bx, t); i < n; i += opt_stride(blocks)) {
                if (i < nw) w[i] += 1.0f; else b[i - nw] += 1.0f;
            }
        partial[bx] = 1.0;
    }
    for (int64_t i = 0; i < nw; ++i) bad += w[i] != 1.0f;
    for (int64_t i = 0; i < nb; ++i) bad += b[i] != 1.0f;
    for (int al = 0; al < 4; ++al) {                         // adamw_kernel for every alignment of the two segments
        const OptUnits u = opt_units(nw, nb, (al & 1) != 0, (al & 2) != 0);
        const int64_t units = opt_unit_count(u);
        const uint32_t grid = (uint32_t)((units + kOptThreads - 1) / kOptThreads);
        for (uint32_t bx = 0; bx < grid; ++bx)
            for (uint32_t t = 0; t < kOptThreads; ++t) {
                const int64_t i = (int64_t)bx * kOptThreads + t;
                if (i >= units) continue;
                uint32_t seg, width;
                int64_t first;
                opt_unit(u, i, seg, first, width);
                bad += (width != 1 && width != 4) || (width == 4 && (first & 3) != 0) || (width == 4 && !((seg ? al & 2 : al & 1)));
                float* p = (seg ? b : w) + first;
                for (uint32_t k = 0; k < width; ++k) p[k] += 1.0f;
            }
        for (int64_t i = 0; i < nw; ++i) bad += w[i] != (float)(2 + al);
        for (int64_t i = 0; i < nb; ++i) bad += b[i] != (float)(2 + al);
    }
    printf("item o %lld %lld blocks %u mismatches %lld\n", (long long)nw, (long long)nb, blocks, bad);
    free(w); free(b); free(partial);
    return bad ? 1 : 0;
}

static int run_item(uint32_t ind, uint32_t hid, uint32_t layers, uint32_t out, int64_t n, uint32_t M) {
    const TrainLayout L = train_layout(layers, ind, hid, out, n);
    const RunLayout R = run_layout(L, n, M);
    unsigned char* s = (unsigned char*)malloc(R.bytes);
    if (!s) return 2;
    memset(s, 0, R.bytes);
    const uint64_t off[10] = { 0, R.offCoords, R.offFeats, R.offLabels, R.offLogits, R.offDlogits, R.offGw, R.offGb, R.offGnorm, R.offOpt };
    const uint64_t len[10] = { L.bytes, (uint64_t)n * 12, (uint64_t)n * M * 4, (uint64_t)n * 4, (uint64_t)n * out * 4, (uint64_t)n * out * 4,
                               R.nw * 4, R.nb * 4, 16, R.optBytes };
    long long bad = 0;
    for (int k = 0; k < 10; ++k) {
        bad += (off[k] & 255u) != 0;
        for (uint64_t i = 0; i < len[k]; ++i) { bad += s[off[k] + i] != 0; s[off[k] + i] = (unsigned char)(k + 1); }
    }
    uint64_t nw = 0, nb = 0;
    for (uint32_t l = 0; l < layers; ++l) { nw += (uint64_t)L.in[l] * L.out[l]; nb += L.out[l]; }
    bad += nw != R.nw || nb != R.nb || R.optBytes != opt_scratch_bytes((int64_t)(nw + nb));
    printf("item r %u %u %u %u %lld %u bytes %llu mismatches %lld\n", ind, hid, layers, out, (long long)n, M, (unsigned long long)R.bytes, bad);
    free(s);
    return bad ? 1 : 0;
}

static int big_item() {
    struct Vol { uint32_t M, H, W, D; };
    const Vol vols[3] = { { 8, 512, 512, 1023 }, { 8, 1290, 1290, 1290 }, { 1, 2, 2, 536870911 } };
    long long bad = 0;
    for (const Vol& v : vols) {
        const int64_t hwd = (int64_t)v.H * v.W * v.D;
        bad += hwd >= (1ll << 31);
        const unsigned __int128 total = (unsigned __int128)v.M * (unsigned __int128)hwd;
        for (uint32_t i = 0; i < 20000; ++i) {
            SamplePoint p = sample_point(99, 3, i, 65535, v.H, v.W, v.D);
            if (i == 0) { p.x = v.H - 1; p.y = v.W - 1; p.z = v.D - 1; }       // the last voxel
            const int64_t vo = voxel_offset(p.x, p.y, p.z, v.W, v.D);
            const unsigned __int128 want = ((unsigned __int128)p.x * v.W + p.y) * v.D + p.z;
            bad += p.cs >= 65535 || p.x >= v.H || p.y >= v.W || p.z >= v.D;
            bad += vo < 0 || (unsigned __int128)vo != want || vo >= hwd;
            const int64_t mo = mod_offset(v.M - 1, vo, hwd);
            bad += mo < 0 || (unsigned __int128)mo != (unsigned __int128)(v.M - 1) * hwd + want || (unsigned __int128)mo >= total;
        }
    }
    printf("item big mismatches %lld\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    int items = 0, failed = philox_known();
    for (int a = 1; a < argc;) {
        int rc;
        if (!strcmp(argv[a], "s") && a + 6 < argc) {
            rc = sample_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                             (uint32_t)atoi(argv[a + 5]), atoll(argv[a + 6]));
            a += 7;
        } else if (!strcmp(argv[a], "o") && a + 2 < argc) {
            rc = optim_item(atoll(argv[a + 1]), atoll(argv[a + 2]));
            a += 3;
        } else if (!strcmp(argv[a], "r") && a + 6 < argc) {
            rc = run_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                          atoll(argv[a + 5]), (uint32_t)atoi(argv[a + 6]));
            a += 7;
        } else if (!strcmp(argv[a], "big")) {
            rc = big_item();
            a += 1;
        } else {
            fprintf(stderr, "usage: inr_loop_harness (s <ncases> <M> <H> <W> <D> <n> | o <nw> <nb> | r <in> <hidden> <layers> <out> <n> <M> | big)...\n");
            return 2;
        }
        if (rc == 2) return 2;
        failed += rc;
        ++items;
    }
    printf("inr_loop_harness: %d items, %d failed\n", items, failed);
    return failed ? 1 : 0;
}
