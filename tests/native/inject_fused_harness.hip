// Host harness of the fused forward of the coordinate-injection INR (csrc/inr_inject_fused.h): walks the weight staging with
// its padding, each wave's A-buffer assembly of [h | coords | mods | 0], the fragment reads of every MFMA step, the epilogue
// writes and the row guards against the count exactly as csrc/inr_inject_fused.hip's kernel does, lane by lane, over heap
// buffers of exactly the sizes the layout and the row count state -- under AddressSanitizer + UBSan
// (tests/test_inject_fused_host.py builds it host-only and runs it as a program).  The inputs and outputs hold exactly
// min(count, n_max) rows, so touching a row at or beyond the count is a heap overflow.  The products are summed in
// increasing k in fp32, so on a selection or integer net the logits it writes are the definition's bits.
//
//   inject_fused_harness cases.bin out.bin
// cases.bin: u32 count, then per case 16 u32 { L, F, M, width[8], coordLayers, modLayers, n_max, have_count, count }, then B, w, b,
// coords [rows][3], mods [rows][M] as fp32 (rows = min(count, n_max), or n_max).  out.bin: per case logits [rows][C] fp32 and
// argmax [rows] int16.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mri-raytracer_amd/csrc/inr_inject_fused.h"

using namespace mrirt;

template <typename T>
struct Exact {                                           // a heap block of exactly n elements: ASan guards both ends
    T* p; size_t n;
    explicit Exact(size_t count) : p((T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1)), n(count) { memset(p, 0xA5, count * sizeof(T)); }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

constexpr uint32_t kGrid = 2;                            // workgroups of the emulated launch: tiles are dealt by a grid stride

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t cases = 0;
    if (!read_exact(f, &cases, 4)) return 2;
    for (uint32_t ci = 0; ci < cases; ++ci) {
        uint32_t hd[16];
        if (!read_exact(f, hd, sizeof hd)) return 2;
        const uint32_t L = hd[0], F = hd[1], M = hd[2], *width = hd + 3, cl = hd[11], ml = hd[12], nMax = hd[13];
        if (inj_check_shape(L, F, M, width, cl, ml) != 0) { printf("FAILED shape of case %u\n", ci); return 1; }
        const InjNet N = inj_net(L, F, M, width, cl, ml);
        const InjFusedLayout Y = inj_fused_layout(N);
        if (!inj_fused_fits(Y) || Y.bytes % 16 != 0) { printf("FAILED fit of case %u\n", ci); return 1; }
        const uint32_t n = fused_rows(nMax, hd[14] != 0, hd[15]);
        Exact<float> B((size_t)(F / 2) * 3), w(N.nw), b(N.nb), coords((size_t)n * 3), mods((size_t)n * M);
        if (!read_exact(f, B.p, B.n * 4) || !read_exact(f, w.p, w.n * 4) || !read_exact(f, b.p, b.n * 4) ||
            !read_exact(f, coords.p, coords.n * 4) || !read_exact(f, mods.p, mods.n * 4)) return 2;
        Exact<float> logits((size_t)n * N.C);
        Exact<int16_t> am((size_t)n);
        const uint32_t half = F >> 1;
        for (uint32_t block = 0; block < kGrid; ++block) {
            Exact<float> ldsBlock((size_t)(Y.bytes / sizeof(float)));      // one workgroup's dynamic LDS
            float* lds = ldsBlock.p;
            // staging, every thread
            for (uint32_t t = 0; t < kFusedThreads; ++t) {
                for (uint32_t l = 0; l < L; ++l) {
                    for (uint32_t e = t; e < Y.kPad[l] * Y.pitch[l]; e += kFusedThreads) {
                        const int64_t src = fused_stage_src(N, Y, l, e);
                        lds[Y.wOff[l] + e] = src >= 0 ? w.p[src] : 0.0f;
                    }
                    for (uint32_t c = t; c < Y.outPad[l]; c += kFusedThreads) lds[Y.bOff[l] + c] = c < N.out[l] ? b.p[N.bOff[l] + c] : 0.0f;
                }
                for (uint32_t e = t; e < half * 3u; e += kFusedThreads) lds[Y.offB + e] = B.p[e];
            }
            const uint32_t tiles = (uint32_t)(((uint64_t)n + kFusedTileRows - 1) / kFusedTileRows);
            for (uint32_t tile = block; tile < tiles; tile += kGrid)
                for (uint32_t wave = 0; wave < kFusedWaves; ++wave) {
                    const uint32_t buf0 = Y.offWave + wave * Y.waveFloats, buf1 = buf0 + Y.bufFloats[0];
                    const uint32_t row0 = tile * kFusedTileRows + wave * kFusedWaveRows;
                    if (row0 >= n) continue;
                    float c3[64][3], ext[64][kFusedExt];
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        const uint32_t r16 = lane & 15u, g = lane >> 4, row = row0 + r16;
                        const bool valid = row < n;
                        for (int k = 0; k < 3; ++k) c3[lane][k] = valid ? coords.p[3 * (size_t)row + k] : 0.0f;
                        for (uint32_t i = 0; i < kFusedExt; ++i) {
                            const uint32_t e = g + 4u * i;
                            ext[lane][i] = e < 3u ? c3[lane][g] : (valid && e - 3u < M) ? mods.p[(size_t)row * M + (e - 3u)] : 0.0f;
                        }
                        for (uint32_t j = g; j < half; j += 4u) {
                            float sn, cs;
                            inj_feature(c3[lane][0], c3[lane][1], c3[lane][2], lds[Y.offB + 3 * j], lds[Y.offB + 3 * j + 1], lds[Y.offB + 3 * j + 2], sn, cs);
                            lds[buf0 + fused_a_index(j, r16)] = sn;
                            lds[buf0 + fused_a_index(half + j, r16)] = cs;
                        }
                    }
                    for (uint32_t l = 0; l < L; ++l) {
                        float* in = lds + ((l & 1u) ? buf1 : buf0);
                        float* out = lds + ((l & 1u) ? buf0 : buf1);
                        for (uint32_t lane = 0; lane < 64; ++lane) {
                            for (uint32_t i = 0; i < kFusedExt; ++i) {
                                const int k = fused_ext_k(N, l, (lane >> 4) + 4u * i);
                                if (k >= 0) in[fused_a_index((uint32_t)k, lane & 15u)] = ext[lane][i];
                            }
                            if (lane < (Y.kPad[l] - N.in[l]) * kFusedWaveRows) in[fused_a_index(N.in[l], 0) + lane] = 0.0f;
                        }
                        const bool head = l + 1u == L;
                        const uint32_t nt = Y.outPad[l] >> 4;
                        for (uint32_t j0 = 0; j0 < nt; j0 += kFusedGroup) {
                            const uint32_t NT = nt - j0 < kFusedGroup ? nt - j0 : kFusedGroup;
                            float acc[kFusedGroup][64][4] = {};
                            for (uint32_t s = 0; s < Y.kPad[l] / 4; ++s) {
                                float av[64], bv[kFusedGroup][64];
                                for (uint32_t lane = 0; lane < 64; ++lane) {
                                    av[lane] = in[fused_frag_a(s, lane)];
                                    for (uint32_t j = 0; j < NT; ++j) bv[j][lane] = lds[fused_frag_b(Y, l, s, j0 + j, lane)];
                                }
                                // v_mfma_f32_16x16x4_f32: operand lane q holds A[row q & 15][k q >> 4] and B[k q >> 4][col q & 15]
                                for (uint32_t j = 0; j < NT; ++j)
                                    for (uint32_t lane = 0; lane < 64; ++lane)
                                        for (int r = 0; r < 4; ++r)
                                            for (uint32_t k = 0; k < 4; ++k)
                                                acc[j][lane][r] = acc[j][lane][r] + av[16 * k + 4 * (lane >> 4) + r] * bv[j][16 * k + (lane & 15u)];
                            }
                            for (uint32_t j = 0; j < NT; ++j)
                                for (uint32_t lane = 0; lane < 64; ++lane) {
                                    const uint32_t col = 16u * (j0 + j) + (lane & 15u);
                                    if (col >= N.out[l]) continue;
                                    const float bias = lds[Y.bOff[l] + col];
                                    for (int r = 0; r < 4; ++r) {
                                        float t = acc[j][lane][r] + bias;
                                        if (!head) t = !(t <= 0.0f) ? t : 0.0f;
                                        out[fused_epi_index(j0 + j, lane) + r] = t;
                                        const uint32_t row = row0 + 4u * (lane >> 4) + r;
                                        if (head && row < n) logits.p[(size_t)row * N.C + col] = t;
                                    }
                                }
                        }
                    }
                    for (uint32_t lane = 0; lane < kFusedWaveRows; ++lane)
                        if (row0 + lane < n)
                            am.p[row0 + lane] = (int16_t)inj_argmax_strided(lds + ((L & 1u) ? buf1 : buf0) + fused_a_index(0, lane), N.C, kFusedWaveRows);
                }
        }
        fwrite(logits.p, 4, logits.n, o);
        fwrite(am.p, 2, am.n, o);
        printf("case %u lds %llu rows %u\n", ci, (unsigned long long)Y.bytes, n);
    }
    fclose(o);
    fclose(f);
    printf("inject_fused_harness: %u cases done\n", cases);
    return 0;
}
