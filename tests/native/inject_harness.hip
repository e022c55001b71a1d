// Host harness of the coordinate-injection INR (csrc/inr_inject.h): walks the scratch layout, the three-part A view, the
// tile staging, the epilogue's bounds, the Philox counter and the chunk walk of a volume exactly as csrc/inr_inject.hip's
// kernels do, thread by thread, over heap buffers of exactly the sizes the ABI states -- under AddressSanitizer + UBSan
// (tests/test_inject_host.py builds it host-only and runs it as a program).  The products are summed in increasing k in
// fp32, so on a selection net the logits it writes are the definition's bits.
//
//   inject_harness cases.bin out.bin
// cases.bin: u32 count, then per case 20 u32 { L, F, M, width[8], coordLayers, modLayers, n, H, W, D, chunk, dropout, sample }
// (H == 0: a point case with coords [n][3] and mods [n][M]; else a volume case, n = H W D, mods [M][H][W][D]), u64 seed, f32 keep,
// then B, w, b, (coords,) mods as fp32.  out.bin: per case the logits [n][C] fp32 and argmax [n] int16.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_inject.h"
#include "../../mri-raytracer_amd/csrc/siren_sincos.h"

using namespace mrirt;

template <typename T>
struct Exact {                                           // a heap block of exactly n elements: ASan guards both ends
    T* p; size_t n;
    explicit Exact(size_t count) : p((T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1)), n(count) { memset(p, 0xA5, count * sizeof(T)); }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct Drop { bool on; uint64_t seed; uint32_t thr, s; float scale; };

// inj_features_kernel, every thread of every block
static void features(const InjNet& N, const float* B, const float* coordsIn, float* coordsOut, float* feat, int64_t n, int64_t base,
                     const uint32_t hwd[3]) {
    const uint32_t half = N.F >> 1;
    const int64_t threads = ((n * half + kInjThreads - 1) / kInjThreads) * kInjThreads;
    for (int64_t t = 0; t < threads; ++t) {
        if (t >= n * (int64_t)half) continue;
        const int64_t i = t / half;
        const uint32_t j = (uint32_t)(t - i * half);
        float cx, cy, cz;
        if (coordsIn) { cx = coordsIn[3 * i]; cy = coordsIn[3 * i + 1]; cz = coordsIn[3 * i + 2]; }
        else {
            uint32_t x, y, z;
            inj_voxel(base + i, hwd[1], hwd[2], x, y, z);
            if (x >= hwd[0] || y >= hwd[1] || z >= hwd[2]) { printf("FAILED voxel %lld\n", (long long)(base + i)); exit(1); }
            cx = sample_coord(x, hwd[0]); cy = sample_coord(y, hwd[1]); cz = sample_coord(z, hwd[2]);
            if (j == 0) { coordsOut[3 * i] = cx; coordsOut[3 * i + 1] = cy; coordsOut[3 * i + 2] = cz; }
        }
        const float ux = (cx + 1.0f) * 0.5f, uy = (cy + 1.0f) * 0.5f, uz = (cz + 1.0f) * 0.5f;
        const float p = ((ux * B[3 * j]) + (uy * B[3 * j + 1])) + (uz * B[3 * j + 2]);
        float sn, cs;
        siren_sincos(6.2831855f * p, sn, cs);
        feat[i * N.F + j] = sn;
        feat[i * N.F + half + j] = cs;
    }
}

// inj_gemm_kernel<BN, EPI>: every block, every thread's staging, the epilogue's bounds
static void layer(const InjView& A, const TrView& Bv, uint32_t M, uint32_t Ncols, int64_t K, float* C, const float* bias, bool head,
                  const Drop& d, uint64_t index0, uint32_t l) {
    const int BN = Ncols <= 16 ? 16 : 64;
    const int pitchA = TrLds<64>::pitch, pitchB = BN == 16 ? TrLds<16>::pitch : TrLds<64>::pitch;
    Exact<float> As((size_t)kTrBK * pitchA), Bs((size_t)kTrBK * pitchB), acc((size_t)kTrBM * BN);
    const uint32_t mt = (M + kTrBM - 1) / kTrBM, nt = BN == 16 ? 1u : (Ncols + 63) / 64;
    for (uint32_t bx = 0; bx < mt; ++bx)
        for (uint32_t by = 0; by < nt; ++by) {
            const uint32_t m0 = bx * kTrBM, n0 = by * BN;
            for (size_t e = 0; e < acc.n; ++e) acc.p[e] = 0.0f;
            for (int64_t k0 = 0; k0 < K; k0 += kTrBK) {
                for (uint32_t t = 0; t < (uint32_t)kTrThreads; ++t) {
                    for (int i = 0; i < kTrBM / 16; ++i) {
                        uint32_t r, k;
                        tr_stage_coord<kTrBM, true>(t, i, r, k);
                        int64_t off;
                        const int src = inj_view_src(A, m0 + r, k0 + k, K, off);
                        As.p[k * pitchA + r] = src == 0 ? A.h.p[off] : src == 1 ? A.c.p[off] : src == 2 ? A.m.p[off] : 0.0f;
                    }
                    for (int i = 0; i < BN / 16; ++i) {
                        uint32_t r, k;
                        if (BN == 16) tr_stage_coord<16, false>(t, i, r, k); else tr_stage_coord<64, false>(t, i, r, k);
                        const int64_t off = tr_view_offset(Bv, n0 + r, k0 + k, K);
                        Bs.p[k * pitchB + r] = off >= 0 ? Bv.p[off] : 0.0f;
                    }
                }
                for (int kk = 0; kk < kTrBK; ++kk)
                    for (int r = 0; r < kTrBM; ++r)
                        for (int c = 0; c < BN; ++c) acc.p[r * BN + c] = acc.p[r * BN + c] + As.p[kk * pitchA + r] * Bs.p[kk * pitchB + c];
            }
            for (uint32_t t = 0; t < (uint32_t)kTrThreads; ++t) {
                const uint32_t lane = t & 63u, wave = t >> 6;
                for (int j = 0; j < BN / 16; ++j) {
                    const uint32_t col = n0 + 16u * j + tr_acc_col(lane);
                    if (col >= Ncols) continue;
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t lr = 16u * wave + tr_acc_row(lane, r), row = m0 + lr;
                        if (row >= M) continue;
                        float v = acc.p[lr * BN + (16u * j + tr_acc_col(lane))] + bias[col];
                        if (!head) v = !(v <= 0.0f) ? v : 0.0f;
                        if (!head && d.on) v = inj_mask_word(d.seed, index0 + row, d.s, l, col) < d.thr ? v * d.scale : 0.0f;
                        C[(int64_t)row * Ncols + col] = v;
                    }
                }
            }
        }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    for (uint32_t ci = 0; ci < count; ++ci) {
        uint32_t hd[20];
        uint64_t seed;
        float keep;
        if (!read_exact(f, hd, sizeof hd) || !read_exact(f, &seed, 8) || !read_exact(f, &keep, 4)) return 2;
        const uint32_t L = hd[0], F = hd[1], M = hd[2], *width = hd + 3, cl = hd[11], ml = hd[12];
        const int64_t n = hd[13];
        const uint32_t hwd[3] = { hd[14], hd[15], hd[16] };
        const int64_t chunk = hd[17];
        const bool volume = hwd[0] != 0;
        if (inj_check_shape(L, F, M, width, cl, ml) != 0) { printf("FAILED shape of case %u\n", ci); return 1; }
        const InjNet N = inj_net(L, F, M, width, cl, ml);
        Drop d = { hd[18] != 0 && keep != 1.0f, seed, hd[18] ? inj_threshold(keep) : 0u, hd[19], 1.0f / keep };
        Exact<float> B((size_t)(F / 2) * 3), w(N.nw), b(N.nb), coords(volume ? 0 : (size_t)n * 3), mods((size_t)n * M);
        if (!read_exact(f, B.p, B.n * 4) || !read_exact(f, w.p, w.n * 4) || !read_exact(f, b.p, b.n * 4) ||
            !read_exact(f, coords.p, coords.n * 4) || !read_exact(f, mods.p, mods.n * 4)) return 2;
        const int64_t per = volume ? chunk : n;
        const InjLayout Y = inj_layout(N, per);
        Exact<char> scratch(Y.bytes);
        Exact<float> logits((size_t)n * N.C);
        Exact<int16_t> am((size_t)n);
        const uint64_t passes = volume ? inj_passes(n, chunk) : 1;
        int64_t covered = 0;
        for (uint64_t p = 0; p < passes; ++p) {
            int64_t first = 0, len = n;
            if (volume) inj_pass_range(n, chunk, p, first, len);
            if (first != covered || len < 1 || len > per) { printf("FAILED pass %llu of case %u\n", (unsigned long long)p, ci); return 1; }
            covered += len;
            float* sc = (float*)(scratch.p + Y.offCoords);
            features(N, B.p, volume ? nullptr : coords.p, sc, (float*)(scratch.p + Y.offFeat), len, first, hwd);
            const float* cp = volume ? sc : coords.p;
            const float* mp = M ? mods.p + (volume ? first : 0) : nullptr;
            for (uint32_t l = 0; l < L; ++l) {
                const bool head = l + 1 == L;
                const float* h = l == 0 ? (const float*)(scratch.p + Y.offFeat) : (const float*)(scratch.p + inj_act_offset(Y, l - 1));
                const InjView A = inj_layer_view(N, l, len, h, cp, mp, volume ? 1 : (int64_t)M, volume ? n : 1);
                const TrView Bv = TrView{ w.p + N.wOff[l], 1, (int64_t)N.out[l], N.out[l], 0u };
                float* C = head ? logits.p + first * N.C : (float*)(scratch.p + inj_act_offset(Y, l));
                layer(A, Bv, (uint32_t)len, N.out[l], N.in[l], C, b.p + N.bOff[l], head, d, (uint64_t)first, l);
            }
            for (int64_t i = 0; i < len; ++i) am.p[first + i] = (int16_t)inj_argmax(logits.p + (first + i) * N.C, N.C);
        }
        if (covered != n) { printf("FAILED coverage of case %u\n", ci); return 1; }
        fwrite(logits.p, 4, logits.n, o);
        fwrite(am.p, 2, am.n, o);
        printf("case %u scratch %llu passes %llu\n", ci, (unsigned long long)Y.bytes, (unsigned long long)passes);
    }
    fclose(o);
    fclose(f);
    printf("inject_harness: %u cases done\n", count);
    return 0;
}
