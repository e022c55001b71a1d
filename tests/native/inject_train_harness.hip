// Host harness of the coordinate-injection INR's training step (csrc/inr_inject.h): walks the step's scratch layout, the
// transposed three-part view with its row of ones, the slab ranges, the tile staging and the epilogues' bounds exactly as
// csrc/inr_inject_train.hip's kernels do, thread by thread, over heap buffers of exactly the sizes the ABI states -- under
// AddressSanitizer + UBSan (tests/test_inject_train_host.py builds it host-only and runs it as a program).  Every sum is the
// k-ordered chain acc <- float(double(acc) + double(a) double(b)) of tests/inject_ref.py's matmul32, so the gradients it
// writes are the definition's bits.
//
//   inject_train_harness cases.bin out.bin
// cases.bin: u32 count, then per case 16 u32 { L, F, M, width[8], coordLayers, modLayers, n, dropout, sample }, u64 seed,
// f32 keep, u32 accumulate, then B, w, b, coords [n][3], mods [n][M], dlogits [n][C] and, when accumulating, the old grad_B,
// grad_w, grad_b, all fp32.  out.bin: per case logits [n][C], grad_B, grad_w, grad_b.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
static float chain(float acc, float a, float b) { return (float)((double)acc + (double)a * (double)b); }

// One launch of a 64 x BN tile kernel: every block, every thread's staging of both operands (R / 16 elements each), the
// chain over the staged tile, the epilogue's bounds.  fa(non, k, kEnd) / fb(non, k, kEnd) read one operand element through
// its view; ep(row, col, v) stores.
template <bool AKFAST, bool BKFAST, class FA, class FB, class EP>
static void tiles(uint32_t M, uint32_t N, int64_t kBegin, int64_t kEnd, FA fa, FB fb, EP ep) {
    const int BN = N <= 16 ? 16 : 64;
    const int pitchA = TrLds<64>::pitch, pitchB = BN == 16 ? TrLds<16>::pitch : TrLds<64>::pitch;
    Exact<float> As((size_t)kTrBK * pitchA), Bs((size_t)kTrBK * pitchB), acc((size_t)kTrBM * BN);
    const uint32_t mt = (M + kTrBM - 1) / kTrBM, nt = BN == 16 ? 1u : (N + 63) / 64;
    for (uint32_t bx = 0; bx < mt; ++bx)
        for (uint32_t by = 0; by < nt; ++by) {
            const uint32_t m0 = bx * kTrBM, n0 = by * BN;
            for (size_t e = 0; e < acc.n; ++e) acc.p[e] = 0.0f;
            for (int64_t k0 = kBegin; k0 < kEnd; k0 += kTrBK) {
                for (uint32_t t = 0; t < (uint32_t)kTrThreads; ++t) {
                    for (int i = 0; i < kTrBM / 16; ++i) {
                        uint32_t r, k;
                        tr_stage_coord<kTrBM, AKFAST>(t, i, r, k);
                        As.p[k * pitchA + r] = fa(m0 + r, k0 + k, kEnd);
                    }
                    for (int i = 0; i < BN / 16; ++i) {
                        uint32_t r, k;
                        if (BN == 16) tr_stage_coord<16, BKFAST>(t, i, r, k); else tr_stage_coord<64, BKFAST>(t, i, r, k);
                        Bs.p[k * pitchB + r] = fb(n0 + r, k0 + k, kEnd);
                    }
                }
                for (int kk = 0; kk < kTrBK; ++kk)
                    for (int r = 0; r < kTrBM; ++r)
                        for (int c = 0; c < BN; ++c) acc.p[r * BN + c] = chain(acc.p[r * BN + c], As.p[kk * pitchA + r], Bs.p[kk * pitchB + c]);
            }
            for (uint32_t t = 0; t < (uint32_t)kTrThreads; ++t) {
                const uint32_t lane = t & 63u, wave = t >> 6;
                for (int j = 0; j < BN / 16; ++j) {
                    const uint32_t col = n0 + 16u * j + tr_acc_col(lane);
                    if (col >= N) continue;
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t lr = 16u * wave + tr_acc_row(lane, r), row = m0 + lr;
                        if (row >= M) continue;
                        ep(row, col, acc.p[lr * BN + (16u * j + tr_acc_col(lane))]);
                    }
                }
            }
        }
}

static float view_read(const TrView& v, uint32_t non, int64_t k, int64_t kEnd) {
    const int64_t off = tr_view_offset(v, non, k, kEnd);
    return off >= 0 ? v.p[off] : (off == -2 ? 1.0f : 0.0f);
}

// inj_xt_slab_kernel over every slab, then inj_slab_reduce_kernel
static void slab_product(const InjSlabArgs& g, uint32_t slabs, uint32_t in, uint32_t out, float* gw, float* gb, bool accumulate, bool scaleB) {
    for (uint32_t z = 0; z < slabs; ++z) {
        int64_t k0, k1;
        tr_slab_range(g.K, g.slabLen, z, k0, k1);
        if (k0 >= k1 || k1 > g.K) { printf("FAILED slab range %u\n", z); exit(1); }
        tiles<false, false>(g.M, g.N, k0, k1,
            [&](uint32_t non, int64_t k, int64_t kEnd) {
                int64_t off;
                const int src = inj_viewT_src(g.A, non, k, kEnd, off);
                return src == 0 ? g.A.h[off] : src == 1 ? g.A.c[off] : src == 2 ? g.A.m[off] : src == 3 ? 1.0f : 0.0f;
            },
            [&](uint32_t non, int64_t k, int64_t kEnd) { return view_read(g.B, non, k, kEnd); },
            [&](uint32_t row, uint32_t col, float v) { g.C[(uint64_t)z * g.slabStride + (uint64_t)row * g.N + col] = v; });
    }
    const uint32_t elems = (in + (scaleB ? 0u : 1u)) * out, threads = ((elems + 255) / 256) * 256;
    for (uint32_t i = 0; i < threads; ++i) {
        if (i >= elems) continue;
        float* dst = scaleB ? gw + i : tr_reduce_dst(i, in, out, gw, gb);
        float s = (accumulate && !scaleB) ? *dst : 0.0f;
        for (uint32_t z = 0; z < slabs; ++z) s += g.C[(uint64_t)z * g.slabStride + i];
        if (scaleB) {
            s = 6.2831855f * s;
            if (accumulate) s = *dst + s;
        }
        *dst = s;
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
        uint32_t hd[16], accumulate;
        uint64_t seed;
        float keep;
        if (!read_exact(f, hd, sizeof hd) || !read_exact(f, &seed, 8) || !read_exact(f, &keep, 4) || !read_exact(f, &accumulate, 4)) return 2;
        const uint32_t L = hd[0], F = hd[1], M = hd[2], *width = hd + 3, cl = hd[11], ml = hd[12];
        const int64_t n = hd[13];
        if (inj_check_shape(L, F, M, width, cl, ml) != 0) { printf("FAILED shape of case %u\n", ci); return 1; }
        const InjNet N = inj_net(L, F, M, width, cl, ml);
        const bool drop = hd[14] != 0 && keep != 1.0f;
        const uint32_t thr = drop ? inj_threshold(keep) : 0u, sample = hd[15];
        const float scale = 1.0f / keep;
        const uint32_t half = F / 2;
        Exact<float> B((size_t)half * 3), w(N.nw), b(N.nb), coords((size_t)n * 3), mods((size_t)n * M), dl((size_t)n * N.C);
        Exact<float> gB((size_t)half * 3), gw(N.nw), gb(N.nb), logits((size_t)n * N.C);
        if (!read_exact(f, B.p, B.n * 4) || !read_exact(f, w.p, w.n * 4) || !read_exact(f, b.p, b.n * 4) || !read_exact(f, coords.p, coords.n * 4) ||
            !read_exact(f, mods.p, mods.n * 4) || !read_exact(f, dl.p, dl.n * 4)) return 2;
        if (accumulate && (!read_exact(f, gB.p, gB.n * 4) || !read_exact(f, gw.p, gw.n * 4) || !read_exact(f, gb.p, gb.n * 4))) return 2;
        const InjTrainLayout T = inj_train_layout(N, n);
        Exact<char> scratch(T.bytes);
        char* base = scratch.p;
        const float* mp = M ? mods.p : nullptr;
        // every region is aligned, ordered and inside the buffer
        uint64_t prev = 0;
        const uint64_t offs[] = { T.offFeat, T.offDz, T.offDF, T.offC01, T.offSlab, T.bytes };
        for (uint64_t v : offs) {
            if ((v & 255u) != 0 || v < prev) { printf("FAILED layout of case %u\n", ci); return 1; }
            prev = v;
        }
        if (T.offSlab + (uint64_t)T.slabs * T.slabElems * 4 > T.bytes || T.offFeat != loss_scratch_bytes(n)) { printf("FAILED slab room of case %u\n", ci); return 1; }

        // ---- forward: the features, then the layers through the three-part view, each activation in its own region
        float* feat = (float*)(base + T.offFeat);
        for (int64_t p = 0; p < n; ++p)
            for (uint32_t j = 0; j < half; ++j) {
                const float ux = (coords.p[3 * p] + 1.0f) * 0.5f, uy = (coords.p[3 * p + 1] + 1.0f) * 0.5f, uz = (coords.p[3 * p + 2] + 1.0f) * 0.5f;
                const float q = ((ux * B.p[3 * j]) + (uy * B.p[3 * j + 1])) + (uz * B.p[3 * j + 2]);
                siren_sincos(6.2831855f * q, feat[p * F + j], feat[p * F + half + j]);
            }
        for (uint32_t l = 0; l < L; ++l) {
            const bool head = l + 1 == L;
            const float* h = l == 0 ? feat : (const float*)(base + T.offH[l - 1]);
            const InjView A = inj_layer_view(N, l, n, h, coords.p, mp, (int64_t)M, 1);
            float* C = head ? logits.p : (float*)(base + T.offH[l]);
            for (int64_t p = 0; p < n; ++p)
                for (uint32_t j = 0; j < N.out[l]; ++j) {
                    float acc = 0.0f;
                    for (int64_t k = 0; k < (int64_t)N.in[l]; ++k) {
                        int64_t off;
                        const int src = inj_view_src(A, (uint32_t)p, k, N.in[l], off);
                        const float x = src == 0 ? A.h.p[off] : src == 1 ? A.c.p[off] : src == 2 ? A.m.p[off] : 0.0f;
                        acc = chain(acc, x, w.p[N.wOff[l] + k * N.out[l] + j]);
                    }
                    float v = acc + b.p[N.bOff[l] + j];
                    if (!head) v = !(v <= 0.0f) ? v : 0.0f;
                    if (!head && drop) v = inj_mask_word(seed, (uint64_t)p, sample, l, j) < thr ? v * scale : 0.0f;
                    C[p * N.out[l] + j] = v;
                }
        }

        // ---- backward: the launches of mrirt_inject_backward
        float* slab = (float*)(base + T.offSlab);
        float* dF = (float*)(base + T.offDF);
        float* c01 = (float*)(base + T.offC01);
        const float* dz = dl.p;
        for (uint32_t l = L; l-- > 0;) {
            const float* hin = l == 0 ? feat : (const float*)(base + T.offH[l - 1]);
            slab_product(inj_slab_args(N, T, l, n, hin, coords.p, mp, dz, slab), T.slabs, N.in[l], N.out[l], gw.p + N.wOff[l], gb.p + N.bOff[l],
                         accumulate != 0, false);
            float* out = l == 0 ? dF : (float*)(base + inj_dz_offset(N, T, l));
            const InjDzArgs a = inj_dz_args(N, l, n, dz, w.p, l == 0 ? nullptr : hin, drop ? scale : 1.0f, out);
            tiles<true, true>(a.M, a.N, 0, a.K,
                [&](uint32_t non, int64_t k, int64_t kEnd) { return view_read(a.A, non, k, kEnd); },
                [&](uint32_t non, int64_t k, int64_t kEnd) { return view_read(a.B, non, k, kEnd); },
                [&](uint32_t row, uint32_t col, float v) {
                    const int64_t at = (int64_t)row * a.N + col;
                    if (l != 0 && drop) v = v * a.scale;
                    if (l != 0) v = a.act[at] > 0.0f ? v : 0.0f;
                    a.C[at] = v;
                });
            dz = out;
        }
        const int64_t gThreads = ((n * half + kInjThreads - 1) / kInjThreads) * kInjThreads;      // inj_g_kernel, every thread
        for (int64_t t = 0; t < gThreads; ++t) {
            if (t >= n * (int64_t)half) continue;
            const int64_t p = t / half;
            const uint32_t j = (uint32_t)(t - p * half);
            const float ux = (coords.p[3 * p] + 1.0f) * 0.5f, uy = (coords.p[3 * p + 1] + 1.0f) * 0.5f, uz = (coords.p[3 * p + 2] + 1.0f) * 0.5f;
            if (j == 0) { c01[3 * p] = ux; c01[3 * p + 1] = uy; c01[3 * p + 2] = uz; }
            const float q = ((ux * B.p[3 * j]) + (uy * B.p[3 * j + 1])) + (uz * B.p[3 * j + 2]);
            const float ang = 6.2831855f * q;
            const float g = (dF[p * F + j] * feat[p * F + half + j]) - (dF[p * F + half + j] * feat[p * F + j]);
            dF[p * F + j] = __builtin_fabsf(ang) <= 1048576.0f ? g : 0.0f;
        }
        slab_product(inj_slab_args_B(N, T, n, dF, c01, slab), T.slabs, half, 3, gB.p, nullptr, accumulate != 0, true);

        fwrite(logits.p, 4, logits.n, o);
        fwrite(gB.p, 4, gB.n, o);
        fwrite(gw.p, 4, gw.n, o);
        fwrite(gb.p, 4, gb.n, o);
        printf("case %u scratch %llu slabs %u\n", ci, (unsigned long long)T.bytes, T.slabs);
    }
    fclose(o);
    fclose(f);
    printf("inject_train_harness: %u cases done\n", count);
    return 0;
}
