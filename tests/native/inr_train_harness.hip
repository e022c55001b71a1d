// The index arithmetic of the INR training kernels (csrc/inr_train.h: staging coordinates, operand views, LDS images, the
// MFMA accumulator map, slab ranges, the scratch layout) on the CPU under AddressSanitizer + UBSan.  For every shape given it
// replays the launches of one training step block by block and thread by thread, with the same functions the kernels call
// and the same launch arguments the library's host code builds (tr_forward_args, tr_slab_args, tr_mask_args, the offsets),
// over heap buffers of EXACTLY the sizes the library asks for (inputs, weights, logits, the scratch of
// train_layout, gradients): an index past one is an ASan report.  With integer data it also computes what the kernels compute
// (the MFMA as its definition over the operand lane map) and compares logits, dW and db with a plain triple loop, so a
// misplaced element is a wrong integer.  Large shapes walk the addresses only (compute = 0).
//
//   inr_train_harness <in> <hidden> <layers> <out> <n> <compute> ...      (six numbers per shape)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_train.h"

using namespace mrirt;

static volatile float g_sink;

template <int R, bool KFAST>
static void stage(const TrView& v, uint32_t non0, int64_t k0, int64_t kEnd, float* lds) {
    for (uint32_t t = 0; t < (uint32_t)kTrThreads; ++t)
        for (int i = 0; i < R / 16; ++i) {
            uint32_t r, k;
            tr_stage_coord<R, KFAST>(t, i, r, k);
            const int64_t off = tr_view_offset(v, non0 + r, k0 + k, kEnd);
            lds[k * TrLds<R>::pitch + r] = off >= 0 ? v.p[off] : (off == -2 ? 1.0f : 0.0f);
        }
}

template <int BN, bool AKFAST, bool BKFAST>
static void run_blocks(const TrGemmArgs& g, uint32_t slabs, int epi, bool compute) {       // epi: 0 bias, 1 mask, 2 slab
    const uint32_t mt = (g.M + kTrBM - 1) / kTrBM, nt = (g.N + BN - 1) / BN;
    std::vector<float> As(kTrBK * TrLds<kTrBM>::pitch), Bs(kTrBK * TrLds<BN>::pitch);    // exactly the kernel's LDS arrays
    std::vector<float> acc((size_t)kTrBM * BN);
    for (uint32_t z = 0; z < slabs; ++z)
        for (uint32_t bx = 0; bx < mt; ++bx)
            for (uint32_t by = 0; by < nt; ++by) {
                const uint32_t m0 = bx * kTrBM, n0 = by * BN;
                int64_t kb = 0, ke = g.K;
                if (epi == 2) tr_slab_range(g.K, g.slabLen, z, kb, ke);
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int64_t k0 = kb; k0 < ke; k0 += kTrBK) {
                    stage<kTrBM, AKFAST>(g.A, m0, k0, ke, As.data());
                    stage<BN, BKFAST>(g.B, n0, k0, ke, Bs.data());
                    for (uint32_t wave = 0; wave < 4; ++wave)
                        for (int s = 0; s < kTrBK / 4; ++s) {
                            float av[64], bv[BN / 16][64];
                            for (uint32_t lane = 0; lane < 64; ++lane) {
                                const uint32_t kk = 4u * s + (lane >> 4);
                                av[lane] = As[kk * TrLds<kTrBM>::pitch + 16u * wave + (lane & 15u)];
                                for (int j = 0; j < BN / 16; ++j) bv[j][lane] = Bs[kk * TrLds<BN>::pitch + 16u * j + (lane & 15u)];
                            }
                            if (!compute) { g_sink = av[63] + bv[BN / 16 - 1][63]; continue; }
                            for (int j = 0; j < BN / 16; ++j)             // D[i][c] += sum_k A[i][k] B[k][c]; lane 16 k + i holds A[i][k], B[k][i]
                                for (uint32_t i = 0; i < 16; ++i)
                                    for (uint32_t c = 0; c < 16; ++c)
                                        for (uint32_t k = 0; k < 4; ++k)
                                            acc[(size_t)(16 * wave + i) * BN + 16 * j + c] += av[16 * k + i] * bv[j][16 * k + c];
                        }
                }
                for (uint32_t wave = 0; wave < 4; ++wave)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < BN / 16; ++j)
                            for (int r = 0; r < 4; ++r) {
                                const uint32_t lr = 16u * wave + tr_acc_row(lane, r), lc = 16u * j + tr_acc_col(lane);
                                const uint32_t row = m0 + lr, col = n0 + lc;
                                if (row >= g.M || col >= g.N) continue;
                                float v = acc[(size_t)lr * BN + lc];
                                if (epi == 0) {
                                    v += g.bias[col];
                                    if (g.relu) v = v > 0.0f ? v : 0.0f;
                                    g.C[(int64_t)row * g.ldc + col] = v;
                                } else if (epi == 1) {
                                    const int64_t at = (int64_t)row * g.ldc + col;
                                    g.C[at] = g.mask[at] > 0.0f ? v : 0.0f;
                                } else {
                                    g.C[(uint64_t)z * g.slabStride + (uint64_t)row * g.N + col] = v;
                                }
                            }
            }
}

template <bool AKFAST, bool BKFAST>
static void run(const TrGemmArgs& g, uint32_t slabs, int epi, bool compute) {               // launch_gemm's choice of tile
    if (g.N <= 16) run_blocks<16, AKFAST, BKFAST>(g, slabs, epi, compute);
    else run_blocks<64, AKFAST, BKFAST>(g, slabs, epi, compute);
}

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int one_shape(uint32_t ind, uint32_t hid, uint32_t layers, uint32_t out, int64_t n, bool compute) {
    const TrainLayout L = train_layout(layers, ind, hid, out, n);
    const size_t nw = L.wOff[layers - 1] + (size_t)L.in[layers - 1] * L.out[layers - 1], nb = L.bOff[layers - 1] + L.out[layers - 1];
    // every buffer exactly its size (malloc: ASan guards both ends)
    float* w = (float*)malloc(nw * sizeof(float));
    float* b = (float*)malloc(nb * sizeof(float));
    float* gw = (float*)malloc(nw * sizeof(float));
    float* gb = (float*)malloc(nb * sizeof(float));
    float* feats = (float*)malloc((size_t)n * ind * sizeof(float));
    float* logits = (float*)malloc((size_t)n * out * sizeof(float));
    float* dlogits = (float*)malloc((size_t)n * out * sizeof(float));
    char* scratch = (char*)malloc(L.bytes);
    if (!w || !b || !gw || !gb || !feats || !logits || !dlogits || !scratch) return 2;
    uint32_t seed = ind * 7919u + hid * 31u + layers * 3u + out + (uint32_t)n;
    for (size_t i = 0; i < nw; ++i) { const uint32_t r = rnd(seed) % 16; w[i] = r == 0 ? 1.0f : r == 1 ? -1.0f : 0.0f; }
    for (size_t i = 0; i < nb; ++i) b[i] = (float)((int)(rnd(seed) % 3) - 1);
    for (size_t i = 0; i < (size_t)n * ind; ++i) feats[i] = (float)((int)(rnd(seed) % 5) - 2);
    for (size_t i = 0; i < (size_t)n * out; ++i) dlogits[i] = (float)((int)(rnd(seed) % 5) - 2);
    // the launches of mrirt_inr_forward_f32 and mrirt_inr_backward, from the argument builders the library itself calls
    float* x = (float*)(scratch + L.offX);
    memcpy(x, feats, (size_t)n * ind * sizeof(float));                    // the raw kind's feature kernel
    const float* h = x;
    for (uint32_t l = 0; l < layers; ++l) {
        float* o = l + 1 == layers ? logits : (float*)(scratch + tr_in_offset(L, l + 1, n));
        run<true, false>(tr_forward_args(L, l, n, h, w, b, o), 1, 0, compute);
        h = o;
    }
    float* slab = (float*)(scratch + L.offSlab);
    const float* dz = dlogits;
    for (uint32_t l = layers; l-- > 0;) {
        const float* hin = (const float*)(scratch + tr_in_offset(L, l, n));
        run<false, false>(tr_slab_args(L, l, n, hin, dz, slab), L.slabs, 2, compute);
        for (uint32_t i = 0; i < (L.in[l] + 1) * L.out[l]; ++i) {         // tr_slab_reduce_kernel
            float* dst = tr_reduce_dst(i, L.in[l], L.out[l], gw + L.wOff[l], gb + L.bOff[l]);
            float s = 0.0f;
            for (uint32_t z = 0; z < L.slabs; ++z) s += slab[(uint64_t)z * L.slabElems + i];
            *dst = s;
        }
        if (l == 0) break;
        float* dzPrev = (float*)(scratch + tr_dz_offset(L, l, n));
        run<true, true>(tr_mask_args(L, l, n, dz, w, hin, dzPrev), 1, 1, compute);
        dz = dzPrev;
    }
    long long bad = 0;
    if (compute) {                                       // the plain definition, in double (every value is a small integer)
        std::vector<double> hh(feats, feats + (size_t)n * ind), zz;
        std::vector<std::vector<double>> hs;
        for (uint32_t l = 0; l < layers; ++l) {
            hs.push_back(hh);
            zz.assign((size_t)n * L.out[l], 0.0);
            for (int64_t p = 0; p < n; ++p)
                for (uint32_t j = 0; j < L.out[l]; ++j) {
                    double s = b[L.bOff[l] + j];
                    for (uint32_t i = 0; i < L.in[l]; ++i) s += hh[p * L.in[l] + i] * w[L.wOff[l] + (size_t)i * L.out[l] + j];
                    zz[p * L.out[l] + j] = (l + 1 < layers && s < 0.0) ? 0.0 : s;
                }
            hh = zz;
        }
        for (size_t i = 0; i < (size_t)n * out; ++i) bad += logits[i] != (float)hh[i];
        std::vector<double> d(dlogits, dlogits + (size_t)n * out), dp;
        for (uint32_t l = layers; l-- > 0;) {
            for (uint32_t i = 0; i < L.in[l]; ++i)
                for (uint32_t j = 0; j < L.out[l]; ++j) {
                    double s = 0.0;
                    for (int64_t p = 0; p < n; ++p) s += hs[l][p * L.in[l] + i] * d[p * L.out[l] + j];
                    bad += gw[L.wOff[l] + (size_t)i * L.out[l] + j] != (float)s;
                }
            for (uint32_t j = 0; j < L.out[l]; ++j) {
                double s = 0.0;
                for (int64_t p = 0; p < n; ++p) s += d[p * L.out[l] + j];
                bad += gb[L.bOff[l] + j] != (float)s;
            }
            if (l == 0) break;
            dp.assign((size_t)n * L.in[l], 0.0);
            for (int64_t p = 0; p < n; ++p)
                for (uint32_t i = 0; i < L.in[l]; ++i) {
                    double s = 0.0;
                    for (uint32_t j = 0; j < L.out[l]; ++j) s += d[p * L.out[l] + j] * w[L.wOff[l] + (size_t)i * L.out[l] + j];
                    dp[p * L.in[l] + i] = hs[l][p * L.in[l] + i] > 0.0 ? s : 0.0;
                }
            d = dp;
        }
    }
    printf("shape %u %u %u %u %lld compute %d scratch %llu slabs %u x %u mismatches %lld\n", ind, hid, layers, out, (long long)n, (int)compute,
           (unsigned long long)L.bytes, L.slabs, L.slabLen, bad);
    free(w); free(b); free(gw); free(gb); free(feats); free(logits); free(dlogits); free(scratch);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 1) % 6 != 0) { fprintf(stderr, "usage: inr_train_harness (<in> <hidden> <layers> <out> <n> <compute>)...\n"); return 2; }
    int shapes = 0, failed = 0;
    for (int a = 1; a + 5 < argc; a += 6) {
        const int rc = one_shape((uint32_t)atoi(argv[a]), (uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]),
                                 atoll(argv[a + 4]), atoi(argv[a + 5]) != 0);
        if (rc == 2) return 2;
        failed += rc;
        ++shapes;
    }
    // the loss kernels' scratch: block b's sums and the totals stay inside loss_scratch_bytes(n) for every block count
    for (int64_t n : { (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)65536, (int64_t)65537, (int64_t)1 << 30 }) {
        const uint32_t blocks = loss_blocks(n);
        double* sums = (double*)malloc(loss_scratch_bytes(n));
        if (!sums) return 2;
        for (uint32_t bl = 0; bl <= blocks; ++bl)
            for (uint32_t v = 0; v < kLossVals; ++v) sums[(uint64_t)bl * kLossVals + v] = 1.0;
        free(sums);
    }
    printf("inr_train_harness: %d shapes, %d failed\n", shapes, failed);
    return failed ? 1 : 0;
}
