// The index arithmetic of Muon's kernels (csrc/inr_muon.h: the layer table, the strided views of the three Newton-Schulz
// products, the element -> layer lookup, the scratch layout) on the CPU under AddressSanitizer + UBSan.  Every item replays
// mrirt_muon_orthogonalize launch by launch, block by block and thread by thread with the functions the kernels call, over
// heap buffers of EXACTLY the real sizes: an index past one is an ASan report.  The replayed result is compared with a plain
// triple loop over explicit (transposed where in > out) matrices, which must give the same bits: a wrong stride, a wrong
// transposition or a wrong layer offset is a wrong number.  Items:
//   n <in> <hidden> <layers> <out> <ns_steps>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_muon.h"

using namespace mrirt;

static const float kC[3] = { 3.4445f, -4.7750f, 2.0315f };

// one launch of muon_gemm_kernel for every layer: which = 0 gram, 1 poly, 2 update; returns the number of badly covered outputs
template <bool AKFAST, bool BKFAST>
static long long replay_product(const MuonPlan& P, int which, const float* X, float* A, float* B, float* Xn) {
    const uint32_t gx = muon_tiles(P.maxR, kTrBM), gy = muon_tiles(which == 2 ? P.maxC : P.maxR, kMuonBN);
    long long bad = 0;
    std::vector<float> As(kTrBK * TrLds<kTrBM>::pitch), Bs(kTrBK * TrLds<kMuonBN>::pitch), acc(kTrBM * kMuonBN);
    for (uint32_t z = 0; z < P.numLayers; ++z) {
        const MuonLayer& y = P.layer[z];
        const MuonGemm g = which == 0 ? muon_gram_args(y, X, A) : which == 1 ? muon_poly_args(y, A, B) : muon_update_args(y, B, X, Xn);
        std::vector<int> hits((size_t)g.M * g.N, 0);
        for (uint32_t bx = 0; bx < gx; ++bx)
            for (uint32_t by = 0; by < gy; ++by) {
                const uint32_t m0 = bx * kTrBM, n0 = by * kMuonBN;
                if (m0 >= g.M || n0 >= g.N) continue;
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int64_t k0 = 0; k0 < g.K; k0 += kTrBK) {
                    for (uint32_t t = 0; t < (uint32_t)kTrThreads; ++t) {
                        for (int i = 0; i < kTrBM / 16; ++i) {
                            uint32_t r, k;
                            tr_stage_coord<kTrBM, AKFAST>(t, i, r, k);
                            const int64_t off = tr_view_offset(g.A, m0 + r, k0 + k, g.K);
                            As[k * TrLds<kTrBM>::pitch + r] = off >= 0 ? g.A.p[off] : (off == -2 ? 1.0f : 0.0f);
                        }
                        for (int i = 0; i < kMuonBN / 16; ++i) {
                            uint32_t r, k;
                            tr_stage_coord<kMuonBN, BKFAST>(t, i, r, k);
                            const int64_t off = tr_view_offset(g.B, n0 + r, k0 + k, g.K);
                            Bs[k * TrLds<kMuonBN>::pitch + r] = off >= 0 ? g.B.p[off] : (off == -2 ? 1.0f : 0.0f);
                        }
                    }
                    for (int k = 0; k < kTrBK; ++k)
                        for (int r = 0; r < kTrBM; ++r)
                            for (int c = 0; c < kMuonBN; ++c)
                                acc[r * kMuonBN + c] = acc[r * kMuonBN + c] + As[k * TrLds<kTrBM>::pitch + r] * Bs[k * TrLds<kMuonBN>::pitch + c];
                }
                for (uint32_t wave = 0; wave < 4; ++wave)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < kMuonBN / 16; ++j)
                            for (int r = 0; r < 4; ++r) {
                                const uint32_t col = n0 + 16u * j + tr_acc_col(lane), row = m0 + 16u * wave + tr_acc_row(lane, r);
                                if (col >= g.N || row >= g.M) continue;
                                const int64_t at = (int64_t)row * g.cR + (int64_t)col * g.cC;
                                const float v = acc[(row - m0) * kMuonBN + (col - n0)];
                                g.C[at] = which == 0 ? v : which == 1 ? kC[1] * g.D[at] + kC[2] * v : kC[0] * g.D[at] + v;
                                ++hits[(size_t)row * g.N + col];
                            }
            }
        for (int h : hits) bad += h != 1;
    }
    return bad;
}

// NS of one layer on explicit matrices: X is r x c (the transpose of m when in > out), plain loops in increasing k
static void plain_ns(const float* m, uint32_t in, uint32_t out, double denom, uint32_t steps, float* res) {
    const bool t = in > out;
    const uint32_t r = t ? out : in, c = t ? in : out;
    std::vector<float> X((size_t)r * c), Xn((size_t)r * c), A((size_t)r * r), B((size_t)r * r);
    for (uint32_t i = 0; i < r; ++i)
        for (uint32_t j = 0; j < c; ++j) X[(size_t)i * c + j] = (float)((double)(t ? m[(size_t)j * out + i] : m[(size_t)i * out + j]) / denom);
    for (uint32_t s = 0; s < steps; ++s) {
        for (uint32_t i = 0; i < r; ++i)
            for (uint32_t j = 0; j < r; ++j) {
                float a = 0.0f;
                for (uint32_t k = 0; k < c; ++k) a = a + X[(size_t)i * c + k] * X[(size_t)j * c + k];
                A[(size_t)i * r + j] = a;
            }
        for (uint32_t i = 0; i < r; ++i)
            for (uint32_t j = 0; j < r; ++j) {
                float a = 0.0f;
                for (uint32_t k = 0; k < r; ++k) a = a + A[(size_t)i * r + k] * A[(size_t)k * r + j];
                B[(size_t)i * r + j] = kC[1] * A[(size_t)i * r + j] + kC[2] * a;
            }
        for (uint32_t i = 0; i < r; ++i)
            for (uint32_t j = 0; j < c; ++j) {
                float a = 0.0f;
                for (uint32_t k = 0; k < r; ++k) a = a + B[(size_t)i * r + k] * X[(size_t)k * c + j];
                Xn[(size_t)i * c + j] = kC[0] * X[(size_t)i * c + j] + a;
            }
        X.swap(Xn);
    }
    for (uint32_t i = 0; i < r; ++i)
        for (uint32_t j = 0; j < c; ++j) res[t ? (size_t)j * out + i : (size_t)i * out + j] = X[(size_t)i * c + j];
}

static int ns_item(uint32_t in, uint32_t hidden, uint32_t layers, uint32_t out, uint32_t steps) {
    const MuonPlan P = muon_plan(layers, in, hidden, out);
    const MuonLayout L = muon_layout(P);
    long long bad = 0;
    // the regions of the scratch follow one another without overlap and end at its size
    const uint64_t mat = P.nw * sizeof(float), gram = P.gramElems * sizeof(float);
    bad += L.offMhat < opt_scratch_bytes((int64_t)(P.nw + P.nb)) || L.offO < L.offMhat + mat || L.offNs < L.offO + mat || L.offDenom != L.offNs ||
           L.offX0 < L.offDenom + kTrMaxLayers * sizeof(double) || L.offX1 < L.offX0 + mat || L.offA < L.offX1 + mat || L.offB < L.offA + gram ||
           L.bytes < L.offB + gram || (L.bytes & 255u) != 0;
    uint64_t w = 0, g = 0;
    for (uint32_t l = 0; l < layers; ++l) {              // the table: consecutive matrices, r <= c, strides of the flat layout
        const MuonLayer& y = P.layer[l];
        bad += y.wOff != w || y.gOff != g || y.r > y.c || (uint64_t)y.r * y.c != (uint64_t)y.in * y.out;
        bad += (y.in > y.out) ? (y.sR != 1 || y.sC != (int64_t)y.out) : (y.sR != (int64_t)y.out || y.sC != 1);
        w += (uint64_t)y.in * y.out; g += (uint64_t)y.r * y.r;
    }
    bad += w != P.nw || g != P.gramElems;
    float* m = (float*)malloc(P.nw * sizeof(float));
    float* res = (float*)malloc(P.nw * sizeof(float));
    float* want = (float*)malloc(P.nw * sizeof(float));
    char* base = (char*)malloc(L.bytes);
    if (!m || !res || !want || !base) return 2;
    memset(base, 0xA5, L.bytes);
    uint32_t seed = 12345u + in * 7u + hidden + out * 131u;
    for (uint64_t i = 0; i < P.nw; ++i) { seed = seed * 1664525u + 1013904223u; m[i] = (float)((int)(seed >> 20) - 2048) / 512.0f; }
    // muon_norm_kernel: block l, thread t, elements t, t + kMuonThreads, ...
    double* denom = (double*)(base + L.offDenom);
    for (uint32_t l = 0; l < layers; ++l) {
        const MuonLayer& y = P.layer[l];
        double part[kMuonThreads];
        long long seen = 0;
        for (uint32_t t = 0; t < kMuonThreads; ++t) {
            double acc = 0.0;
            for (int64_t i = t; i < (int64_t)y.in * y.out; i += kMuonThreads) { acc += (double)m[y.wOff + i] * (double)m[y.wOff + i]; ++seen; }
            part[t] = acc;
        }
        bad += seen != (long long)y.in * y.out;
        double tot = 0.0;
        for (uint32_t wv = 0; wv < kMuonThreads / 64; ++wv) {
            double lanes[64];
            for (int k = 0; k < 64; ++k) lanes[k] = part[64 * wv + k];
            for (int o = 32; o > 0; o >>= 1)
                for (int k = 0; k < o; ++k) lanes[k] += lanes[k + o];
            tot += lanes[0];
        }
        denom[l] = sqrt(tot) + 1e-8;
    }
    // muon_scale_kernel: one thread per element, its layer from the lookup
    float* X[2] = { (float*)(base + L.offX0), (float*)(base + L.offX1) };
    const uint32_t blocks = (uint32_t)((P.nw + kMuonThreads - 1) / kMuonThreads);
    for (uint32_t bx = 0; bx < blocks; ++bx)
        for (uint32_t t = 0; t < kMuonThreads; ++t) {
            const int64_t i = (int64_t)bx * kMuonThreads + t;
            if (i >= (int64_t)P.nw) continue;
            const uint32_t l = muon_layer_of(P, i);
            bad += l >= layers || i < (int64_t)P.layer[l].wOff || i >= (int64_t)P.layer[l].wOff + (int64_t)P.layer[l].in * P.layer[l].out;
            X[0][i] = (float)((double)m[i] / denom[l]);
        }
    float* A = (float*)(base + L.offA);
    float* B = (float*)(base + L.offB);
    for (uint32_t k = 0; k < steps; ++k) {
        const float* cur = X[k & 1u];
        float* next = k + 1 == steps ? res : X[(k + 1) & 1u];
        bad += replay_product<true, true>(P, 0, cur, A, B, next);
        bad += replay_product<true, false>(P, 1, cur, A, B, next);
        bad += replay_product<true, false>(P, 2, cur, A, B, next);
    }
    for (uint32_t l = 0; l < layers; ++l) plain_ns(m + P.layer[l].wOff, P.layer[l].in, P.layer[l].out, denom[l], steps, want + P.layer[l].wOff);
    long long differ = 0;
    for (uint64_t i = 0; i < P.nw; ++i) differ += memcmp(&res[i], &want[i], sizeof(float)) != 0;
    printf("item n %u %u %u %u %u: scratch %llu B, nw %llu, layout / coverage errors %lld, elements differing from the plain loops %lld\n",
           in, hidden, layers, out, steps, (unsigned long long)L.bytes, (unsigned long long)P.nw, bad, differ);
    printf("item done %d\n", (bad || differ) ? 1 : 0);
    free(m); free(res); free(want); free(base);
    return (bad || differ) ? 1 : 0;
}

int main(int argc, char** argv) {
    int items = 0, failed = 0;
    for (int a = 1; a < argc;) {
        if (strcmp(argv[a], "n") || a + 5 >= argc) {
            fprintf(stderr, "usage: inr_muon_harness (n <in> <hidden> <layers> <out> <ns_steps>)...\n");
            return 2;
        }
        const int rc = ns_item((uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]), (uint32_t)atoi(argv[a + 4]),
                               (uint32_t)atoi(argv[a + 5]));
        a += 6;
        if (rc == 2) return 2;
        failed += rc;
        ++items;
    }
    printf("inr_muon_harness: %d items, %d failed\n", items, failed);
    return failed ? 1 : 0;
}
