// The SIREN training step's index arithmetic and its sine on the CPU under AddressSanitizer + UBSan.
// For every shape given it replays the launches of mrirt_siren_forward_f32 and mrirt_siren_backward block by block and
// thread by thread, with the functions the kernels call and the launch arguments the library's host code builds
// (siren_layout, tr_siren_feature_src, tr_sine_args, tr_forward_args, tr_slab_args, tr_cos_args, the offsets), over heap
// buffers of EXACTLY the sizes the library asks for: an index past one is an ASan report.  With compute = 1 the nets are
// selection nets (one non-zero term per dot product), and logits, dW and db are compared bit for bit with the plain
// definition evaluated with the same siren_sincos.  Then siren_sincos runs over the edges of its domain and beyond
// (2^20 and its neighbours, the largest floats, infinities, NaN, zeros, denormals): any undefined conversion is a UBSan report.
//
//   inr_siren_harness <in> <hidden> <layers> <out> <n> <raw> <compute> ...      (seven numbers per shape)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/inr_train.h"
#include "../../mri-raytracer_amd/csrc/siren_sincos.h"

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

enum { kBias = 0, kSlab = 2, kSine = 3, kCos = 4 };

template <int BN, bool AKFAST, bool BKFAST>
static void run_blocks(const TrGemmArgs& g, uint32_t slabs, int epi, bool compute) {
    const uint32_t mt = (g.M + kTrBM - 1) / kTrBM, nt = (g.N + BN - 1) / BN;
    std::vector<float> As(kTrBK * TrLds<kTrBM>::pitch), Bs(kTrBK * TrLds<BN>::pitch);
    std::vector<float> acc((size_t)kTrBM * BN);
    for (uint32_t z = 0; z < slabs; ++z)
        for (uint32_t bx = 0; bx < mt; ++bx)
            for (uint32_t by = 0; by < nt; ++by) {
                const uint32_t m0 = bx * kTrBM, n0 = by * BN;
                int64_t kb = 0, ke = g.K;
                if (epi == kSlab) tr_slab_range(g.K, g.slabLen, z, kb, ke);
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
                            for (int j = 0; j < BN / 16; ++j)
                                for (uint32_t i = 0; i < 16; ++i)
                                    for (uint32_t c = 0; c < 16; ++c)
                                        for (uint32_t k = 0; k < 4; ++k)                    // the k-ordered chain, unfused is the same here:
                                            acc[(size_t)(16 * wave + i) * BN + 16 * j + c] += av[16 * k + i] * bv[j][16 * k + c];      // one non-zero term
                        }
                }
                for (uint32_t wave = 0; wave < 4; ++wave)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < BN / 16; ++j)
                            for (int r = 0; r < 4; ++r) {
                                const uint32_t lr = 16u * wave + tr_acc_row(lane, r), lc = 16u * j + tr_acc_col(lane);
                                const uint32_t row = m0 + lr, col = n0 + lc;
                                if (row >= g.M || col >= g.N) continue;
                                const float v = acc[(size_t)lr * BN + lc];
                                const int64_t at = (int64_t)row * g.ldc + col;
                                if (epi == kBias) g.C[at] = v + g.bias[col];
                                else if (epi == kSine) {
                                    float sn, cs;
                                    siren_sincos(v + g.bias[col], sn, cs);
                                    g.C[at] = sn;
                                    g.cosOut[at] = cs;
                                } else if (epi == kCos) g.C[at] = v * g.mask[at];
                                else g.C[(uint64_t)z * g.slabStride + (uint64_t)row * g.N + col] = v;
                            }
            }
}

template <bool AKFAST, bool BKFAST>
static void run(const TrGemmArgs& g, uint32_t slabs, int epi, bool compute) {               // launch_gemm's choice of tile
    if (g.N <= 16) run_blocks<16, AKFAST, BKFAST>(g, slabs, epi, compute);
    else run_blocks<64, AKFAST, BKFAST>(g, slabs, epi, compute);
}

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)(rnd(s) % 4001) / 1000.0f - 2.0f; }          // -2 .. 2

static int one_shape(uint32_t ind, uint32_t hid, uint32_t layers, uint32_t out, int64_t n, bool raw, bool compute) {
    const SirenLayout S = siren_layout(layers, ind, hid, out, n);
    const TrainLayout& L = S.T;
    const uint32_t M = raw ? 0u : ind - 3u;
    const float w0 = 30.0f;
    const size_t nw = L.wOff[layers - 1] + (size_t)L.in[layers - 1] * L.out[layers - 1], nb = L.bOff[layers - 1] + L.out[layers - 1];
    float* w = (float*)calloc(nw, sizeof(float));
    float* b = (float*)malloc(nb * sizeof(float));
    float* gw = (float*)malloc(nw * sizeof(float));
    float* gb = (float*)malloc(nb * sizeof(float));
    float* coords = raw ? nullptr : (float*)malloc((size_t)n * 3 * sizeof(float));
    float* feats = (raw || M) ? (float*)malloc((size_t)n * (raw ? ind : M) * sizeof(float)) : nullptr;
    float* logits = (float*)malloc((size_t)n * out * sizeof(float));
    float* dlogits = (float*)calloc((size_t)n * out, sizeof(float));
    char* scratch = (char*)malloc(S.bytes);                              // exactly mrirt_siren_train_scratch_bytes
    if (!w || !b || !gw || !gb || !logits || !dlogits || !scratch || (!raw && !coords) || ((raw || M) && !feats)) return 2;
    uint32_t seed = ind * 7919u + hid * 31u + layers * 3u + out + (uint32_t)n;
    for (uint32_t l = 0; l < layers; ++l)                                // a selection net: column j of layer l has one 1
        for (uint32_t j = 0; j < L.out[l]; ++j) {
            const uint32_t i = l == 0 ? j % L.in[l] : l + 1 < layers ? (j * 5u + 3u * l) % L.in[l] : (7u * l + j) % L.in[l];      // 5 is a unit mod 2^k
            w[L.wOff[l] + (size_t)i * L.out[l] + j] = 1.0f;
        }
    for (size_t i = 0; i < nb; ++i) b[i] = unit(seed);
    if (coords) for (size_t i = 0; i < (size_t)n * 3; ++i) coords[i] = unit(seed);
    if (feats) for (size_t i = 0; i < (size_t)n * (raw ? ind : M); ++i) feats[i] = unit(seed);
    const int64_t pstar = n - 1;
    for (uint32_t j = 0; j < out; ++j) dlogits[pstar * out + j] = unit(seed) + 3.0f;
    // mrirt_siren_forward_f32
    float* x = (float*)(scratch + L.offX);
    for (int64_t i = 0; i < n * (int64_t)ind; ++i) {                    // tr_siren_features_kernel
        uint32_t src;
        int64_t off;
        tr_siren_feature_src(i, ind, M, raw ? 1u : 0u, src, off);
        x[i] = w0 * (src ? feats[off] : coords[off]);
    }
    const float* h = x;
    for (uint32_t l = 0; l < layers; ++l) {
        const bool head = l + 1 == layers;
        float* o = head ? logits : (float*)(scratch + tr_in_offset(L, l + 1, n));
        if (head) run<true, false>(tr_forward_args(L, l, n, h, w, b, o), 1, kBias, compute);
        else run<true, false>(tr_sine_args(S, l, n, h, w, b, o, (float*)(scratch + tr_cos_offset(S, l, n))), 1, kSine, compute);
        h = o;
    }
    // mrirt_siren_backward
    float* slab = (float*)(scratch + L.offSlab);
    const float* dz = dlogits;
    for (uint32_t l = layers; l-- > 0;) {
        const float* hin = (const float*)(scratch + tr_in_offset(L, l, n));
        run<false, false>(tr_slab_args(L, l, n, hin, dz, slab), L.slabs, kSlab, compute);
        for (uint32_t i = 0; i < (L.in[l] + 1) * L.out[l]; ++i) {         // tr_slab_reduce_kernel
            float* dst = tr_reduce_dst(i, L.in[l], L.out[l], gw + L.wOff[l], gb + L.bOff[l]);
            float s = 0.0f;
            for (uint32_t z = 0; z < L.slabs; ++z) s += slab[(uint64_t)z * L.slabElems + i];
            *dst = s;
        }
        if (l == 0) break;
        float* dzPrev = (float*)(scratch + tr_dz_offset(L, l, n));
        run<true, true>(tr_cos_args(S, l, n, dz, w, (const float*)(scratch + tr_cos_offset(S, l - 1, n)), dzPrev), 1, kCos, compute);
        dz = dzPrev;
    }
    long long bad = 0;
    if (compute) {                                       // the plain definition in fp32; every dot product has one non-zero term
        std::vector<float> hh(x, x + (size_t)n * ind), zz, cc;
        std::vector<std::vector<float>> hs, cosines;
        for (uint32_t l = 0; l < layers; ++l) {
            hs.push_back(hh);
            zz.assign((size_t)n * L.out[l], 0.0f);
            cc.assign((size_t)n * L.out[l], 0.0f);
            for (int64_t p = 0; p < n; ++p)
                for (uint32_t j = 0; j < L.out[l]; ++j) {
                    float s = 0.0f;
                    for (uint32_t i = 0; i < L.in[l]; ++i) s += hh[p * L.in[l] + i] * w[L.wOff[l] + (size_t)i * L.out[l] + j];
                    s = s + b[L.bOff[l] + j];
                    if (l + 1 < layers) siren_sincos(s, zz[p * L.out[l] + j], cc[p * L.out[l] + j]);
                    else zz[p * L.out[l] + j] = s;
                }
            hh = zz;
            cosines.push_back(cc);
        }
        for (size_t i = 0; i < (size_t)n * out; ++i) bad += !(logits[i] == hh[i]);
        std::vector<float> d(dlogits, dlogits + (size_t)n * out), dp;
        for (uint32_t l = layers; l-- > 0;) {
            for (uint32_t i = 0; i < L.in[l]; ++i)
                for (uint32_t j = 0; j < L.out[l]; ++j) {
                    float s = 0.0f;
                    for (int64_t p = 0; p < n; ++p) s += hs[l][p * L.in[l] + i] * d[p * L.out[l] + j];
                    bad += !(gw[L.wOff[l] + (size_t)i * L.out[l] + j] == s);
                }
            for (uint32_t j = 0; j < L.out[l]; ++j) {
                float s = 0.0f;
                for (int64_t p = 0; p < n; ++p) s += d[p * L.out[l] + j];
                bad += !(gb[L.bOff[l] + j] == s);
            }
            if (l == 0) break;
            dp.assign((size_t)n * L.in[l], 0.0f);
            for (int64_t p = 0; p < n; ++p)
                for (uint32_t i = 0; i < L.in[l]; ++i) {
                    float s = 0.0f;
                    for (uint32_t j = 0; j < L.out[l]; ++j) s += d[p * L.out[l] + j] * w[L.wOff[l] + (size_t)i * L.out[l] + j];
                    dp[p * L.in[l] + i] = s * cosines[l - 1][p * L.in[l] + i];
                }
            d = dp;
        }
    }
    printf("shape %u %u %u %u %lld raw %d compute %d scratch %llu (cosines at %llu) slabs %u x %u mismatches %lld\n", ind, hid, layers, out,
           (long long)n, (int)raw, (int)compute, (unsigned long long)S.bytes, (unsigned long long)S.offC, L.slabs, L.slabLen, bad);
    free(w); free(b); free(gw); free(gb); free(coords); free(feats); free(logits); free(dlogits); free(scratch);
    return bad ? 1 : 0;
}

// siren_sincos over the edges of its domain: results in [-1, 1] or NaN as stated, and no undefined operation on the way
static int sincos_edges() {
    const float edge = 1048576.0f;
    const float args[] = { 0.0f, -0.0f, 1e-45f, -1e-45f, 1.17549435e-38f, 1.0f, -1.0f, 0.78539819f, 1.5707964f, -1.5707964f, 3.1415927f, 6.2831855f,
                           edge, -edge, nextafterf(edge, 0.0f), nextafterf(edge, INFINITY), -nextafterf(edge, INFINITY), 2097152.0f, 2147483648.0f,
                           -2147483648.0f, 4294967296.0f, 9.223372e18f, -9.223372e18f, 1.8446744e19f, 3.4028235e38f, -3.4028235e38f, INFINITY, -INFINITY,
                           NAN, -NAN };
    int bad = 0;
    for (float a : args) {
        float s, c;
        siren_sincos(a, s, c);
        const bool inside = fabsf(a) <= edge;
        if (a != a || fabsf(a) == INFINITY) bad += !(s != s && c != c);
        else if (inside) bad += !(fabsf(s - (float)sin((double)a)) <= 1.2e-7f && fabsf(c - (float)cos((double)a)) <= 1.2e-7f && fabsf(s) <= 1.0f && fabsf(c) <= 1.0f);
        else bad += !(s == 0.0f && c == 1.0f);
    }
    for (int k = -70000; k <= 70000; ++k) {              // every quadrant transition of the domain's inner part, and far multiples
        for (float a : { (float)(k * 1.5707963267948966), (float)(k * 15.0 * 1.5707963267948966) }) {
            if (fabsf(a) > edge) continue;
            for (float v : { a, nextafterf(a, INFINITY), nextafterf(a, -INFINITY) }) {
                float s, c;
                siren_sincos(v, s, c);
                bad += !(s == (float)sin((double)v) && c == (float)cos((double)v));
            }
        }
    }
    printf("sincos edges: %d bad\n", bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 8 || (argc - 1) % 7 != 0) { fprintf(stderr, "usage: inr_siren_harness (<in> <hidden> <layers> <out> <n> <raw> <compute>)...\n"); return 2; }
    int shapes = 0, failed = 0;
    for (int a = 1; a + 6 < argc; a += 7) {
        const int rc = one_shape((uint32_t)atoi(argv[a]), (uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2]), (uint32_t)atoi(argv[a + 3]),
                                 atoll(argv[a + 4]), atoi(argv[a + 5]) != 0, atoi(argv[a + 6]) != 0);
        if (rc == 2) return 2;
        failed += rc;
        ++shapes;
    }
    const int edges = sincos_edges();
    printf("inr_siren_harness: %d shapes, %d failed, %d sincos edges bad\n", shapes, failed, edges);
    return (failed || edges) ? 1 : 0;
}
