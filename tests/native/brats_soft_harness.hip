// The per-sample chain of the soft prediction overlay (csrc/brats_soft.h, the code the kernels run per lane) on the CPU under
// AddressSanitizer + UBSan.  It replays every logits row of every case of tests/brats_soft_cases.py through soft_event, and
// every event the fp64 reference recorded through soft_grad (written out by tests/test_brats_soft_sanitizers.py), both with
// dword loads and, where C % 4 == 0, with the 16-byte loads.  Every row is read from, and every gradient row written to, a heap
// allocation of exactly C floats, so one element past a row is an ASan report.  It then feeds rows no network produces (NaN,
// infinities, one-hot +-1e4, all equal): no event or a finite one, never a trap.  Per case it prints the sums the test compares.
//
//   brats_soft_harness <case.bin>...   each: float64 [36] header (C, rows, events, D, lut[8][4]), then float64 [rows][C] logits
//                                      (fp32 values), then float64 [events][6] (row, T, G0, G1, G2, gR)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/brats_soft.h"

using namespace mrirt;

static std::vector<double> load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<double> v(n / sizeof(double));
    if (fread(v.data(), sizeof(double), v.size(), f) != v.size()) { fprintf(stderr, "short read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

static float* exact_row(uint32_t C) {                       // exactly C floats, 16-byte aligned (aligned_alloc wants a multiple)
    void* p = nullptr;
    if (posix_memalign(&p, 16, C * sizeof(float)) != 0) exit(2);
    return static_cast<float*>(p);
}

struct Sums { double events, alpha, c, dsum, dabs, ddot; };

template <bool VEC>
static Sums replay(const std::vector<double>& d, uint32_t C, size_t rows, size_t events, double D, const SoftRow* lut, int& failed) {
    Sums s = { 0, 0, 0, 0, 0, 0 };
    const double* logits = &d[36];
    const double* ev = &d[36 + rows * C];
    float* z = exact_row(C);
    float* dl = exact_row(C);
    for (size_t r = 0; r < rows; ++r) {
        for (uint32_t j = 0; j < C; ++j) z[j] = (float)logits[r * C + j];
        SoftEvent e;
        if (soft_event<VEC>(z, C, lut, D, e)) {
            s.events += 1.0; s.alpha += (double)e.alphaF; s.c += ((double)e.cF[0] + (double)e.cF[1]) + (double)e.cF[2];
            float C0 = 0.25f, C1 = 0.5f, C2 = 0.75f, T = 0.5f;
            soft_apply(e, C0, C1, C2, T);
            if (!(T >= 0.0f && T <= 0.5f)) { ++failed; printf("FAILED: T = %g after an event\n", T); }
        }
    }
    for (size_t i = 0; i < events; ++i) {
        const double* q = &ev[6 * i];
        const size_t r = (size_t)q[0];
        for (uint32_t j = 0; j < C; ++j) { z[j] = (float)logits[r * C + j]; dl[j] = NAN; }
        SoftEvent e;
        if (!soft_event<VEC>(z, C, lut, D, e)) { ++failed; printf("FAILED: row %zu draws no event\n", r); continue; }
        const double G[3] = { q[2], q[3], q[4] };
        soft_grad<VEC>(e, z, C, lut, D, q[1], G, q[5], dl);
        for (uint32_t j = 0; j < C; ++j) {
            const double key = (double)(((r * C + j) * 2654435761u) % 1021u);
            s.dsum += dl[j]; s.dabs += fabs((double)dl[j]); s.ddot += (double)dl[j] * key;
        }
        soft_zero_row<VEC>(dl, C);
        for (uint32_t j = 0; j < C; ++j) if (dl[j] != 0.0f || std::signbit(dl[j])) { ++failed; printf("FAILED: zero row\n"); }
    }
    // rows no network produces
    const float odd[8] = { NAN, INFINITY, -INFINITY, 1e4f, -1e4f, 0.0f, 3.4e38f, -3.4e38f };
    for (int a = 0; a < 8; ++a) for (int b = 0; b < 8; ++b) {
        for (uint32_t j = 0; j < C; ++j) { z[j] = (j & 1u) ? odd[a] : odd[b]; dl[j] = NAN; }
        SoftEvent e;
        if (soft_event<VEC>(z, C, lut, D, e)) {
            const double G[3] = { 1.0, -2.0, 0.5 };
            if (!(e.alphaF >= 0.0f && e.alphaF <= 1.0f) || !std::isfinite(e.cF[0] + e.cF[1] + e.cF[2])) { ++failed; printf("FAILED: odd row event\n"); }
            soft_grad<VEC>(e, z, C, lut, D, 0.75, G, 0.125, dl);
            for (uint32_t j = 0; j < C; ++j) if (!std::isfinite(dl[j])) { ++failed; printf("FAILED: odd row gradient %g\n", dl[j]); }
        }
    }
    free(z);
    free(dl);
    return s;
}

int main(int argc, char** argv) {
    int failed = 0;
    for (int ci = 1; ci < argc; ++ci) {
        const std::vector<double> d = load(argv[ci]);
        if (d.size() < 36) { fprintf(stderr, "%s: no header\n", argv[ci]); return 2; }
        const uint32_t C = (uint32_t)d[0];
        const size_t rows = (size_t)d[1], events = (size_t)d[2];
        const double D = d[3];
        if (C < 1 || C > kSoftMaxClasses || d.size() != 36 + rows * C + 6 * events) { fprintf(stderr, "%s: size does not match its header\n", argv[ci]); return 2; }
        float lutf[8][4];
        for (int k = 0; k < 8; ++k) for (int j = 0; j < 4; ++j) lutf[k][j] = (float)d[4 + 4 * k + j];
        if (!soft_lut_ok(lutf)) { ++failed; printf("FAILED: the case's LUT is refused\n"); }
        SoftRow* lut = (SoftRow*)malloc(kSoftDrawn * sizeof(SoftRow));             // exactly the eight rows
        if (!lut) return 2;
        for (uint32_t k = 0; k < kSoftDrawn; ++k) lut[k] = soft_row(lutf[k]);
        const Sums a = replay<false>(d, C, rows, events, D, lut, failed);
        printf("case %d classes %u rows %zu events %.0f alpha %.17g c %.17g dl %.17g %.17g %.17g\n", ci - 1, C, rows, a.events, a.alpha, a.c,
               a.dsum, a.dabs, a.ddot);
        if (C % 4 == 0) {
            const Sums b = replay<true>(d, C, rows, events, D, lut, failed);
            if (memcmp(&a, &b, sizeof(Sums)) != 0) { ++failed; printf("FAILED: the 16-byte row path gives other bits\n"); }
        }
        free(lut);
    }
    // the LUT check itself
    {
        float lut[8][4];
        memset(lut, 0, sizeof(lut));
        if (!soft_lut_ok(lut)) { ++failed; printf("FAILED: a zero LUT is refused\n"); }
        lut[0][3] = -1.0f;
        if (!soft_lut_ok(lut)) { ++failed; printf("FAILED: row 0 draws nothing and must not be checked\n"); }
        const float bad[4] = { -1.0f, NAN, INFINITY, -INFINITY };
        for (int k = 1; k < 8; ++k) for (int b = 0; b < 4; ++b) {
            lut[k][3] = bad[b];
            if (soft_lut_ok(lut)) { ++failed; printf("FAILED: lut[%d].w = %g accepted\n", k, bad[b]); }
            lut[k][3] = 1.0f;
        }
    }
    printf("brats_soft_harness: %d cases, %d failed\n", argc - 1, failed);
    return failed == 0 ? 0 : 1;
}
