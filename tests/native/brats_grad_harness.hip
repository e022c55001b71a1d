// The per-sample math of the K1 backward pass (csrc/brats_grad.h, the code the kernel runs per lane) on the CPU under
// AddressSanitizer + UBSan.  It replays every sample of every case of tests/brats_grad_cases.py (written out by
// tests/test_brats_grad_sanitizers.py from the fp64 reference's records) through grad_sample / grad_modality / grad_corners and
// scatters into gradient buffers that are heap allocations of exactly X*Y*Z elements, so an index past one is an ASan report.
// It then feeds grad_corners cells that the forward's clamp can never produce (the last voxel, one past it, 2^32 - 1): the
// indices must stay inside the grid.  Per case it prints the sums the test compares with the reference.
//
//   brats_grad_harness <case.bin>...     each: float64 [18] header (X, Y, Z, n, enabled[4], weight[4], ww, wl, intensityAlpha,
//                                        gamma, stepSize, wsum), then float64 [n][10] (ix, iy, iz, fx, fy, fz, v, T, g1, gR)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mri-raytracer_amd/csrc/brats_grad.h"

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

int main(int argc, char** argv) {
    int failed = 0;
    for (int ci = 1; ci < argc; ++ci) {
        const std::vector<double> d = load(argv[ci]);
        if (d.size() < 18) { fprintf(stderr, "%s: no header\n", argv[ci]); return 2; }
        const uint32_t X = (uint32_t)d[0], Y = (uint32_t)d[1], Z = (uint32_t)d[2];
        const size_t n = (size_t)d[3], nvox = (size_t)X * Y * Z;
        if (d.size() != 18 + 10 * n) { fprintf(stderr, "%s: size does not match its header\n", argv[ci]); return 2; }
        uint32_t enabled[4];
        float weight[4];
        for (int m = 0; m < 4; ++m) { enabled[m] = (uint32_t)d[4 + m]; weight[m] = (float)d[8 + m]; }
        GradTf tf;
        tf.ww = (float)d[12]; tf.wl = (float)d[13]; tf.intensityAlpha = (float)d[14]; tf.gamma = (float)d[15];
        tf.stepSize = (float)d[16]; tf.wsum = (float)d[17];
        double* gv[4] = { nullptr, nullptr, nullptr, nullptr };
        for (int m = 0; m < 4; ++m)
            if (enabled[m]) { gv[m] = (double*)calloc(nvox, sizeof(double)); if (!gv[m]) return 2; }   // exactly the grid
        double tfsum[4] = { 0.0, 0.0, 0.0, 0.0 };
        size_t events = 0;
        for (size_t i = 0; i < n; ++i) {
            const double* s = &d[18 + 10 * i];
            GradSample gs;
            if (!grad_sample(tf, (float)s[6], (float)s[7], s[8], s[9], gs)) continue;
            ++events;
            tfsum[0] += gs.dww; tfsum[1] += gs.dwl; tfsum[2] += gs.da; tfsum[3] += gs.dgamma;
            if (gs.dv == 0.0) continue;
            GradCorners c;
            grad_corners((uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[2], (float)s[3], (float)s[4], (float)s[5], X, Y, Z, c);
            for (int m = 0; m < 4; ++m) {
                if (!enabled[m]) continue;
                const double ds = grad_modality(tf, gs.dv, weight[m]);
                for (int k = 0; k < 8; ++k) gv[m][c.idx[k]] += ds * (double)c.w[k];
            }
        }
        // cells the forward never produces: the clamps alone must keep every index inside the grid
        {
            float* probe = (float*)calloc(nvox, sizeof(float));
            if (!probe) return 2;
            const uint32_t odd[5] = { 0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu };
            for (uint32_t ax = 0; ax < 5; ++ax) for (uint32_t ay = 0; ay < 5; ++ay) for (uint32_t az = 0; az < 5; ++az) {
                const uint32_t ix = odd[ax] < 2 ? X - 1u + odd[ax] : odd[ax], iy = odd[ay] < 2 ? Y - 1u + odd[ay] : odd[ay];
                const uint32_t iz = odd[az] < 2 ? Z - 1u + odd[az] : odd[az];
                GradCorners c;
                grad_corners(ix, iy, iz, 0.25f, 0.5f, 0.75f, X, Y, Z, c);
                float wsum = 0.0f;
                for (int k = 0; k < 8; ++k) { probe[c.idx[k]] += c.w[k]; wsum += c.w[k]; }
                if (!(fabsf(wsum - 1.0f) < 1e-6f)) { ++failed; printf("FAILED: corner weights sum to %g\n", wsum); }
            }
            free(probe);
        }
        printf("case %d samples %zu events %zu", ci - 1, n, events);
        for (int m = 0; m < 4; ++m) {
            double sum = 0.0, abs = 0.0, dot = 0.0;
            if (gv[m]) for (size_t i = 0; i < nvox; ++i) { sum += gv[m][i]; abs += fabs(gv[m][i]); dot += gv[m][i] * (double)((i * 2654435761u) % 1021u); }
            printf(" vol%d %.17g %.17g %.17g", m, sum, abs, dot);
            free(gv[m]);
        }
        printf(" tf %.17g %.17g %.17g %.17g\n", tfsum[0], tfsum[1], tfsum[2], tfsum[3]);
    }
    printf("brats_grad_harness: %d cases, %d failed\n", argc - 1, failed);
    return failed == 0 ? 0 : 1;
}
