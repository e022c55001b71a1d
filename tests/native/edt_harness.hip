// The distance transform's per-thread text (csrc/edt_line.h, the code the kernels run) on the CPU under AddressSanitizer +
// UBSan: the sequence of mrirt_hausdorff — per class three line passes over F_T and F_P, a masked maximum, the finish —
// with the 256 "threads" of a tile run one after the other, inside a scratch allocation of exactly edt_scratch(...).total
// bytes and with every tile and coordinate table a heap allocation of exactly its size, so a read or write past one is an
// ASan report.  Prints, per case, the scratch size and the bits of every class's Hausdorff distance.
//
//   edt_harness <cases.bin>     cases.bin: uint32 count, then per case uint32 H W D numClasses, float32 spacing[3],
//                               int16 pred[H*W*D], int16 truth[H*W*D]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/edt_line.h"

using namespace mrirt;

template <class T>
static void rd(FILE* f, T* dst, size_t n) {
    if (fread(dst, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}

static void run_pass(const uint32_t hwd[3], int axis, float s, const int16_t* labels, int32_t cls, double* field) {
    const EdtPass p = edt_pass(hwd, axis, s);
    if (((uint64_t)p.n * p.tl + p.n) * sizeof(double) > kEdtTileBytes) { printf("FAILED: tile over the staging budget\n"); exit(1); }
    for (uint32_t o = 0; o < p.outer; ++o)
        for (uint32_t chunk = 0; chunk < p.chunks; ++chunk) {
            std::vector<double> tile((size_t)p.n * p.tl), ctab(p.n);
            for (uint32_t t = 0; t < kEdtThreads; ++t) edt_tile_load(p, o, chunk, field, labels, cls, tile.data(), ctab.data(), t, kEdtThreads);
            for (uint32_t t = 0; t < kEdtThreads; ++t) edt_tile_compute(p, o, chunk, tile.data(), ctab.data(), field, t, kEdtThreads);
        }
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: edt_harness cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t count = 0;
    rd(f, &count, 1);
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t hdr[4];
        float spacing[3];
        rd(f, hdr, 4);
        rd(f, spacing, 3);
        const uint32_t nc = hdr[3];
        if (edt_check_volume(hdr, spacing) != 0 || nc == 0 || nc > kEdtMaxClasses) { printf("FAILED: case %u rejected\n", k); return 1; }
        const int64_t voxels = (int64_t)hdr[0] * hdr[1] * hdr[2];
        std::vector<int16_t> pred((size_t)voxels), truth((size_t)voxels);
        rd(f, pred.data(), pred.size());
        rd(f, truth.data(), truth.size());
        const EdtScratch lay = edt_scratch(voxels, nc);
        char* scratch = new char[(size_t)lay.total];
        double* fT = reinterpret_cast<double*>(scratch + lay.field[0]);
        double* fP = reinterpret_cast<double*>(scratch + lay.field[1]);
        uint64_t* acc = reinterpret_cast<uint64_t*>(scratch + lay.acc);
        for (uint32_t w = 0; w < nc * kEdtAccWords; ++w) acc[w] = 0;
        for (uint32_t c = 0; c < nc; ++c) {
            for (int axis = 0; axis < 3; ++axis) {
                run_pass(hdr, axis, spacing[axis], axis == 0 ? truth.data() : nullptr, (int32_t)c, fT);
                run_pass(hdr, axis, spacing[axis], axis == 0 ? pred.data() : nullptr, (int32_t)c, fP);
            }
            uint64_t* a = acc + (size_t)c * kEdtAccWords;
            for (int64_t v = 0; v < voxels; ++v) {
                if (pred[v] == (int32_t)c) { const uint64_t b = edt_bits(fT[v]); if (b > a[0]) a[0] = b; a[2] = 1; }
                if (truth[v] == (int32_t)c) { const uint64_t b = edt_bits(fP[v]); if (b > a[1]) a[1] = b; a[3] = 1; }
            }
        }
        printf("case %u scratch %lld hd", k, (long long)lay.total);
        for (uint32_t c = 0; c < nc; ++c) {
            const uint64_t* a = acc + (size_t)c * kEdtAccWords;
            if (a[2] != 0 && a[3] != 0) {
                const double sq = edt_from_bits(a[0] > a[1] ? a[0] : a[1]);
                printf(" %016llx", (unsigned long long)edt_bits(sqrt(sq)));
            } else printf(" nan");
        }
        printf("\n");
        delete[] scratch;
    }
    fclose(f);
    printf("edt_harness: %u cases done\n", count);
    return 0;
}
