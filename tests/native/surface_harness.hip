// The surface nets' per-thread text (csrc/surface_cells.h, the code the kernels run) on the CPU under AddressSanitizer +
// UBSan: the sequence of mrirt_surface_extract — classify tile by tile with the 256 "threads" of a tile run one after the
// other, the sums level by level, the vertices, the triangles — inside a scratch allocation of exactly surf_plan(...).total
// bytes, with every tile a heap allocation of exactly its size and the outputs exactly V and T long, so a read or write
// past one is an ASan report.  Prints, per case, the scratch size and the counts, then the vertex words and the triangles
// (cases of more than kPrintVerts vertices: a 64-bit FNV-1a hash of each array instead).
//
//   surface_harness <cases.bin>     cases.bin: uint32 count, then per case uint32 n0 n1 n2 classMask, float32 spacing[3],
//                                   float32 origin[3], int16 labels[n0*n1*n2]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/surface_cells.h"

using namespace mrirt;

constexpr uint64_t kPrintVerts = 2000;

template <class T>
static void rd(FILE* f, T* dst, size_t n) {
    if (fread(dst, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}

static uint64_t fnv(const void* p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: surface_harness cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t count = 0;
    rd(f, &count, 1);
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t hdr[4];
        float spacing[3], origin[3];
        rd(f, hdr, 4);
        rd(f, spacing, 3);
        rd(f, origin, 3);
        SurfPlan p;
        if (surf_plan(hdr, &p) != 0 || surf_check_frame(spacing, origin) != 0) { printf("FAILED: case %u rejected\n", k); return 1; }
        const SurfGeom& g = p.g;
        std::vector<int16_t> labels((size_t)hdr[0] * hdr[1] * hdr[2]);
        rd(f, labels.data(), labels.size());
        char* scratch = new char[(size_t)p.total];
        uint8_t* code = reinterpret_cast<uint8_t*>(scratch + p.code);
        uint32_t* vidx = reinterpret_cast<uint32_t*>(scratch + p.vidx);
        SurfCount* level[kSurfMaxLevels];
        for (uint32_t l = 0; l < p.levels; ++l) level[l] = reinterpret_cast<SurfCount*>(scratch + p.level[l]);

        // classify
        const uint32_t tiles = g.tiles[0] * g.tiles[1] * g.tiles[2];
        for (uint32_t tileId = 0; tileId < tiles; ++tileId) {
            std::vector<uint8_t> tile(kSurfTileBytes);
            uint32_t o[3];
            surf_tile_origin(g, tileId, o);
            for (uint32_t t = 0; t < kSurfThreads; ++t) surf_tile_load(g, labels.data(), hdr[3], o, tile.data(), t, kSurfThreads);
            for (uint32_t t = 0; t < kSurfThreads; ++t) surf_tile_classify(g, o, tile.data(), code, t);
        }
        // sums upwards, the top level's scan, the scans downwards
        for (uint32_t chunk = 0; chunk < p.count[0]; ++chunk) {
            SurfCount s{ 0, 0 };
            for (uint32_t i = 0; i < kSurfChunk && chunk * kSurfChunk + i < g.cells; ++i) {
                const uint32_t cell = chunk * kSurfChunk + i;
                uint32_t c[3];
                surf_cell_coords(g, cell, c);
                const uint32_t packed = surf_cell_counts(code[cell], c);
                s = s + SurfCount{ packed & 0xFFFFu, packed >> 16 };
            }
            level[0][chunk] = s;
        }
        for (uint32_t l = 1; l < p.levels; ++l)
            for (uint32_t chunk = 0; chunk < p.count[l]; ++chunk) {
                SurfCount s{ 0, 0 };
                for (uint32_t i = 0; i < kSurfChunk && chunk * kSurfChunk + i < p.count[l - 1]; ++i) s = s + level[l - 1][chunk * kSurfChunk + i];
                level[l][chunk] = s;
            }
        if (p.count[p.levels - 1] > kSurfChunk) { printf("FAILED: the top level does not fit one chunk\n"); return 1; }
        SurfCount totals{ 0, 0 };
        for (uint32_t l = p.levels; l-- > 0;)
            for (uint32_t chunk = 0; chunk * kSurfChunk < p.count[l]; ++chunk) {
                SurfCount run = l + 1 < p.levels ? level[l + 1][chunk] : SurfCount{ 0, 0 };
                for (uint32_t i = 0; i < kSurfChunk && chunk * kSurfChunk + i < p.count[l]; ++i) {
                    const SurfCount item = level[l][chunk * kSurfChunk + i];
                    level[l][chunk * kSurfChunk + i] = run;
                    run = run + item;
                }
                if (l + 1 == p.levels) totals = run;
            }
        const uint64_t V = totals.v, T = 2 * totals.q;
        // emit
        std::vector<float> verts((size_t)V * 3);
        std::vector<int32_t> tris((size_t)T * 3);
        for (uint32_t chunk = 0; chunk < p.count[0]; ++chunk) {
            uint64_t v = level[0][chunk].v;
            for (uint32_t i = 0; i < kSurfChunk && chunk * kSurfChunk + i < g.cells; ++i) {
                const uint32_t cell = chunk * kSurfChunk + i;
                if (!surf_active(code[cell])) continue;
                uint32_t c[3];
                surf_cell_coords(g, cell, c);
                vidx[cell] = (uint32_t)v;
                surf_vertex(code[cell], c, spacing, origin, verts.data() + 3 * v);
                ++v;
            }
        }
        for (uint32_t chunk = 0; chunk < p.count[0]; ++chunk) {
            uint64_t q = level[0][chunk].q;
            for (uint32_t i = 0; i < kSurfChunk && chunk * kSurfChunk + i < g.cells; ++i) {
                const uint32_t cell = chunk * kSurfChunk + i;
                uint32_t c[3];
                surf_cell_coords(g, cell, c);
                const uint32_t axes = surf_quad_axes(code[cell], c);
                for (int a = 0; a < 3; ++a)
                    if ((axes >> a) & 1u) {
                        surf_quad(g, a, code[cell], cell, vidx, tris.data() + 6 * q);
                        ++q;
                    }
            }
        }
        printf("case %u scratch %lld levels %u V %llu T %llu\n", k, (long long)p.total, p.levels, (unsigned long long)V, (unsigned long long)T);
        if (V <= kPrintVerts) {
            printf("v");
            for (float x : verts) { uint32_t u; memcpy(&u, &x, 4); printf(" %08x", u); }
            printf("\nt");
            for (int32_t i : tris) printf(" %d", i);
            printf("\n");
        } else {
            printf("vhash %016llx\nthash %016llx\n", (unsigned long long)fnv(verts.data(), verts.size() * 4),
                   (unsigned long long)fnv(tris.data(), tris.size() * 4));
        }
        delete[] scratch;
    }
    fclose(f);
    printf("surface_harness: %u cases done\n", count);
    return 0;
}
