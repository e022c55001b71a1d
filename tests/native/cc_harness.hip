// The connected components' per-thread text (csrc/cc_index.h, the code the kernels run) on the CPU under AddressSanitizer +
// UBSan: the sequence of mrirt_cc_label — the local pass tile by tile with the 256 "threads" of a tile run one after the
// other between the barriers, the merge, the flatten, the root counts level by level, the three numbering passes — then
// mrirt_cc_sizes, mrirt_cc_filter and mrirt_slice_counts, with the parent array exactly the volume long, the scratch exactly
// cc_plan(...).total bytes, every tile a heap allocation of exactly its size and the sizes exactly N long, so a read or
// write past one is an ASan report.
//
//   cc_harness <cases.bin> <out.bin>
//     cases.bin: uint32 count, then per case uint32 n0 n1 n2 classMask connectivity minVoxels keepLargest, int32 fill,
//                int16 labels[n0*n1*n2]
//     out.bin:   per case int64 scratchBytes, int64 N, int32 components[n0*n1*n2], int32 sizes[N], int16 filtered[n0*n1*n2],
//                int64 counts[n2][3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mri-raytracer_amd/csrc/cc_index.h"

using namespace mrirt;

template <class T>
static void rd(FILE* f, T* dst, size_t n) {
    if (n != 0 && fread(dst, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}

template <class T>
static void wr(FILE* f, const T* src, size_t n) {
    if (n != 0 && fwrite(src, sizeof(T), n, f) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: cc_harness cases.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t count = 0;
    rd(f, &count, 1);
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t hdr[7];
        int32_t fill;
        rd(f, hdr, 7);
        rd(f, &fill, 1);
        const uint32_t classMask = hdr[3], connectivity = hdr[4], keepLargest = hdr[6];
        const int64_t minVoxels = hdr[5];
        CcPlan p;
        if (cc_plan(hdr, &p) != 0 || connectivity < 1 || connectivity > 3) { printf("FAILED: case %u rejected\n", k); return 1; }
        const CcGeom& g = p.g;
        std::vector<int16_t> labels(g.total);
        rd(f, labels.data(), labels.size());
        std::vector<int32_t> parent(g.total);
        char* scratch = new char[(size_t)p.total];
        uint32_t* level[kCcMaxLevels];
        for (uint32_t l = 0; l < p.levels; ++l) level[l] = reinterpret_cast<uint32_t*>(scratch + p.level[l]);

        // local pass
        for (uint32_t tileId = 0; tileId < g.numTiles; ++tileId) {
            std::vector<int32_t> tile(kCcTileVox);
            std::vector<int32_t> roots((size_t)kCcThreads * kCcPerThread);
            uint32_t org[3];
            cc_tile_origin(g, tileId, org);
            for (uint32_t t = 0; t < kCcThreads; ++t) cc_tile_load(g, labels.data(), classMask, org, tile.data(), t);
            for (uint32_t t = 0; t < kCcThreads; ++t) cc_tile_link(connectivity, tile.data(), t);
            for (uint32_t t = 0; t < kCcThreads; ++t) cc_tile_roots(tile.data(), t, roots.data() + (size_t)t * kCcPerThread);
            for (uint32_t t = 0; t < kCcThreads; ++t) cc_tile_store(g, org, roots.data() + (size_t)t * kCcPerThread, parent.data(), t);
        }
        // merge, flatten
        for (uint32_t tileId = 0; tileId < g.numTiles; ++tileId) {
            uint32_t org[3];
            cc_tile_origin(g, tileId, org);
            for (uint32_t t = 0; t < kCcThreads; ++t) cc_merge_thread(g, connectivity, org, parent.data(), t);
        }
        for (uint32_t i = 0; i < g.total; ++i) cc_flatten_element(parent.data(), i);
        // root counts upwards, the scans downwards
        for (uint32_t chunk = 0; chunk < p.count[0]; ++chunk) {
            uint32_t s = 0;
            for (uint32_t i = chunk * kCcChunk; i < (chunk + 1) * kCcChunk && i < g.total; ++i) s += cc_is_root(parent.data(), i);
            level[0][chunk] = s;
        }
        for (uint32_t l = 1; l < p.levels; ++l)
            for (uint32_t chunk = 0; chunk < p.count[l]; ++chunk) {
                uint32_t s = 0;
                for (uint32_t i = chunk * kCcChunk; i < (chunk + 1) * kCcChunk && i < p.count[l - 1]; ++i) s += level[l - 1][i];
                level[l][chunk] = s;
            }
        if (p.count[p.levels - 1] > kCcChunk) { printf("FAILED: the top level does not fit one chunk\n"); return 1; }
        int64_t N = 0;
        for (uint32_t l = p.levels; l-- > 0;)
            for (uint32_t chunk = 0; chunk * kCcChunk < p.count[l]; ++chunk) {
                uint32_t run = l + 1 < p.levels ? level[l + 1][chunk] : 0u;
                for (uint32_t i = chunk * kCcChunk; i < (chunk + 1) * kCcChunk && i < p.count[l]; ++i) {
                    const uint32_t item = level[l][i];
                    level[l][i] = run;
                    run += item;
                }
                if (l + 1 == p.levels) N = run;
            }
        // number
        for (uint32_t chunk = 0; chunk < p.count[0]; ++chunk) {
            uint32_t num = level[0][chunk];
            for (uint32_t i = chunk * kCcChunk; i < (chunk + 1) * kCcChunk && i < g.total; ++i)
                if (cc_is_root(parent.data(), i)) parent[i] = cc_encode_number(++num);
        }
        for (uint32_t i = 0; i < g.total; ++i) cc_spread_element(parent.data(), i);
        for (uint32_t i = 0; i < g.total; ++i) cc_flip_element(parent.data(), i);
        // sizes, filter, slice counts
        std::vector<int32_t> sizes((size_t)N, 0);
        for (uint32_t group = 0; group * kCcSizeChunks < p.count[0]; ++group) {
            std::vector<int32_t> tags(kCcSizeSlots, 0), slots(kCcSizeSlots, 0);
            for (uint32_t t = 0; t < kCcThreads; ++t)
                for (uint32_t q = 0; q < kCcSizeChunks; ++q) {
                    const uint32_t chunk = group * kCcSizeChunks + q;
                    if (chunk < p.count[0])
                        cc_sizes_thread(parent.data(), g.total, N, tags.data(), slots.data(), sizes.data(), chunk * kCcChunk + t * kCcItems);
                }
            for (uint32_t t = 0; t < kCcSizeSlots; ++t) cc_sizes_flush(tags.data(), slots.data(), sizes.data(), t);
        }
        unsigned long long best = 0;
        if (keepLargest)
            for (int64_t c = 0; c < N; ++c) {
                const unsigned long long key = cc_size_key(sizes[(size_t)c], (uint32_t)c);
                best = key > best ? key : best;
            }
        std::vector<int16_t> filtered(g.total);
        for (uint32_t i = 0; i < g.total; ++i)
            filtered[i] = cc_filter_value(labels[i], parent[i], sizes.data(), N, minVoxels, keepLargest, best, (int16_t)fill);
        std::vector<int64_t> counts((size_t)g.n[2] * 3, 0);
        for (uint32_t row = 0; row < g.n[0] * g.n[1]; ++row)
            for (uint32_t z = 0; z < g.n[2]; ++z) {
                const uint32_t v = row * g.n[2] + z;
                const uint32_t fl = cc_slice_flags(labels[v], z > 0 ? labels[v - 1] : (int16_t)0, z > 0);
                counts[(size_t)z * 3 + 0] += fl & 1u;
                counts[(size_t)z * 3 + 1] += (fl >> 1) & 1u;
                counts[(size_t)z * 3 + 2] += fl >> 2;
            }
        const int64_t head[2] = { p.total, N };
        wr(o, head, 2);
        wr(o, parent.data(), parent.size());
        wr(o, sizes.data(), sizes.size());
        wr(o, filtered.data(), filtered.size());
        wr(o, counts.data(), counts.size());
        printf("case %u scratch %lld levels %u N %lld\n", k, (long long)p.total, p.levels, (long long)N);
        delete[] scratch;
    }
    fclose(f);
    if (fclose(o) != 0) { fprintf(stderr, "cannot close the output\n"); return 2; }
    printf("cc_harness: %u cases done\n", count);
    return 0;
}
