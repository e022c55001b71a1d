// The index arithmetic of the case preparation (csrc/prep_index.h) walked on the CPU, built host-only under
// AddressSanitizer + UBSan by tests/test_prep_host.py.  Reads commands from the file named on the command line, one per line,
// and answers each with one line that the test compares with tests/prep_ref.py:
//   K bits(hex)                         -> K key(hex) inverse(hex)
//   P n q(bits, hex)                    -> P k g(bits, hex)
//   S rank c0 .. c255                   -> S bin remaining
//   A p0 p1 p2 p3                       -> A nslots s0 s1 s2 s3
//   R i n                               -> R m
//   W n                                 -> W blocks total
//   T d0 d1 d2 axis TO TL TI r          -> T tiles ok      every staged element's source lies inside the volume (it is READ
//                                          from a buffer exactly the volume's size) and every output is written exactly once
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../mri-raytracer_amd/csrc/prep_index.h"

using namespace mrirt;

static int walk_tiles(const uint32_t dims[3], int axis, uint32_t TO, uint32_t TL, uint32_t TI, int r, long long* tilesOut) {
    const PrepLineGeom g = prep_line_geom(dims, axis, TO, TL, TI);
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<uint8_t> volume(n, 1), written(n, 0);           // exactly n long: a wrong index is an ASan report
    const uint32_t rows = TL + 2u * (uint32_t)r;
    if (rows > TL + 2u * kPrepMaxRadius) return 0;
    std::vector<uint8_t> stage((size_t)TO * rows * TI);
    int ok = 1;
    for (int64_t t = 0; t < g.tiles; ++t) {
        int64_t o0, l0, i0;
        prep_tile_origin(g, t, TO, TL, TI, &o0, &l0, &i0);
        for (uint32_t e = 0; e < TO * rows * TI; ++e) {
            uint32_t o, l, i;
            prep_stage_coords(e, rows, TI, &o, &l, &i);
            uint8_t v = 0;
            if (o0 + o < g.outer && i0 + i < g.inner) {
                const int64_t src = prep_reflect(l0 + (int64_t)l - r, g.len);
                if (src < 0 || src >= g.len) ok = 0;
                else v = volume[(size_t)(((o0 + o) * g.len + src) * g.inner + (i0 + i))];
            }
            stage[e] = v;
        }
        for (uint32_t e = 0; e < TO * TL * TI; ++e) {
            uint32_t o, l, i;
            prep_stage_coords(e, TL, TI, &o, &l, &i);
            if (o0 + o < g.outer && l0 + l < g.len && i0 + i < g.inner) {
                for (int j = -r; j <= r; ++j)
                    if (stage[((size_t)o * rows + (l + r + j)) * TI + i] != 1) ok = 0;      // every tap was staged from the volume
                written[(size_t)(((o0 + o) * g.len + (l0 + l)) * g.inner + (i0 + i))] += 1;
            }
        }
    }
    for (size_t k = 0; k < n; ++k)
        if (written[k] != 1) ok = 0;
    *tilesOut = (long long)g.tiles;
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: prep_harness commands.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char op;
    long long done = 0;
    while (fscanf(f, " %c", &op) == 1) {
        if (op == 'K') {
            unsigned bits;
            if (fscanf(f, "%x", &bits) != 1) return 3;
            const uint32_t k = prep_key(bits);
            printf("K %08x %08x\n", k, prep_key_inverse(k));
        } else if (op == 'P') {
            long long n; unsigned qb;
            if (fscanf(f, "%lld %x", &n, &qb) != 2) return 3;
            uint32_t k; float g;
            prep_rank(n, prep_u2f(qb), &k, &g);
            printf("P %u %08x\n", k, prep_f2u(g));
        } else if (op == 'S') {
            unsigned rank;
            std::vector<uint32_t> h(kPrepBins);
            if (fscanf(f, "%u", &rank) != 1) return 3;
            for (uint32_t b = 0; b < kPrepBins; ++b)
                if (fscanf(f, "%u", &h[b]) != 1) return 3;
            uint32_t rem;
            const uint32_t bin = prep_select_bin(h.data(), rank, &rem);
            printf("S %u %u\n", bin, rem);
        } else if (op == 'A') {
            uint32_t p[kPrepRanks], s[kPrepRanks];
            for (uint32_t r = 0; r < kPrepRanks; ++r)
                if (fscanf(f, "%u", &p[r]) != 1) return 3;
            const uint32_t ns = prep_assign_slots(p, s);
            printf("A %u %u %u %u %u\n", ns, s[0], s[1], s[2], s[3]);
        } else if (op == 'R') {
            long long i, n;
            if (fscanf(f, "%lld %lld", &i, &n) != 2) return 3;
            printf("R %lld\n", (long long)prep_reflect(i, n));
        } else if (op == 'W') {
            long long n;
            if (fscanf(f, "%lld", &n) != 1) return 3;
            PrepWindowPlan p;
            if (prep_window_plan(n, &p)) printf("W %u %lld\n", p.blocks, (long long)p.total);
            else printf("W 0 0\n");
        } else if (op == 'T') {
            uint32_t d[3], TO, TL, TI; int axis, r;
            if (fscanf(f, "%u %u %u %d %u %u %u %d", &d[0], &d[1], &d[2], &axis, &TO, &TL, &TI, &r) != 8) return 3;
            long long tiles = 0;
            const int ok = walk_tiles(d, axis, TO, TL, TI, r, &tiles);
            printf("T %lld %s\n", tiles, ok ? "ok" : "FAILED");
        } else {
            fprintf(stderr, "unknown command %c\n", op);
            return 3;
        }
        ++done;
    }
    fclose(f);
    printf("prep_harness: %lld commands done\n", done);
    return 0;
}
