// The K4 traversal (csrc/mesh_trace.h, the code the kernel runs) on the CPU under AddressSanitizer + UBSan, over a valid tree
// and over malformed buffers: child indices out of range, negative and huge leaf counts, a triangle index >= vertCount, a
// cycle (through the stack bound and through the pop bound), a stack shallower than the tree, NaN boxes and NaN indices.
// Every buffer is a heap allocation of exactly its count (and the stack exactly its capacity), so a read or write past one
// is an ASan report.  Each ray must end; on the malformed inputs the fault status must be raised.  Malformed buffers are
// exercised here only, never on the GPU.
//
//   mesh_harness <nodes.bin> <tris.bin> <verts.bin> <depth>     (float32 [N][8], uint32 [M][4], float32 [V][4])
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mri-raytracer_amd/csrc/mesh_trace.h"

using namespace mrirt;

struct HostStack {
    std::vector<uint32_t> v;
    explicit HostStack(uint32_t cap) : v(cap) {}
    uint32_t get(uint32_t i) const { return v.at(i); }
    void set(uint32_t i, uint32_t x) { v.at(i) = x; }
};

template <class T>
static std::vector<T> load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v(n / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

struct Buffers {
    std::vector<float4> nodes;     // 2 per node
    std::vector<uint4> tris;
    std::vector<float4> verts;
    MeshBufs view() const {
        MeshBufs m;
        m.nodes = nodes.data(); m.tris = tris.data(); m.verts = verts.data();
        m.nodeCount = (uint32_t)(nodes.size() / 2); m.triCount = (uint32_t)tris.size(); m.vertCount = (uint32_t)verts.size();
        return m;
    }
};

static int g_checks = 0, g_failed = 0;
static void check(bool ok, const char* what) {
    ++g_checks;
    if (!ok) { ++g_failed; printf("FAILED: %s\n", what); }
}

// rays from eyes around and inside the unit box toward points in it (deterministic)
static std::vector<MeshRay> rays() {
    std::vector<MeshRay> out;
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f * 2.0f - 1.0f; };
    const float eyes[4][3] = { { 1.1f, 0.9f, 1.6f }, { 0.05f, 0.03f, 0.02f }, { 0.0f, 0.0f, 2.5f }, { 2.0f, 0.05f, 0.0008f } };
    for (int e = 0; e < 4; ++e)
        for (int i = 0; i < 300; ++i) {
            MeshRay r;
            float d[3];
            for (int k = 0; k < 3; ++k) { r.o[k] = eyes[e][k]; d[k] = 0.6f * rnd() - eyes[e][k]; }
            if (i == 0) { d[0] = 0.0f; d[1] = 0.0f; d[2] = -1.0f; }      // axis-aligned: the 1e-8 clamp
            normalize3(d[0], d[1], d[2]);
            for (int k = 0; k < 3; ++k) r.d[k] = d[k];
            mesh_ray_setup(r);
            out.push_back(r);
        }
    return out;
}

struct Tally { int faults = 0, hits = 0, rays = 0; uint64_t pops = 0; };

static Tally walk(const Buffers& b, uint32_t cap) {
    Tally t;
    const MeshBufs m = b.view();
    for (const MeshRay& r : rays()) {
        HostStack st(cap);
        MeshHit h;
        const int rc = mesh_trace(m, r, st, cap, h);
        ++t.rays;
        t.pops += h.pops;
        if (rc != MESH_TRACE_OK) ++t.faults;
        else if (h.t < 1e29f) {
            ++t.hits;
            if (h.tri >= m.triCount) { check(false, "hit triangle index in range"); }
        }
        if (h.pops > m.nodeCount) check(false, "pops bounded by nodeCount");
    }
    return t;
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: mesh_harness nodes.bin tris.bin verts.bin depth\n"); return 2; }
    Buffers valid;
    valid.nodes = load<float4>(argv[1]);
    valid.tris = load<uint4>(argv[2]);
    valid.verts = load<float4>(argv[3]);
    const uint32_t depth = (uint32_t)atoi(argv[4]);
    const uint32_t N = (uint32_t)(valid.nodes.size() / 2), M = (uint32_t)valid.tris.size(), V = (uint32_t)valid.verts.size();

    Tally t = walk(valid, depth);
    printf("valid tree: %d rays, %d hits, %d faults, %llu pops\n", t.rays, t.hits, t.faults, (unsigned long long)t.pops);
    check(t.faults == 0 && t.hits > 0, "valid tree: no fault, some hits");

    auto faulting = [&](const char* what, const Buffers& b, uint32_t cap) {
        Tally f = walk(b, cap);
        printf("%-34s %d of %d rays stopped with the fault status\n", what, f.faults, f.rays);
        check(f.faults > 0, what);
    };
    const size_t root = 1;                                   // second float4 of node 0: (max.yz, leftFirst, countOrRight)
    { Buffers b = valid; b.nodes[root].z = (float)N; faulting("left child out of range", b, depth); }
    { Buffers b = valid; b.nodes[root].w = -(float)(N + 5); faulting("right child out of range", b, depth); }
    { Buffers b = valid; b.nodes[root].w = -1.0e9f; faulting("negative count (child 1e9 - 1)", b, depth); }
    { Buffers b = valid; b.nodes[root].w = 0.0f; faulting("inner node with count 0", b, depth); }
    { Buffers b = valid; b.nodes[root].z = 0.0f; b.nodes[root].w = 1.0e9f; faulting("huge leaf count", b, depth); }
    { Buffers b = valid; b.nodes[root].z = (float)M; b.nodes[root].w = 1.0f; faulting("leaf range past the triangles", b, depth); }
    { Buffers b = valid; for (auto& x : b.tris) x.y = V; faulting("triangle index >= vertCount", b, depth); }
    { Buffers b = valid; b.nodes[root].z = 0.0f; faulting("cycle to the root (stack bound)", b, depth); }
    { Buffers b = valid; b.nodes[root].z = NAN; faulting("NaN index", b, depth); }
    { Buffers b = valid; b.nodes[root].z = INFINITY; faulting("infinite index", b, depth); }
    if (depth > 1) faulting("tree deeper than the stack", valid, depth - 1);
    {
        // a cycle that keeps the stack at one entry: 0 -> 1 -> 0 -> ..., node 2's box far away (never pushed)
        Buffers b;
        b.nodes.assign(6, make_float4(0, 0, 0, 0));
        for (int n = 0; n < 2; ++n) { b.nodes[2 * n] = make_float4(-2, -2, -2, 2); b.nodes[2 * n + 1] = make_float4(2, 2, 0, 0); }
        b.nodes[2 * 2] = make_float4(50, 50, 50, 51); b.nodes[2 * 2 + 1] = make_float4(51, 51, 0, 1);
        b.nodes[1].z = 1.0f; b.nodes[1].w = -3.0f;                // root: left 1, right 2
        b.nodes[3].z = 0.0f; b.nodes[3].w = -3.0f;                // node 1: left 0 (the root), right 2
        b.tris.assign(1, make_uint4(0, 1, 2, 0));
        b.verts.assign(3, make_float4(0, 0, 0, 1));
        faulting("cycle at constant stack (pop bound)", b, 8);
    }
    {
        // NaN boxes everywhere below the root: every ray ends, nothing is read out of range
        Buffers b = valid;
        for (uint32_t n = 1; n < N; ++n) { b.nodes[2 * n] = make_float4(NAN, NAN, NAN, NAN); b.nodes[2 * n + 1].x = NAN; b.nodes[2 * n + 1].y = NAN; }
        Tally f = walk(b, depth);
        printf("%-34s %d rays ended, %d faults\n", "NaN boxes", f.rays, f.faults);
        check(f.rays > 0 && f.hits == 0, "NaN boxes: rays end without hits");
    }
    printf("mesh_harness: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
