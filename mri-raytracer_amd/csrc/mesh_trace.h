// K4 traversal core: the BVH walk of bvhTrace, scripts/mesh_rt/mesh_rt.slang:39-136, written once for the device kernel
// (csrc/mesh_rt.hip) and for the host (tests/native/mesh_harness.hip walks it under AddressSanitizer + UBSan over valid and
// malformed buffers).  Unfused fp32 in the shader's order (compiled with -ffp-contract=off).
//
// What the shader decides, this decides: the same nodes popped and culled in the same order, the same triangles tested, the
// same winner among equal t.  What it adds is a guard on every index the buffers hold — node and triangle indices decoded
// out of range, a stack deeper than its capacity, or more pops than there are nodes (a cycle; a tree pops each node at
// most once per ray) stop the ray with MESH_TRACE_FAULT instead of reading out of bounds or spinning.
#pragma once
#include "mrirt_device.h"

namespace mrirt {

constexpr uint32_t kMeshMaxStack = 64;          // the shader's uint stack[64]; the launch sizes its stack from the tree's depth

struct MeshBufs {
    const float4* nodes;        // 2 per node: (min.xyz, max.x), (max.yz, leftFirst, triCountOrRight)
    const uint4* tris;          // xyz = vertex indices
    const float4* verts;        // xyz = position
    uint32_t nodeCount, triCount, vertCount;
};

struct MeshRay {
    float o[3], d[3];
    float rcp[3];               // 1 / d, each component first pushed away from 0 to +-1e-8 (:78-82)
};

enum MeshTraceStatus { MESH_TRACE_OK = 0, MESH_TRACE_FAULT = 1 };

MRIRT_HD void mesh_ray_setup(MeshRay& r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float dd = r.d[k];
        if (fabsf(dd) < 1e-8f) dd = (dd >= 0.0f) ? 1e-8f : -1e-8f;
        r.rcp[k] = 1.0f / dd;
    }
}

// aabbHit, :39-49 (HLSL min / max return the other operand of a NaN, as fminf / fmaxf)
MRIRT_HD bool mesh_aabb_hit(const MeshRay& r, const float4& a, const float4& b, float& tmin) {
    const float bmin[3] = { a.x, a.y, a.z }, bmax[3] = { a.w, b.x, b.y };
    float tsm[3], tbg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t0 = (bmin[k] - r.o[k]) * r.rcp[k];
        const float t1 = (bmax[k] - r.o[k]) * r.rcp[k];
        tsm[k] = fminf(t0, t1);
        tbg[k] = fmaxf(t0, t1);
    }
    const float tN = fmaxf(fmaxf(tsm[0], tsm[1]), tsm[2]);
    const float tF = fminf(fminf(tbg[0], tbg[1]), tbg[2]);
    tmin = tN;
    return tF >= fmaxf(tN, 0.0f);
}

MRIRT_HD void mesh_cross(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// triHit, :51-71, without the normal: it is a function of the triangle alone, so the kernel forms it once, for the winner
MRIRT_HD bool mesh_tri_hit(const MeshRay& r, const float4& A, const float4& B, const float4& Cv, float& t) {
    const float ab[3] = { B.x - A.x, B.y - A.y, B.z - A.z };
    const float ac[3] = { Cv.x - A.x, Cv.y - A.y, Cv.z - A.z };
    float p[3];
    mesh_cross(r.d, ac, p);
    const float det = dot3(ab[0], ab[1], ab[2], p[0], p[1], p[2]);
    if (fabsf(det) < 1e-8f) return false;
    const float invDet = 1.0f / det;
    const float s[3] = { r.o[0] - A.x, r.o[1] - A.y, r.o[2] - A.z };
    const float u = dot3(s[0], s[1], s[2], p[0], p[1], p[2]) * invDet;
    if (u < 0.0f || u > 1.0f) return false;
    float q[3];
    mesh_cross(s, ab, q);
    const float v = dot3(r.d[0], r.d[1], r.d[2], q[0], q[1], q[2]) * invDet;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float th = dot3(ac[0], ac[1], ac[2], q[0], q[1], q[2]) * invDet;
    if (th <= 1e-5f) return false;
    t = th;
    return true;
}

// int(b.z + 0.5) and int(b.w +- 0.5) (:96-97), refusing what has no int value (NaN, out of range) instead of converting it
MRIRT_HD bool mesh_decode(const float4& b, int64_t& leftFirst, int64_t& countOrRight) {
    const float x = b.z + 0.5f;
    const float y = b.w + (b.w >= 0.0f ? 0.5f : -0.5f);
    if (!(x > -1.0f && x < 2147483648.0f)) return false;
    if (!(y > -2147483648.0f && y < 2147483648.0f)) return false;
    leftFirst = (int64_t)(int32_t)x;
    countOrRight = (int64_t)(int32_t)y;
    return true;
}

struct MeshHit {
    float t;
    uint32_t tri;               // index into tris of the nearest hit, 0xffffffff for none
    uint32_t pops, tests;       // nodes popped, triangles tested
};

// bvhTrace, :75-136.  Stack: get(i) / set(i, v) over cap >= 1 entries (cap <= kMeshMaxStack).
template <class Stack>
MRIRT_HD int mesh_trace(const MeshBufs& m, const MeshRay& r, Stack& st, uint32_t cap, MeshHit& h) {
    h.t = 1e30f; h.tri = 0xffffffffu; h.pops = 0; h.tests = 0;
    if (m.nodeCount == 0 || cap == 0) return MESH_TRACE_FAULT;
    uint32_t sp = 0;
    st.set(sp++, 0u);                                            // root at 0
    while (sp > 0) {
        const uint32_t ni = st.get(--sp);                        // < nodeCount: only checked indices are pushed
        if (h.pops >= m.nodeCount) return MESH_TRACE_FAULT;      // a cycle
        ++h.pops;
        const float4 a = m.nodes[2u * ni], b = m.nodes[2u * ni + 1u];
        float tmin;
        if (!mesh_aabb_hit(r, a, b, tmin) || tmin > h.t) continue;
        int64_t lf, cr;
        if (!mesh_decode(b, lf, cr)) return MESH_TRACE_FAULT;
        if (cr > 0) {
            // leaf: triangles [lf, lf + cr)
            if (lf + cr > (int64_t)m.triCount) return MESH_TRACE_FAULT;
            const uint32_t start = (uint32_t)lf, count = (uint32_t)cr;
            for (uint32_t i = 0; i < count; ++i) {
                const uint32_t ti = start + i;
                const uint4 idx = m.tris[ti];
                if (idx.x >= m.vertCount || idx.y >= m.vertCount || idx.z >= m.vertCount) return MESH_TRACE_FAULT;
                ++h.tests;
                float t;
                if (mesh_tri_hit(r, m.verts[idx.x], m.verts[idx.y], m.verts[idx.z], t) && t < h.t) { h.t = t; h.tri = ti; }
            }
        } else {
            // inner: left = lf, right = -cr - 1
            const int64_t rr = -cr - 1;
            if (lf >= (int64_t)m.nodeCount || rr < 0 || rr >= (int64_t)m.nodeCount) return MESH_TRACE_FAULT;
            const uint32_t l = (uint32_t)lf, rc = (uint32_t)rr;
            const float4 al = m.nodes[2u * l], bl = m.nodes[2u * l + 1u];
            const float4 ar = m.nodes[2u * rc], br = m.nodes[2u * rc + 1u];
            float tl, tr;
            const bool hl = mesh_aabb_hit(r, al, bl, tl);
            const bool hr = mesh_aabb_hit(r, ar, br, tr);
            const uint32_t need = (hl ? 1u : 0u) + (hr ? 1u : 0u);
            if (sp + need > cap) return MESH_TRACE_FAULT;        // deeper than the stack the launch was sized for
            if (hl && hr) {
                if (tl < tr) { st.set(sp++, rc); st.set(sp++, l); }
                else         { st.set(sp++, l); st.set(sp++, rc); }
            } else if (hl) {
                st.set(sp++, l);
            } else if (hr) {
                st.set(sp++, rc);
            }
        }
    }
    return MESH_TRACE_OK;
}

}  // namespace mrirt
